"""Drop-in replacement for the hot-path helpers of the reference `utils.py`.

Same function names, argument order, shapes, dtypes and return layouts as
Findeton/mpi-vision `utils.py` (citations below are `utils.py:line`).  The
per-pixel work of every helper runs in hand-written gfx950 HIP kernels in
`libmpiv.so` (C-ABI declared in `include/mpiv.h`); only the tiny 3x3/4x4
per-plane matrices are set up on the host, in torch-CPU fp32 with the
reference's own association order, because their bits decide the 1e-5 parity
(SURVEY.md §8a).

There is no CPU fallback: calling a compute helper without a ROCm device or
without the built library raises.
"""
from __future__ import annotations

import torch

from . import _host, _lib
from .camera import (deprocess_image_torch, make_intrinsics_matrix, parse_camera_lines,  # noqa: F401
                     preprocess_image_torch, read_file_lines, scale_intrinsics)

# The reference keeps a module-level device (utils.py:5).  Every helper reads it
# at call time, exactly like the reference does.
device = torch.device("cuda")


# ---------------------------------------------------------------------------
# Host-only helpers (pure Python / tiny matrices)
# ---------------------------------------------------------------------------

def inv_depths(start_depth, end_depth, num_depths):
    """Plane depths uniform in inverse depth, far->near (utils.py:297-318).

    Reproduces the reference's arithmetic exactly (same expression order), its
    quirk that num_depths < 2 still yields both end points, and its
    descending order."""
    inv_near = 1.0 / start_depth
    inv_far = 1.0 / end_depth
    out = [start_depth, end_depth]
    n_minus_1 = float(num_depths - 1)
    out.extend(1.0 / (inv_near + (inv_far - inv_near) * (float(i) / n_minus_1))
               for i in range(1, num_depths - 1))
    out.sort(reverse=True)
    return out


def meshgrid_abs_torch(batch, height, width):
    """[batch, 3, height, width] grid of (x, y, 1) (utils.py:18-33)."""
    xs = torch.arange(width, dtype=torch.float32).expand(height, width)
    ys = torch.arange(height, dtype=torch.float32).unsqueeze(1).expand(height, width)
    grid = torch.stack([xs, ys, torch.ones(height, width)], 0)
    return grid.unsqueeze(0).repeat(batch, 1, 1, 1).to(device)


def divide_safe_torch(num, den, name=None):
    """num / den with den == 0 replaced by 1e-8 (utils.py:35-39)."""
    return _host.divide_safe(num, den)


def transpose_torch(rot):
    """Swap the last two axes (utils.py:41-42)."""
    return rot.transpose(-2, -1)


def inv_homography_torch(k_s, k_t, rot, t, n_hat, a):
    """Plane-induced target->source homography K_s (R^T + R^T t n R^T / (a - n R^T t)) K_t^-1
    (utils.py:44-67).  Tiny [...,3,3] math, evaluated on the host in torch-CPU fp32
    in the reference's op order (materialised operands, like the reference's
    repeats), and returned on the inputs' device."""
    dev = k_s.device
    host = [_host._cpu32(x).contiguous() for x in (k_s, k_t, rot, t, n_hat, a)]
    return _host.inv_homography(*host).to(dev)


# ---------------------------------------------------------------------------
# Device helpers (HIP kernels)
# ---------------------------------------------------------------------------

def transform_points_torch(points, homography):
    """points [..., H, W, 3] @ homography^T (utils.py:69-88), on the GPU."""
    return _lib.transform_points(points, homography)


def normalize_homogeneous_torch(points):
    """uv / w with w == 0 -> 1e-8 (utils.py:90-101), on the GPU."""
    return _lib.normalize_homogeneous(points)


def bilinear_wrapper_torch(imgs, coords):
    """grid_sample(bilinear, zeros, align_corners=False) of imgs [..., H_s, W_s, C] at
    coords [..., H_t, W_t, 2] in [0,1] (x first).  Returns [..., C, H_t, W_t] like the
    reference (utils.py:104-134).  Differentiable w.r.t. imgs and coords (HIP adjoint, ATen's CPU
    grid_sampler_2d_backward bits); no double backward."""
    return _lib.bilinear_sample(imgs, coords, channels_last_out=False)


def resampler_wrapper_torch(imgs, coords):
    """grid_sample of NHWC imgs at coords [N, H', W', 2] -> [N, H', W', C] (utils.py:395-407).
    Differentiable w.r.t. imgs and coords, as bilinear_wrapper_torch."""
    return _lib.bilinear_sample(imgs, coords, channels_last_out=True)


def over_composite(rgbas):
    """Back-to-front over-compositing of a list of [B,H,W,4] images; the first image's
    alpha is ignored (utils.py:136-157).  Differentiable w.r.t. every layer (HIP adjoint, the
    reference's CPU autograd bits); raises under a HIP-graph capture (host pointer table)."""
    return _lib.over_composite(rgbas)


def transform_plane_imgs_torch(imgs, pixel_coords_trg, k_s, k_t, rot, t, n_hat, a):
    """Warp [..., H_s, W_s, C] plane images with per-plane homographies; returns
    [..., C, H_t, W_t] (utils.py:160-195, including its x/(H-1), y/(W-1) normalisation).
    Differentiable w.r.t. imgs (the sampler's HIP adjoint).  The camera arguments (k_s, k_t, rot, t,
    n_hat, a) and pixel_coords_trg are not differentiable here: for camera gradients use
    mpi_render_view_torch."""
    hom = inv_homography_torch(k_s, k_t, rot, t, n_hat, a)
    return _lib.warp_planes(imgs, pixel_coords_trg, hom)


def planar_transform_torch(imgs, pixel_coords_trg, k_s, k_t, rot, t, n_hat, a):
    """Layer-batched planar transform (utils.py:198-233): imgs [L, B, H, W, C],
    per-batch cameras, per-layer planes -> [L, B, C, H_t, W_t].  Differentiable w.r.t. imgs only
    (camera gradients: mpi_render_view_torch)."""
    n_layers = imgs.shape[0]

    def rep(x):
        return x.unsqueeze(0).repeat((n_layers,) + (1,) * x.dim())

    return transform_plane_imgs_torch(imgs, rep(pixel_coords_trg), rep(k_s), rep(k_t),
                                      rep(rot), rep(t), n_hat, a)


def projective_forward_homography_torch(src_images, intrinsics, pose, depths):
    """Forward-warp [L, B, H, W, C] layers to the target pose (utils.py:237-265);
    returns [L, B, C, H, W].  Differentiable w.r.t. src_images only (camera gradients:
    mpi_render_view_torch)."""
    n_layers, n_batch, height, width, _ = src_images.shape
    rot, t = pose[:, :3, :3], pose[:, :3, 3:]
    n_hat = torch.tensor([0.0, 0.0, 1.0], device=pose.device).reshape(1, 1, 1, 3)
    n_hat = n_hat.repeat(n_layers, n_batch, 1, 1)
    a = -depths.reshape(n_layers, n_batch, 1, 1)
    grid = meshgrid_abs_torch(n_batch, height, width).permute(0, 2, 3, 1)
    return planar_transform_torch(src_images, grid, intrinsics, intrinsics, rot, t, n_hat, a)


def _camera_grad(tgt_pose, planes, intrinsics) -> bool:
    """True when the caller asks for a gradient w.r.t. the camera: the render then takes the
    autograd homography chain; otherwise nothing changes."""
    return torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad
                                           for x in (tgt_pose, planes, intrinsics))


def mpi_render_view_torch(rgba_layers, tgt_pose, planes, intrinsics):
    """Render [B, H, W, 3] target views from an MPI [B, H, W, P, 4] (utils.py:267-294).

    `planes` must be a tensor of P depths, far->near (a list raises AttributeError,
    as in the reference, utils.py:279).  The whole warp + over-composite runs as ONE
    fused HIP kernel; the MPI may be a stride-0 broadcast over the batch.  When
    rgba_layers requires grad the result is differentiable w.r.t. it (HIP backward,
    bit-exact to the reference's autograd).  When tgt_pose, planes or intrinsics requires grad it
    is differentiable w.r.t. them too, as in the reference: d frame / d homographies in HIP
    (render_bwd_cam.hip), the 3x3 chain behind it in torch on the host
    (_host.render_homographies_autograd: one device-to-host copy of the pose per call)."""
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])  # AttributeError on a list, like the reference
    if rgba_layers.is_cuda and _camera_grad(tgt_pose, planes, intrinsics):
        homs = _host.render_homographies_autograd(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
        # (device homographies into the Function: autograd's copy node carries their gradient back)
        return _lib.RenderFunction.apply(rgba_layers, homs.to(rgba_layers.device))
    if tgt_pose.is_cuda and rgba_layers.is_cuda:  # poses in HBM: the chain runs there too
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    else:
        if rgba_layers.is_cuda:
            _lib.host_under_capture("tgt_pose")  # host poses cannot be part of a captured HIP graph
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), intrinsics, batch_size,
                                         pin=rgba_layers.is_cuda)
    if torch.is_grad_enabled() and rgba_layers.requires_grad:
        # training (ipynb cell 12): the adjoint runs in HIP too, bit-exact to the
        # reference's autograd (render_bwd.hip)
        return _lib.RenderFunction.apply(rgba_layers, homs)
    return _lib.render(rgba_layers, homs)


def mpi_render_view_u8(rgba_layers_u8, tgt_pose, planes, intrinsics):
    """mpi_render_view_torch for an 8-bit MPI [B, H, W, P, 4] uint8 (the reference's own
    test-MPI format, test/rgba_*.png): returns exactly
    mpi_render_view_torch(rgba_layers_u8.float() / 255.0, tgt_pose, planes, intrinsics)
    (the reference's image convention, utils.py:324-331) without the float copy: each
    view is packed at 4 B per texel and rendered by render_texel.hip, which converts every
    tap to RN(u8/255) exactly before the reference's blend.  Inference only (no autograd:
    uint8 tensors carry no gradient).  An extension of the drop-in API."""
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])
    if tgt_pose.is_cuda:
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    else:
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    B, H, W, P, _ = rgba_layers_u8.shape
    if B != batch_size or P != n_planes:
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {batch_size}/{n_planes}")
    homs = homs.reshape(B, P, 9)
    if B > 1 and rgba_layers_u8.stride(0) == 0:  # one MPI, many views: pack once
        return _lib.render_packed_u8(_lib.pack_planes_u8(rgba_layers_u8[0]), homs)
    out = torch.empty((B, H, W, 3), device=rgba_layers_u8.device, dtype=torch.float32)
    packed = None
    for b in range(B):
        packed = _lib.pack_planes_u8(rgba_layers_u8[b], out=packed)
        _lib.render_packed_u8(packed, homs[b:b + 1], out=out[b:b + 1])
    return out


def mpi_render_view_f16(rgba_layers_f16, tgt_pose, planes, intrinsics):
    """mpi_render_view_torch for a half-precision MPI [B, H, W, P, 4] float16 (a network's output
    under autocast, an RGBA16F / EXR asset): returns exactly
    mpi_render_view_torch(rgba_layers_f16.float(), tgt_pose, planes, intrinsics)
    in fp32 without the float copy: each view is packed at 8 B per texel and rendered by
    render_texel.hip, which converts every tap to float (exactly) before the reference's blend.
    The packed MPI is a temporary of this call, so a float copy would serve one launch only: a
    stride-0 batch takes the float-copy route of _lib.render_packed_f16 only from
    _lib.F16_FLOAT_ONCE_MIN_VIEWS views, where copy + float kernel beat the f16 kernel; below, and
    for a non-broadcast batch, the f16 kernel renders (a caller that renders one MPI many times
    packs it once and calls _lib.render_packed_f16, which routes a reused MPI from fewer views).
    Training: when rgba_layers_f16 requires grad (grad enabled) the frame is differentiable w.r.t. it --
    _lib.RenderF16Function: the half tensor is read in place at 8 B per texel by the training forward and
    the adjoint (render_chunk.hip InF16), and rgba_layers_f16.grad arrives in float16, bit for bit
    RN_half of the gradient mpi_render_view_torch(rgba_layers_f16.float(), ...) gives (which is what the
    reference's autograd leaves in a half leaf), with no fp32 gradient and no float copy (but of the one
    row or column of a degenerate frame, H or W < 2, for its forward frame).  A stride-0
    batch gets one half gradient per view and autograd's expand backward sums them in half.  When
    tgt_pose, planes or intrinsics requires grad the frame is differentiable w.r.t. them as in
    mpi_render_view_torch, with the same bits.  With nothing requiring grad, or under no_grad, the
    inference route above runs unchanged.  An extension of the drop-in API."""
    if not isinstance(rgba_layers_f16, torch.Tensor) or rgba_layers_f16.dtype != torch.float16:
        raise RuntimeError("mpi_render_view_f16 expects a float16 [B, H, W, P, 4] tensor")
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])
    if rgba_layers_f16.is_cuda and _camera_grad(tgt_pose, planes, intrinsics):
        if rgba_layers_f16.shape[0] != batch_size or rgba_layers_f16.shape[3] != n_planes:
            raise RuntimeError(f"shape mismatch: MPI batch/planes {rgba_layers_f16.shape[0]}/{rgba_layers_f16.shape[3]} "
                               f"vs poses/planes {batch_size}/{n_planes}")
        homs = _host.render_homographies_autograd(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
        return _lib.RenderF16Function.apply(rgba_layers_f16, homs.to(rgba_layers_f16.device))
    if tgt_pose.is_cuda:
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    else:
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    B, H, W, P, _ = rgba_layers_f16.shape
    if B != batch_size or P != n_planes:
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {batch_size}/{n_planes}")
    homs = homs.reshape(B, P, 9)
    if torch.is_grad_enabled() and rgba_layers_f16.requires_grad:
        return _lib.RenderF16Function.apply(rgba_layers_f16, homs)
    return _lib.render_f16_views(rgba_layers_f16, homs)  # (pack + packed render, view by view or once)


def _render_view2_chain(rgba_layers, tgt_pose, depths, src_intrinsics, tgt_intrinsics, tgt_height, tgt_width):
    """mpi_render_view_torch2's definition, helper by helper: the reference's mpi_render_view_torch
    (utils.py:267-294 -> 237-265) with k_t and the target grid opened up.  P warped [B,4,Ht,Wt] planes
    and P + 2 launches; differentiable w.r.t. rgba_layers (the sampler's and the compositor's HIP
    adjoints)."""
    n_planes, batch = depths.shape[0], tgt_pose.shape[0]
    d = depths.repeat(1, batch)
    imgs = rgba_layers.permute(3, 0, 1, 2, 4)
    rot, t = tgt_pose[:, :3, :3], tgt_pose[:, :3, 3:]
    n_hat = torch.tensor([0.0, 0.0, 1.0], device=tgt_pose.device).reshape(1, 1, 1, 3).repeat(n_planes, batch, 1, 1)
    a = -d.reshape(n_planes, batch, 1, 1)
    grid = meshgrid_abs_torch(batch, tgt_height, tgt_width).permute(0, 2, 3, 1).to(rgba_layers.device)
    warped = planar_transform_torch(imgs, grid, src_intrinsics, tgt_intrinsics, rot, t, n_hat, a)
    warped = warped.permute(0, 1, 3, 4, 2)
    return over_composite([warped[i] for i in range(n_planes)])


def mpi_render_view_torch2(rgba_layers, tgt_pose, planes, src_intrinsics, tgt_intrinsics, tgt_height, tgt_width):
    """Render an MPI [B, Hs, Ws, P, 4] into a target camera of its own size and intrinsics:
    [B, tgt_height, tgt_width, 3] fp32.  Bit for bit over_composite of the P planes of

        planar_transform_torch(rgba_layers.permute(3, 0, 1, 2, 4),
                               meshgrid_abs_torch(B, tgt_height, tgt_width).permute(0, 2, 3, 1),
                               src_intrinsics, tgt_intrinsics, rot, t, n_hat, -depths)

    -- what the reference computes inside mpi_render_view_torch (utils.py:267-294) with the two places
    where it reuses `intrinsics` and `height, width` opened up (planar_transform_torch already takes
    k_s, k_t and a target grid of any size, utils.py:198-233) -- as ONE fused HIP kernel: no warped
    plane and no sampling grid is written.  mpi_render_view_torch2(x, pose, planes, K, K, H, W) equals
    mpi_render_view_torch(x, pose, planes, K).

    The reference normalises the source pixel coordinate a target pixel lands on by the TARGET grid,
    swapped (x / (Ht - 1), y / (Wt - 1), utils.py:186-188), and grid_sample unnormalises over the
    source: a source pixel coordinate x_s is sampled at x_s * Ws / (Ht - 1) - 0.5 and y_s at
    y_s * Hs / (Wt - 1) - 0.5.  So the homography's source coordinates span 0 .. Ht - 1 and
    0 .. Wt - 1 whatever the MPI's size: express BOTH intrinsics at the target's resolution
    (supersampling an MPI 2x: scale its intrinsics by 2 for both arguments).  For a crop window
    [y0 : y0 + h, x0 : x0 + w] of a full frame, the target is h x w: src_intrinsics is the MPI's camera
    scaled to the WINDOW's size (h, w), and tgt_intrinsics is the full frame's camera with only its
    principal point shifted by the window's origin (cx - x0, cy - y0).

    rgba_layers: float32 as defined; uint8 as in mpi_render_view_u8 (exactly the float definition
    on x.float() / 255, from 4-B texels); float16 as in mpi_render_view_f16 (exactly the definition on
    x.float(), from 8-B texels); any other dtype raises.  `planes` must be a tensor (a list raises
    AttributeError as in the reference).  A stride-0 batch is packed once and rendered in one launch,
    any other batch view by view into one output.  Cameras on the host or the device (the autograd
    route too); under a HIP-graph capture host poses raise, and so do source intrinsics on the host
    (their upload cannot be part of the graph).

    The fused render follows the fused-multiply-add chain of the reference's batched matmul, which
    ATen uses from 45 target pixels (Ht * Wt >= 45); smaller targets, where ATen sums plain products
    (_lib.aten_plain), can differ from the helper chain in the last bit of a sample position.

    Autograd: with grad enabled and a float32 rgba_layers that requires grad, the helper chain itself
    runs (planar_transform_torch + over_composite, P warped planes) and d rgba_layers comes back from
    their HIP adjoints.  A float16 MPI requiring grad raises (pass .float()); a uint8 MPI has no
    gradient.  Camera gradients exist for the same-size render only: tgt_pose, planes or an
    intrinsics tensor requiring grad raises RuntimeError.  An extension of the drop-in API."""
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])  # AttributeError on a list, like the reference
    if not isinstance(rgba_layers, torch.Tensor) or rgba_layers.dtype not in (torch.float32, torch.uint8, torch.float16):
        raise RuntimeError("mpi_render_view_torch2 expects a float32, uint8 or float16 MPI, got "
                           f"{getattr(rgba_layers, 'dtype', type(rgba_layers).__name__)}")
    if rgba_layers.dim() != 5 or rgba_layers.shape[-1] != 4:
        raise RuntimeError(f"rgba_layers must be [B,H,W,P,4], got {tuple(rgba_layers.shape)}")
    B, _, _, P, _ = rgba_layers.shape
    if B != batch_size or P != n_planes:
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {batch_size}/{n_planes}")
    size = _lib._target_size((tgt_height, tgt_width))
    if rgba_layers.device.type != "cuda":
        raise RuntimeError("mpi_vision_amd kernels need ROCm device tensors "
                           f"(got a tensor on {rgba_layers.device}); there is no CPU path")
    if torch.is_grad_enabled():
        if any(isinstance(x, torch.Tensor) and x.requires_grad
               for x in (tgt_pose, planes, src_intrinsics, tgt_intrinsics)):
            raise RuntimeError("mpi_render_view_torch2: camera gradients (tgt_pose, planes, intrinsics) exist for the "
                               "same-size render only (mpi_render_view_torch); detach the camera arguments")
        if rgba_layers.requires_grad:
            if rgba_layers.dtype != torch.float32:
                raise RuntimeError("mpi_render_view_torch2: a float16 MPI is not differentiable here; pass "
                                   "rgba_layers.float()")
            return _render_view2_chain(rgba_layers, tgt_pose, depths, src_intrinsics, tgt_intrinsics, *size)
    if tgt_pose.is_cuda:  # poses in HBM: the chain runs there too
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), src_intrinsics, batch_size,
                                                tgt_intrinsics=tgt_intrinsics)
    else:
        _lib.host_under_capture("tgt_pose")  # host poses cannot be part of a captured HIP graph
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), src_intrinsics, batch_size, pin=True,
                                         tgt_intrinsics=tgt_intrinsics)
    homs = homs.reshape(B, P, 9)
    pack, render = {torch.float32: (_lib.pack_planes, _lib.render_packed),
                    torch.uint8: (_lib.pack_planes_u8, lambda *a, **k: _lib.render_packed_u8(*a, route_float=False, **k)),
                    torch.float16: (_lib.pack_planes_f16,
                                    lambda *a, **k: _lib.render_packed_f16(*a, route_float=False, **k))}[rgba_layers.dtype]
    mpi = rgba_layers.detach()
    if B > 1 and mpi.stride(0) == 0:  # one MPI, many views: pack once, one launch
        return render(pack(mpi[0]), homs, size=size)
    out = torch.empty((B,) + size + (3,), device=mpi.device, dtype=torch.float32)
    packed = None
    for b in range(B):
        packed = pack(mpi[b], out=packed)
        render(packed, homs[b:b + 1], out=out[b:b + 1], size=size)
    return out


def _plane_color_mpi(rgba_layers, plane_colors):
    """The float MPI the plane-colour render is defined on: RGB = plane_colors[p] all over plane p,
    alpha = rgba_layers' last channel (torch ops: differentiable w.r.t. both)."""
    B, H, W, P, _ = rgba_layers.shape
    rgb = plane_colors.to(rgba_layers.device)[None, None, None].expand(B, H, W, P, 3)
    return torch.cat([rgb, rgba_layers[..., -1:]], -1)


def mpi_render_plane_colors_torch(rgba_layers, plane_colors, tgt_pose, planes, intrinsics):
    """Composite one constant colour per plane, plane_colors [P, 3], through an MPI's alpha:
    returns exactly (bit for bit)

        mpi_render_view_torch(cat([plane_colors[None, None, None].expand(B, H, W, P, 3),
                                   rgba_layers[..., -1:]], -1), tgt_pose, planes, intrinsics)

    in [B, H, W, 3] fp32 without building that MPI.  rgba_layers is [B, H, W, P, 4] fp32 -- only
    channel 3 is read, in place through its strides -- or an alpha-only [B, H, W, P, 1].  Each view's
    alpha is packed at 4 B per texel and rendered by render_texel.hip's alpha format: a quarter of the
    float render's bytes.  As in the reference, a colour tap outside the plane contributes 0 (zero
    padding), so the result is not colour x coverage, and the back plane's alpha counts as 1.  Poses
    may live on the host or the device; a stride-0 batch is packed once and rendered in one launch.

    Autograd: when rgba_layers, plane_colors, tgt_pose, planes or intrinsics requires grad (and grad
    is enabled), the constant-colour MPI IS built with torch ops and rendered by the differentiable
    mpi_render_view_torch -- the reference's gradients, at the cost of the float MPI's memory
    (16 B per texel).  An extension of the drop-in API."""
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])  # AttributeError on a list, like the reference
    if not isinstance(rgba_layers, torch.Tensor) or rgba_layers.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float but found {getattr(rgba_layers, 'dtype', type(rgba_layers))}")
    if rgba_layers.dim() != 5 or rgba_layers.shape[-1] not in (1, 4):
        raise RuntimeError(f"expected a [B, H, W, P, 4] or [B, H, W, P, 1] MPI, got {tuple(rgba_layers.shape)}")
    _lib._dev(rgba_layers)  # no CPU path
    B, H, W, P, _ = rgba_layers.shape
    if B != batch_size or P != n_planes or tuple(plane_colors.shape) != (P, 3):
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {batch_size}/{n_planes}, "
                           f"plane_colors {tuple(plane_colors.shape)}")
    if torch.is_grad_enabled() and (rgba_layers.requires_grad or plane_colors.requires_grad
                                    or _camera_grad(tgt_pose, planes, intrinsics)):
        return mpi_render_view_torch(_plane_color_mpi(rgba_layers, plane_colors), tgt_pose, planes, intrinsics)
    if tgt_pose.is_cuda:
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    else:
        _lib.host_under_capture("tgt_pose")
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    homs = homs.reshape(B, P, 9)
    colors = _lib._up(plane_colors.detach(), rgba_layers.device, "plane_colors")
    if B > 1 and rgba_layers.stride(0) == 0:  # one MPI, many views: pack once
        return _lib.render_packed_alpha(_lib.pack_planes_alpha(rgba_layers[0]), colors, homs)
    out = torch.empty((B, H, W, 3), device=rgba_layers.device, dtype=torch.float32)
    packed = None
    for b in range(B):
        packed = _lib.pack_planes_alpha(rgba_layers[b], out=packed)
        _lib.render_packed_alpha(packed, colors, homs[b:b + 1], out=out[b:b + 1])
    return out


def mpi_render_depth_torch(rgba_layers, tgt_pose, planes, intrinsics):
    """Disparity, depth and coverage of a rendered view, [B, H, W, 3] fp32: channel 0 the expected
    inverse depth, channel 1 the expected depth, channel 2 the accumulated coverage -- exactly
    mpi_render_plane_colors_torch(rgba_layers, stack([1.0 / planes, planes, ones_like(planes)], -1),
    tgt_pose, planes, intrinsics).  As in the reference's over_composite the back plane's alpha counts
    as 1; coverage falls below 1 only where taps leave the planes.  Same inputs, routes and autograd
    rule as mpi_render_plane_colors_torch.  An extension of the drop-in API."""
    n_planes = len(planes)
    d = planes.reshape([n_planes])  # AttributeError on a list, like the reference
    colors = torch.stack([1.0 / d, d, torch.ones_like(d)], -1)
    return mpi_render_plane_colors_torch(rgba_layers, colors, tgt_pose, planes, intrinsics)


def mpi_from_net_output(mpi_pred, dep):
    """The notebook's MPI assembly (fast-torch-stereo-vision.ipynb cell 10 L79-111):
    the network output [B, 2P+3, H, W] (P blend weights, P alphas, background rgb) and
    dep['ref_img'] [B, H, W, 3] -> rgba_layers [B, H, W, P, 4], P = dep['mpi_planes'].shape[1].
    One HIP pass (assemble.hip) instead of the notebook's P-step torch.cat loop, bit-exact;
    differentiable w.r.t. mpi_pred (HIP backward) when it requires grad."""
    num_mpi_planes = dep['mpi_planes'].shape[1]
    fg_rgb = dep['ref_img'].to(mpi_pred.device)
    if torch.is_grad_enabled() and (mpi_pred.requires_grad or fg_rgb.requires_grad):
        return _lib.AssembleFunction.apply(mpi_pred, fg_rgb, num_mpi_planes)
    return _lib.assemble_mpi(mpi_pred, fg_rgb, num_mpi_planes)


def mpi_render_net_output_torch(mpi_pred, ref_img, tgt_pose, planes, intrinsics):
    """mpi_render_view_torch(mpi_from_net_output(mpi_pred, {'ref_img': ref_img, ...}), tgt_pose,
    planes, intrinsics) -- the two lines of both of the notebook's losses (ipynb cell 12 L7-11,
    L38-42) -- in ONE kernel: each plane's tile footprint is assembled from the network output
    straight into LDS and sampled there (assemble.hip render_netout_kernel); no [B, H, W, P, 4]
    tensor and no packed MPI is written.  Bit-identical to the two-step form.  Differentiable
    w.r.t. mpi_pred and ref_img when either requires grad (_lib.NetOutputRenderFunction: the
    training forward also writes the composite checkpoints; the backward re-assembles the MPI
    for the adjoint, so the MPI is never held between forward and backward), bit-exact to the
    reference's autograd of the two-step form.  Differentiable w.r.t. tgt_pose, planes and
    intrinsics too when any of them requires grad (see mpi_render_view_torch)."""
    batch_size = tgt_pose.shape[0]
    n_planes = len(planes)
    depths = planes.reshape([n_planes, 1])
    if mpi_pred.is_cuda and _camera_grad(tgt_pose, planes, intrinsics):
        homs = _host.render_homographies_autograd(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
        return _lib.NetOutputRenderFunction.apply(mpi_pred, ref_img.to(mpi_pred.device), homs.to(mpi_pred.device),
                                                  n_planes)
    if tgt_pose.is_cuda:
        homs = _host.render_homographies_device(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    else:
        homs = _host.render_homographies(tgt_pose, depths.reshape(-1), intrinsics, batch_size)
    fg = ref_img.to(mpi_pred.device)
    if torch.is_grad_enabled() and (mpi_pred.requires_grad or fg.requires_grad):
        return _lib.NetOutputRenderFunction.apply(mpi_pred, fg, homs, n_planes)
    return _lib.render_net_output(mpi_pred, fg, n_planes, homs)


def pixel2cam_torch(depth, pixel_coords, intrinsics, is_homogeneous=True):
    """Back-project pixels to camera space (utils.py:356-375)."""
    return _lib.pixel2cam(depth, pixel_coords, intrinsics, is_homogeneous)


def cam2pixel_torch(cam_coords, proj):
    """Project camera points to pixels [B, H, W, 2] (utils.py:377-393)."""
    return _lib.cam2pixel(cam_coords, proj)


def projective_inverse_warp_torch(img, depth, pose, intrinsics, ret_flows=False):
    """Inverse-warp a source image to the target plane at per-pixel depth
    (utils.py:409-450).  ret_flows=True is broken in the reference (shape mismatch,
    utils.py:447-448) and raises here too."""
    if ret_flows:
        raise RuntimeError("projective_inverse_warp_torch: ret_flows=True is not supported "
                           "(the reference raises a shape mismatch, utils.py:447-448)")
    batch, height, width, _ = img.shape
    if _warp_grad(img, depth, pose, intrinsics):
        return _warp_autograd(img, depth, pose, intrinsics, intrinsics, height, width)
    ki, proj = _warp_matrices(img, pose, intrinsics, intrinsics)
    return _lib.inverse_warp_depthmap(img, depth, ki, proj, height, width)


def plane_sweep_torch(img, depth_planes, pose, intrinsics):
    """Plane-sweep volume [B, H, W, D*C] (channel d*C+c) of img [B, H, W, C] at the
    listed depths (utils.py:452-471).  One HIP launch writes the whole volume.  When img, pose,
    intrinsics or a depth_planes tensor requires grad (grad enabled, img on the device) the volume is
    differentiable w.r.t. them, as in the reference: one HIP adjoint call (psv_bwd.hip), d img bit-exact
    to the reference's CPU autograd; the same holds for plane_sweep_torch_one / _one2."""
    batch, height, width, _ = img.shape
    return _plane_sweep(img, depth_planes, pose, intrinsics, intrinsics, height, width)


def _plane_sweep(img, depth_planes, pose, src_intrinsics, tgt_intrinsics, height, width, B=None):
    """B given (the unbatched _one calls): img [Hs,Ws,C] and pose [4,4] stand for a batch of 1."""
    if _warp_grad(img, depth_planes, pose, src_intrinsics, tgt_intrinsics):
        return _plane_sweep_autograd(img, depth_planes, pose, src_intrinsics, tgt_intrinsics, height, width, B)
    if img.is_cuda and pose.is_cuda:  # pose in HBM: proj is formed there, in the sweep's own call
        dev = pose.device
        if B is None:
            B = pose.shape[0]
        stream = torch.cuda.current_stream(dev)
        Ks, pose_d = _host.device_cameras(src_intrinsics, pose, B)
        ki = _host.psv_ki_device(tgt_intrinsics, B, dev, stream.cuda_stream)
        return _lib.plane_sweep_pose(img, depth_planes, ki, Ks, pose_d, height, width, stream)
    if B is not None:
        img, pose = img.unsqueeze(0), pose.unsqueeze(0)
    ki, proj = _host.psv_matrices(_batched(src_intrinsics), _batched(tgt_intrinsics), pose, pin=img.is_cuda)
    return _lib.plane_sweep(img, depth_planes, ki, proj, height, width)


def _plane_sweep_autograd(img, depth_planes, pose, src_intrinsics, tgt_intrinsics, height, width, B):
    """The sweep as a node of the autograd graph (_lib.PlaneSweepFunction): mpiv_plane_sweep's launch and bits,
    gradients for img, a depth_planes tensor, pose and the intrinsics.  The matrices come from the no-grad
    routes unless a camera input requires grad; then from _host.psv_matrices_autograd's chain on the host
    (not capturable)."""
    _lib._require_depths(depth_planes)
    if B is not None:
        img, pose = img.unsqueeze(0), pose.unsqueeze(0)
    if any(t.requires_grad for t in (pose, src_intrinsics, tgt_intrinsics)):
        ki, proj = _host.psv_matrices_autograd(_batched(src_intrinsics), _batched(tgt_intrinsics), pose)
        ki, proj = ki.to(img.device), proj.to(img.device)
    elif pose.is_cuda:
        ki, proj = _host.psv_matrices_device(src_intrinsics, tgt_intrinsics, pose, pose.shape[0])
    else:
        ki, proj = _host.psv_matrices(_batched(src_intrinsics), _batched(tgt_intrinsics), pose, pin=True)
    depths = depth_planes if isinstance(depth_planes, torch.Tensor) else _lib._depths_on(depth_planes, img.device)
    return _lib.PlaneSweepFunction.apply(img, depths, ki, proj, height, width)


def _batched(k):
    return k.unsqueeze(0) if k.dim() == 2 else k


def _warp_matrices(img, pose, src_intrinsics, tgt_intrinsics):
    if img.is_cuda and pose.is_cuda:
        return _host.psv_matrices_device(src_intrinsics, tgt_intrinsics, pose, pose.shape[0])
    return _host.psv_matrices(src_intrinsics, tgt_intrinsics, pose)


def _warp_grad(img, depth, *cameras):
    """The inverse warp's differentiable route: grad enabled, a device image, and any input requiring grad."""
    return (torch.is_grad_enabled() and img.is_cuda
            and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (img, depth, *cameras)))


def _warp_autograd(img, depth, pose, src_intrinsics, tgt_intrinsics, tgt_height, tgt_width):
    """projective_inverse_warp_torch[2] as a node of the autograd graph (_lib.InverseWarpFunction): the same
    forward launch and bits, gradients for img, depth, pose and the intrinsics, those of img and depth
    bit-exact to the reference's CPU autograd.  The matrices come from the no-grad routes unless a camera
    input requires grad; then from _host.psv_matrices_autograd's chain on the host (not capturable)."""
    if any(t.requires_grad for t in (pose, src_intrinsics, tgt_intrinsics)):
        ki, proj = _host.psv_matrices_autograd(src_intrinsics, tgt_intrinsics, pose)
        ki, proj = ki.to(img.device), proj.to(img.device)
    else:
        ki, proj = _warp_matrices(img, pose, src_intrinsics, tgt_intrinsics)
    return _lib.InverseWarpFunction.apply(img, depth, ki, proj, tgt_height, tgt_width)


def format_network_input_torch(self, ref_image, psv_src_images, ref_pose, psv_src_poses, planes, intrinsics):
    """Network input [B, H, W, 3 + S*D*3]: the reference image followed by one plane-sweep
    volume per extra source (utils.py:473-498; the unused leading `self` is kept).
    Each source's volume is swept straight into its channel slice of the output
    (no per-source tensors, no torch.cat).  When ref_image, psv_src_images, a pose, the intrinsics or a
    planes tensor requires grad (grad enabled, images on the device) the result is differentiable w.r.t.
    them (_lib.NetworkInputFunction): each source's slice gets the sweep's adjoint of its own channel slice
    of the gradient, read in place; the relative poses and the matrices then stay on the host graph."""
    S = psv_src_poses.shape[1]
    if S and _warp_grad(ref_image, planes, psv_src_images, ref_pose, psv_src_poses, intrinsics) and psv_src_images.is_cuda:
        return _network_input_autograd(ref_image, psv_src_images, ref_pose, psv_src_poses, planes, intrinsics)
    inv_ref = torch.inverse(_host._cpu32(ref_pose))
    rel = [torch.matmul(_host._cpu32(psv_src_poses[:, i]), inv_ref) for i in range(S)]  # utils.py:493
    return _lib.network_input(ref_image, psv_src_images, rel, planes, intrinsics)


def _network_input_autograd(ref_image, psv_src_images, ref_pose, psv_src_poses, planes, intrinsics):
    _lib._require_depths(planes)
    dev = ref_image.device
    S = psv_src_poses.shape[1]
    cams = any(t.requires_grad for t in (ref_pose, psv_src_poses, intrinsics))
    mats = []
    if cams:  # utils.py:493 and the matrices as nodes of the host graph
        host = lambda x: x.to(device="cpu", dtype=torch.float32)  # noqa: E731
        _lib.host_under_capture("the plane sweep's camera chain (poses, intrinsics)")
        poses = host(psv_src_poses)
        for i in range(S):
            rel = torch.matmul(poses[:, i], torch.inverse(host(ref_pose)))
            ki, proj = _host.psv_matrices_autograd(intrinsics, intrinsics, rel)
            mats += [ki.to(dev), proj.to(dev)]
    else:
        inv_ref = torch.inverse(_host._cpu32(ref_pose))
        for i in range(S):
            rel = torch.matmul(_host._cpu32(psv_src_poses[:, i]), inv_ref)
            mats += list(_host.psv_matrices(intrinsics, intrinsics, rel, pin=True))
    depths = planes if isinstance(planes, torch.Tensor) else _lib._depths_on(planes, dev)
    return _lib.NetworkInputFunction.apply(ref_image, psv_src_images, depths, *mats)


def plane_sweep_torch_one(img, depth_planes, pose, intrinsics):
    """Unbatched PSV of img [H, W, C]; returns [1, H, W, D*C] (utils.py:513-533).  The
    caller's own intrinsics tensor (not a per-call view of it) keys the memoised inverse."""
    return _plane_sweep(img, depth_planes, pose, intrinsics, intrinsics, img.shape[0], img.shape[1], B=1)


def projective_inverse_warp_torch2(img, depth, pose, src_intrinsics, tgt_intrinsics,
                                   tgt_height, tgt_width, ret_flows=False):
    """Inverse warp with separate source/target intrinsics and target size
    (utils.py:725-769)."""
    if ret_flows:
        raise RuntimeError("projective_inverse_warp_torch2: ret_flows=True is not supported "
                           "(the reference raises a shape mismatch, utils.py:766-767)")
    if _warp_grad(img, depth, pose, src_intrinsics, tgt_intrinsics):
        return _warp_autograd(img, depth, pose, src_intrinsics, tgt_intrinsics, tgt_height, tgt_width)
    ki, proj = _warp_matrices(img, pose, src_intrinsics, tgt_intrinsics)
    return _lib.inverse_warp_depthmap(img, depth, ki, proj, tgt_height, tgt_width)


def plane_sweep_torch_one2(img, depth_planes, pose, src_intrinsics, tgt_intrinsics,
                           tgt_height, tgt_width):
    """PSV of img [H_s, W_s, C] into a (tgt_height, tgt_width) target grid with separate
    intrinsics; returns [1, tgt_height, tgt_width, D*C] (utils.py:771-799)."""
    return _plane_sweep(img, depth_planes, pose, src_intrinsics, tgt_intrinsics, tgt_height, tgt_width, B=1)
