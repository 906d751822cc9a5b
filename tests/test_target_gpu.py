"""GPU: an MPI rendered into a target camera of its own size and intrinsics -- mpi_render_view_torch2 and
the packed entries behind it (mpiv_render_packed_tgt, _u8_tgt, _f16_tgt; render.hip RenderGeomT).

Two yardsticks, both bit for bit (assert_bits):
  * the kernels: the existing, unfused helper chain fed the same homographies -- _lib.warp_planes (the
    reference's transform_plane_imgs_torch: P warped planes) then _lib.over_composite;
  * the drop-in: the reference's own frames (tests/golden/target.npz, tools/gen_goldens_target.py).

The golden `td` has 45 target pixels: the smallest target at which the reference's batched matmul is the
fused-multiply-add chain the fused render follows; below, ATen sums plain products (_lib.aten_plain),
which the fused render has never followed -- no case here goes below.
"""
import functools

import numpy as np
import pytest
import torch

import lattice_cases
import target_cases as tc
from conftest import assert_bits, render_case_inputs
from test_render_colsep_gpu import _poses as colsep_poses

from mpi_vision_amd import _host, _lib, configs
from mpi_vision_amd import utils as mvu

pytestmark = pytest.mark.gpu

SENT = 1e30  # buffers start at this value: every element must be written


# ---------------------------------------------------------------------------
# the yardstick: warp_planes + over_composite
# ---------------------------------------------------------------------------

def chain(imgs, homs, size):
    """imgs [P, V, Hs, Ws, 4] (any strides), homs [V, P, 9] on the device -> [V, Ht, Wt, 3]: the P warped
    planes of transform_plane_imgs_torch (utils.py:160-195) composited back to front."""
    P, V = imgs.shape[:2]
    Ht, Wt = size
    grid = mvu.meshgrid_abs_torch(V, Ht, Wt).permute(0, 2, 3, 1).to(imgs.device)
    grid = grid[None].expand(P, V, Ht, Wt, 3)
    hom = homs.reshape(V, P, 3, 3).permute(1, 0, 2, 3).contiguous()
    warped = _lib.warp_planes(imgs, grid, hom).permute(0, 1, 3, 4, 2)  # [P, V, Ht, Wt, 4]
    return _lib.over_composite([warped[i] for i in range(P)])


def u8_float(q):
    """q.float() / 255 as the reference computes it: the IEEE division, on the CPU (a device division by a
    constant may multiply by its reciprocal), back on q's device."""
    return (q.cpu().float() / 255).to(q.device)


def chain_one_mpi(view, homs, size):
    """One MPI view [Hs, Ws, P, 4] under V homography sets."""
    V = homs.shape[0]
    Hs, Ws, P, _ = view.shape
    return chain(view.permute(2, 0, 1, 3)[:, None].expand(P, V, Hs, Ws, 4), homs, size)


# ---------------------------------------------------------------------------
# 1: the goldens through the drop-in
# ---------------------------------------------------------------------------

def _drop_in(name, dev, where, mpi=None):
    """mpi_render_view_torch2 on a golden case; where: cameras on the 'device' or the 'host'."""
    B, _, _, size = {**tc.CASES, **tc.DEGENERATE}[name]
    cam = tc.cameras(name)
    if where == "device":
        cam = tuple(c.to(dev) for c in cam)
    pose, depths, ks, kt = cam
    x = tc.mpi(name).to(dev) if mpi is None else mpi
    return mvu.mpi_render_view_torch2(x, pose, depths, ks, kt, *size)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", ["ta", "tb", "tc", "td", "te"])
def test_goldens(name, where, dev):
    """The reference's frames, with the cameras on the device and on the host."""
    assert_bits(_drop_in(name, dev, where), tc.golden()[f"{name}_out"], f"{name}, cameras on the {where}")


@pytest.mark.parametrize("name", ["ta", "tb", "te"])
def test_goldens_one_mpi_many_views(name, dev):
    """A stride-0 batch (packed once, one launch) and its materialised copy (packed view by view): view b of
    both is the frame of MPI 0 under camera b, which the chain gives; view 0 is the golden's."""
    B, (Hs, Ws), P, size = tc.CASES[name]
    one = tc.mpi(name)[:1].to(dev)
    want = chain_one_mpi(one[0], tc.golden_homs(name).to(dev), size)
    assert_bits(want[0], tc.golden()[f"{name}_out"][0], "chain vs the golden, view 0")
    assert_bits(_drop_in(name, dev, "device", one.expand(B, Hs, Ws, P, 4)), want.cpu().numpy(), "stride-0 batch")
    assert_bits(_drop_in(name, dev, "host", one.repeat(B, 1, 1, 1, 1)), want.cpu().numpy(), "materialised batch")


@pytest.mark.parametrize("name", ["ta", "tb"])
@pytest.mark.parametrize("fmt", ["u8", "f16"])
def test_narrow_twins(name, fmt, dev):
    """uint8: exactly the float function on x.float() / 255; float16: exactly the float function on
    x.float() -- batch by batch and as one MPI under both cameras."""
    B, (Hs, Ws), P, _ = tc.CASES[name]
    x = tc.mpi(name)
    q = (x.clamp(0, 1) * 255).round().to(torch.uint8) if fmt == "u8" else x.half()
    fl = u8_float(q) if fmt == "u8" else q.float()
    q, fl = q.to(dev), fl.to(dev)
    want = _drop_in(name, dev, "device", fl).cpu().numpy()
    assert np.isfinite(want).all() and (np.abs(want).sum(-1) > 0).mean() > 0.4
    assert_bits(_drop_in(name, dev, "device", q), want, f"{fmt} batch")
    want1 = _drop_in(name, dev, "device", fl[:1].expand(B, Hs, Ws, P, 4)).cpu().numpy()
    assert_bits(_drop_in(name, dev, "host", q[:1].expand(B, Hs, Ws, P, 4)), want1, f"{fmt} stride-0 batch")


@pytest.mark.parametrize("name", ["d1", "d2"])
def test_degenerate_sizes(name, dev):
    """A one-row target (the reference divides by Ht - 1 = 0) and a one-row source: the generic recipe,
    NaN for NaN and bit for bit elsewhere."""
    lattice_cases.match(_drop_in(name, dev, "device"), tc.golden()[f"{name}_out"], name)


def test_same_size_is_the_render(small, meta, dev):
    """mpi_render_view_torch2(x, pose, planes, K, K, H, W) is mpi_render_view_torch(x, pose, planes, K)."""
    name = "render_a"
    mpi = render_case_inputs(meta["small"], name).to(dev)
    pose, K, planes = (torch.tensor(small[f"{name}_{k}"]).to(dev) for k in ("pose", "K", "depths"))
    H, W = mpi.shape[1:3]
    got = mvu.mpi_render_view_torch2(mpi, pose, planes, K, K.clone(), H, W)
    assert_bits(got, small[f"{name}_out"], "vs the reference's mpi_render_view_torch golden")
    assert_bits(got, mvu.mpi_render_view_torch(mpi, pose, planes, K).cpu().numpy(), "vs mpi_render_view_torch")


# ---------------------------------------------------------------------------
# 2: source and target dimensions kept apart (shapes where swapping one H / W for another still gives a
#    plausible frame)
# ---------------------------------------------------------------------------

SPLIT = [((160, 150), 8, (150, 160)),  # both advances ~1: the tap-reuse rows kernel
         ((75, 80), 8, (150, 160)),    # advance ~0.5
         ((150, 160), 8, (75, 80)),    # minified
         ((37, 203), 7, (150, 70))]    # larger in one axis, smaller in the other; partial tiles in x and y
SPLIT_IDS = ["near1", "half", "minified", "mixed"]
VIEWS = 40
ROWS = "render_rows_tgt_kernel<false, %d, true, false, %d, false, false>"


@functools.lru_cache(maxsize=None)
def _split_homs(size, P):
    """VIEWS cameras built for the target size, _extreme_case style: a slow yaw path, then three poses with
    rotations to +-17 degrees and translations that put some planes partly behind the camera."""
    Ht, Wt = size
    g = torch.Generator().manual_seed(Ht * Wt + P)
    poses = [configs.pose_from(configs.rot_y(0.3 * k), (0.01 * k, -0.005 * k, 0.002 * k)) for k in range(VIEWS - 3)]
    extreme = []
    for k in range(3):
        t = ((torch.rand(3, generator=g) - 0.5) * (0.5 + k)).tolist()
        extreme.append(configs.pose_from(configs.rot_y((k - 1) * 17.0), t))
    poses = extreme + poses  # (the extreme ones come first: every V has them)
    K = configs.f32([configs.intrinsics_matrix(0.6 * Wt, 0.63 * Wt, Wt / 2.0, Ht / 2.0)] * VIEWS)
    return _host.render_homographies(configs.f32(poses), configs.f32(configs.inv_depths(0.3, 30, P)), K, VIEWS)


@functools.lru_cache(maxsize=None)
def _split_mpi(src, P):
    return configs.synthetic_mpi(1, src[0], src[1], P, 2000 + src[0])[0].to("cuda:0")


@functools.lru_cache(maxsize=None)
def _split_want(src, P, size, V):
    """The chain's frames for the first V views (computed once per shape and view count)."""
    want = chain_one_mpi(_split_mpi(src, P), _split_homs(size, P)[:V].to("cuda:0"), size).cpu().numpy()
    assert np.isfinite(want).all() and (np.abs(want).sum(-1) > 0).mean() > 0.15  # (a frame, not the border)
    return want


def _render_tgt(src, P, size, homs, out=None):
    return _lib.render_packed(_lib.pack_planes(_split_mpi(src, P)), homs, size=size, out=out)


@pytest.mark.parametrize("V", [1, 3, VIEWS])
@pytest.mark.parametrize("src,P,size", SPLIT, ids=SPLIT_IDS)
def test_split_shapes_automatic_route(src, P, size, V, dev):
    """The production dispatch at 1, 3 and 40 views: the (4, 4), (8, 4) and (6, 3) rows flavours where both
    advances are near 1, the one-row kernel on the small launches whose advance is far from 1."""
    name, _ = _lib.route("render_packed_tgt", src[0], src[1], P, V, size[0], size[1])
    if src == (160, 150):
        assert name == ROWS % {1: (4, 4), 3: (8, 4), VIEWS: (6, 3)}[V]
    else:
        assert name == "render_packed_tgt_kernel<false, true>"
    out = torch.full((V,) + size + (3,), SENT, device=dev)
    _render_tgt(src, P, size, _split_homs(size, P)[:V], out=out)
    assert_bits(out, _split_want(src, P, size, V), name)


@pytest.mark.parametrize("opts", [dict(render_vshare=11), dict(render_vshare=3), dict(render_vshare=4),
                                  dict(render_vshare=5), dict(render_vshare=4, render_same=1),
                                  dict(render_vshare=4, render_same=2), dict(render_vshare=3, render_same=1),
                                  dict(render_vshare=5, render_same=1), dict(render_vshare=11, render_same=1),
                                  dict(render_tile=-1)],
                         ids=["44", "84", "63", "93", "63same", "63oob", "84same", "93same", "44same", "onerow"])
@pytest.mark.parametrize("src,P,size", SPLIT, ids=SPLIT_IDS)
def test_split_shapes_every_flavour(src, P, size, opts, dev, kopts):
    """Every rows flavour the dispatcher can launch for a target (and the one-row kernel), forced on every
    shape: the flavour affects speed only, the frames are the chain's."""
    V = 3
    kopts(**opts)
    out = torch.full((V,) + size + (3,), SENT, device=dev)
    _render_tgt(src, P, size, _split_homs(size, P)[:V], out=out)
    assert_bits(out, _split_want(src, P, size, V), str(opts))


@pytest.mark.parametrize("fmt", ["u8", "f16"])
@pytest.mark.parametrize("src,P,size", SPLIT, ids=SPLIT_IDS)
def test_split_shapes_narrow(src, P, size, fmt, dev):
    """The u8 and f16 entries at 3 views: the chain on the float MPI the format stands for."""
    V = 3
    x = _split_mpi(src, P)
    if fmt == "u8":
        q = (x.clamp(0, 1) * 255).round().to(torch.uint8)
        fl, packed, render = u8_float(q), _lib.pack_planes_u8(q), _lib.render_packed_u8
    else:
        q = x.half()
        fl, packed, render = q.float(), _lib.pack_planes_f16(q), _lib.render_packed_f16
    homs = _split_homs(size, P)[:V]
    name, _ = _lib.route(f"render_packed_{fmt}_tgt", src[0], src[1], P, V, size[0], size[1])
    assert name == f"render_{fmt}_tgt_kernel<" + ("4, true, 4>" if src == (160, 150) else "2, false, 2>")
    want = chain_one_mpi(fl, homs.to(dev), size).cpu().numpy()
    out = torch.full((V,) + size + (3,), SENT, device=dev)
    render(packed, homs, out=out, size=size, route_float=False)
    assert_bits(out, want, name)
    assert_bits(render(packed, homs, size=size, route_float=True), want, "through the float copy")


def test_narrow_large_launch_flavours(dev, kopts):
    """(4 rows, reuse, 2 in flight) -- what a launch of 2048 blocks and more takes -- for f16 at 72 views, and
    the u8 kernel with 8 and 2 rows in flight."""
    src, P, size = SPLIT[0]
    V = 72
    homs = _split_homs(size, P)[torch.arange(V) % VIEWS]
    assert _lib.route("render_packed_f16_tgt", src[0], src[1], P, V, size[0], size[1])[0] == \
        "render_f16_tgt_kernel<4, true, 2>"
    q = _split_mpi(src, P).half()
    got = _lib.render_packed_f16(_lib.pack_planes_f16(q), homs, size=size, route_float=False)
    want = chain_one_mpi(q.float(), homs[:VIEWS].to(dev), size).cpu().numpy()
    assert_bits(got[:VIEWS], want, "f16, views 0..39")
    assert_bits(got[VIEWS:], want[:V - VIEWS], "f16, views 40..71 (the first 32 again)")
    for (s, p, sz), opts in ((SPLIT[0], dict(u8_flight=8)), (SPLIT[0], dict(u8_flight=2))):
        kopts(**opts)
        q8 = (_split_mpi(s, p).clamp(0, 1) * 255).round().to(torch.uint8)
        h3 = _split_homs(sz, p)[:3]
        got = _lib.render_packed_u8(_lib.pack_planes_u8(q8), h3, size=sz, route_float=False)
        _lib.reset_debug()
        assert_bits(got, chain_one_mpi(u8_float(q8), h3.to(dev), sz).cpu().numpy(), f"u8 {opts}")


# ---------------------------------------------------------------------------
# 3: the column-separable path and the tile order
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _path_homs(kind, size, P):
    """test_render_colsep_gpu's sway (separable) and pitch views, built for the target size."""
    Ht, Wt = size
    f = configs.focal_from_fov(Wt)
    n = len(colsep_poses(kind))
    K = configs.f32([configs.intrinsics_matrix(f, f, Wt / 2.0, Ht / 2.0)] * n)
    return _host.render_homographies(configs.f32(colsep_poses(kind)), configs.f32(configs.inv_depths(1, 100, P)), K, n)


@pytest.mark.parametrize("V", [2, 5, 12])
@pytest.mark.parametrize("kind", ["sway", "pitch"])
def test_column_separable_views(kind, V, dev, kopts):
    """160x150 -> 150x160 on the sway path (h1 == h7 == 0 on every plane: the column set is computed once per
    lane and plane, from the TARGET's normaliser and the SOURCE's clamp) and with 1 degree of pitch (the row
    recipe): render_colsep 0 and -1 give the same frames, the chain's."""
    src, P, size = SPLIT[0]
    homs = _path_homs(kind, size, P)[:V]
    sep = bool((homs[..., 1] == 0).all() and (homs[..., 7] == 0).all())
    assert sep == (kind == "sway")
    assert _lib.route("render_packed_tgt", src[0], src[1], P, V, size[0], size[1])[0].startswith("render_rows_tgt_kernel")
    want = chain_one_mpi(_split_mpi(src, P), homs.to(dev), size).cpu().numpy()
    assert np.isfinite(want).all() and (np.abs(want).sum(-1) > 0).mean() > 0.5
    for cs in (0, -1):
        kopts(render_colsep=cs)
        assert_bits(_render_tgt(src, P, size, homs), want, f"render_colsep={cs}")
    for fmt in ("u8", "f16"):  # the narrow formats' column set
        x = _split_mpi(src, P)
        q = (x.clamp(0, 1) * 255).round().to(torch.uint8) if fmt == "u8" else x.half()
        fl = u8_float(q) if fmt == "u8" else q.float()
        pack, render = (_lib.pack_planes_u8, _lib.render_packed_u8) if fmt == "u8" else \
            (_lib.pack_planes_f16, _lib.render_packed_f16)
        wantq = chain_one_mpi(fl, homs.to(dev), size).cpu().numpy()
        for cs in (0, -1):
            kopts(render_colsep=cs)
            assert_bits(render(pack(q), homs, size=size, route_float=False), wantq, f"{fmt}, render_colsep={cs}")


@pytest.mark.parametrize("order", [-1, 1])
def test_tile_order(order, dev, kopts):
    """37x203 -> 150x70 (2 x 7 tiles of 64 x 24, partial in x and y) at 40 views in the band and the
    interleaved tile order: the tile grid is the target's."""
    src, P, size = SPLIT[3]
    kopts(render_order=order, render_vshare=4)
    out = torch.full((VIEWS,) + size + (3,), SENT, device=dev)
    _render_tgt(src, P, size, _split_homs(size, P), out=out)
    assert_bits(out, _split_want(src, P, size, VIEWS), f"render_order={order}")


# ---------------------------------------------------------------------------
# 4: dead tiles
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [{}, dict(render_vshare=11), dict(render_tile=-1)], ids=["auto", "rows", "onerow"])
def test_dead_tiles(opts, dev, kopts):
    """A 64 x 256 target from a 96 x 96 source under near-identity cameras: source x is normalised by
    Ht - 1 = 63 and unnormalised over Ws = 96, so target columns from ~66 on sample past the source's right
    border -- tile_dead must hold the source's W + 1 against positions from the target's normaliser.  The
    right half (tile columns 2 and 3) is dead on every plane: composite_zero's value, +0; the frame is the
    chain's."""
    src, P, size = (96, 96), 5, (64, 256)
    Ht, Wt = size
    poses = [configs.pose_from(configs.rot_y(0.2 * k), (0.004 * k, -0.002 * k, 0.001 * k)) for k in range(3)]
    K = configs.f32([configs.intrinsics_matrix(1.0 * Wt, 1.0 * Wt, Wt / 2.0, Ht / 2.0)] * 3)
    homs = _host.render_homographies(configs.f32(poses), configs.f32(configs.inv_depths(1, 100, P)), K, 3)
    # the premise, from the homographies: every plane maps target column 128 and beyond to a source x whose
    # sample position x_s * Ws / (Ht - 1) - 0.5 is at least Ws + 1
    h = homs.double().reshape(3, P, 3, 3)
    for x in (128.0, 255.0):
        for y in (0.0, Ht - 1.0):
            p = h @ torch.tensor([x, y, 1.0], dtype=torch.float64)
            assert bool((p[..., 0] / p[..., 2] * src[1] / (Ht - 1) - 0.5 >= src[1] + 2).all())
    kopts(**opts)
    got = _render_tgt(src, P, size, homs).cpu().numpy()
    _lib.reset_debug()
    want = chain_one_mpi(_split_mpi(src, P), homs.to(dev), size).cpu().numpy()
    assert_bits(got, want, f"dead tiles, {opts}")
    assert not got[:, :, 128:].view(np.uint32).any(), "the dead half is composite_zero's +0"
    assert (np.abs(got[:, :, :64]).sum(-1) > 0).mean() > 0.9, "the live tile column is a frame"


# ---------------------------------------------------------------------------
# 5: the autograd rule
# ---------------------------------------------------------------------------

def test_autograd_rule(dev, monkeypatch):
    """tg.  Grad required: the helper chain itself runs (no target launch) and d rgba_layers is the explicit
    chain's, bit for bit, within the README's 1e-5 of the reference's CPU autograd.  No grad: the pack and
    exactly one target launch."""
    g = tc.golden()
    B, (Hs, Ws), P, size = tc.CASES["tg"]
    pose, depths, ks, kt = (c.to(dev) for c in tc.cameras("tg"))
    dout = torch.tensor(g["tg_dout"]).to(dev)
    names = []
    call = _lib._call
    monkeypatch.setattr(_lib, "_call", lambda name, *a: (names.append(name), call(name, *a))[1])

    leaf = tc.mpi("tg").to(dev).requires_grad_(True)
    out = mvu.mpi_render_view_torch2(leaf, pose, depths, ks, kt, *size)
    out.backward(dout)
    assert not [n for n in names if n.endswith("_tgt")], names
    assert_bits(out, g["tg_out"], "frame under autograd")

    ref = tc.mpi("tg").to(dev).requires_grad_(True)
    d = depths.reshape(P, 1).repeat(1, B)
    n_hat = torch.tensor([0.0, 0.0, 1.0], device=dev).reshape(1, 1, 1, 3).repeat(P, B, 1, 1)
    grid = mvu.meshgrid_abs_torch(B, *size).permute(0, 2, 3, 1).to(dev)
    w = mvu.planar_transform_torch(ref.permute(3, 0, 1, 2, 4), grid, ks, kt, pose[:, :3, :3], pose[:, :3, 3:], n_hat,
                                   -d.reshape(P, B, 1, 1)).permute(0, 1, 3, 4, 2)
    mvu.over_composite([w[i] for i in range(P)]).backward(dout)
    assert_bits(leaf.grad, ref.grad.cpu().numpy(), "d rgba_layers vs the explicit helper chain")
    got = leaf.grad.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - g["tg_grad"]).max())
    print(f"d rgba_layers vs the reference's CPU autograd: max |diff| {err:.3g}, "
          f"bit-equal {np.array_equal(got.view(np.uint32), g['tg_grad'].view(np.uint32))}")
    assert err <= 1e-5

    # the same with every camera argument on the host: the same frame and the same gradient
    hleaf = tc.mpi("tg").to(dev).requires_grad_(True)
    hout = mvu.mpi_render_view_torch2(hleaf, *tc.cameras("tg"), *size)
    hout.backward(dout)
    assert not [n for n in names if n.endswith("_tgt")], names
    assert_bits(hout, g["tg_out"], "frame under autograd, host cameras")
    assert_bits(hleaf.grad, got, "d rgba_layers, host cameras")

    for enabled, inp in ((True, leaf.detach()), (False, leaf)):  # nothing requires grad / grad disabled
        names.clear()
        with torch.set_grad_enabled(enabled):
            plain = mvu.mpi_render_view_torch2(inp, pose, depths, ks, kt, *size)
        assert not plain.requires_grad
        assert [n for n in names if "render_packed" in n] == ["mpiv_render_packed_tgt"], names
        assert [n for n in names if "pack_planes" in n] == ["mpiv_pack_planes"], names
        assert not [n for n in names if "grid_sample" in n or "over_composite" in n or "plane_coords" in n], names
        assert_bits(plain, g["tg_out"], "the fused frame")


def test_autograd_refusals(dev):
    """Camera gradients exist for the same-size render only; a half MPI requiring grad points to .float()."""
    B, (Hs, Ws), P, size = tc.CASES["tg"]
    x = tc.mpi("tg").to(dev)
    for k in range(4):
        cam = [c.to(dev) for c in tc.cameras("tg")]
        cam[k] = cam[k].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="same-size render only"):
            mvu.mpi_render_view_torch2(x, *cam, *size)
        with torch.no_grad():  # (grad disabled: nothing is asked for)
            assert_bits(mvu.mpi_render_view_torch2(x, *cam, *size), tc.golden()["tg_out"], "under no_grad")
    cam = [c.to(dev) for c in tc.cameras("tg")]
    half = x.half().requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"\.float\(\)"):
        mvu.mpi_render_view_torch2(half, *cam, *size)
    with torch.no_grad():
        assert mvu.mpi_render_view_torch2(half, *cam, *size).shape == (B,) + size + (3,)


# ---------------------------------------------------------------------------
# 6: memory
# ---------------------------------------------------------------------------

def test_no_warped_planes_are_made(dev):
    """128 x 160 x 16 into 256 x 320: peak growth below the packed MPI (5.5 MB) plus the frame (1 MB) plus one
    warped plane (Ht * Wt * 16 B = 1.3 MB) -- the chain's 16 warped planes alone are 21 MB."""
    Hs, Ws, P, (Ht, Wt) = 128, 160, 16, (256, 320)
    x = configs.synthetic_mpi(1, Hs, Ws, P, 77).to(dev)
    pose = configs.f32([configs.pose_from(configs.rot_y(2.0), (0.05, -0.02, 0.03))]).to(dev)
    K = configs.f32([configs.intrinsics_matrix(0.6 * Wt, 0.6 * Wt, Wt / 2.0, Ht / 2.0)]).to(dev)
    planes = torch.linspace(30.0, 0.3, P, device=dev)
    args = (x, pose, planes, K, K.clone(), Ht, Wt)
    want = mvu.mpi_render_view_torch2(*args).cpu()  # warm-up (memoises inverse(K))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = mvu.mpi_render_view_torch2(*args)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(dev) - base
    packed, frame, plane = P * (Hs + 4) * (Ws + 4) * 16, Ht * Wt * 12, Ht * Wt * 16
    print(f"peak growth {growth} bytes (bound {packed + frame + plane})")
    assert packed <= growth < packed + frame + plane, growth
    assert torch.equal(out.cpu(), want) and bool(torch.isfinite(want).all()) and float(want.abs().sum()) > 0


# ---------------------------------------------------------------------------
# 7: side stream, captured graph
# ---------------------------------------------------------------------------

def _stream_sets(fmt, dev):
    src, P, size = SPLIT[1]
    V = 3
    sets = []
    for k in range(2):
        x = configs.synthetic_mpi(1, src[0], src[1], P, 3000 + k)[0]
        if fmt == "u8":
            x = (x.clamp(0, 1) * 255).round().to(torch.uint8)
        elif fmt == "f16":
            x = x.half()
        sets.append((x.to(dev), _split_homs(size, P)[k * 3:k * 3 + V].contiguous().to(dev)))
    fl = {"f32": lambda t: t, "u8": u8_float, "f16": lambda t: t.float()}[fmt]
    want = [chain_one_mpi(fl(m), h, size).cpu().numpy() for m, h in sets]
    assert not np.array_equal(want[0], want[1])
    return (src, P, size, V), sets, want


def _entries(fmt):
    """(pack, render, packed buffer factory) of a format."""
    if fmt == "u8":
        return _lib.pack_planes_u8, functools.partial(_lib.render_packed_u8, route_float=False), \
            lambda P, H, W, dev: torch.zeros((P, H + 4, W + 4), dtype=torch.int32, device=dev)
    if fmt == "f16":
        return _lib.pack_planes_f16, functools.partial(_lib.render_packed_f16, route_float=False), \
            lambda P, H, W, dev: torch.zeros((P, H + 4, W + 4, 4), dtype=torch.float16, device=dev)
    return _lib.pack_planes, _lib.render_packed, lambda P, H, W, dev: torch.full((P, H + 4, W + 4, 4), SENT, device=dev)


@pytest.mark.parametrize("fmt", ["f32", "u8", "f16"])
def test_side_stream(fmt, dev):
    """The pack and the target render on a side stream: the chain's frames."""
    (src, P, size, V), sets, want = _stream_sets(fmt, dev)
    pack, render, _ = _entries(fmt)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = [render(pack(m), h, out=torch.full((V,) + size + (3,), SENT, device=dev), size=size) for m, h in sets]
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2):
        assert_bits(got[k], want[k], f"side stream, data set {k}")


@pytest.mark.parametrize("fmt", ["f32", "u8", "f16"])
def test_captured_graph_replays_with_new_data(fmt, dev, monkeypatch):
    """The pack + the target render captured on one stream (a single chain of two launches, no parallel
    branches) and replayed with another MPI and other homographies in the static inputs: the chain's frames
    on every replay."""
    (src, P, size, V), sets, want = _stream_sets(fmt, dev)
    pack, render, buf = _entries(fmt)
    sfx = "" if fmt == "f32" else "_" + fmt
    m, h = (t.clone() for t in sets[1])
    pk = buf(P, src[0], src[1], dev)
    out = torch.full((V,) + size + (3,), SENT, device=dev)
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):  # warm-up on the capture stream
        render(pack(m, out=pk), h, out=out, size=size)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    launches = []
    call = _lib._call
    monkeypatch.setattr(_lib, "_call", lambda name, *a: (launches.append((name, a[-1].value)), call(name, *a))[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        render(pack(m, out=pk), h, out=out, size=size)
    monkeypatch.undo()
    # one chain: the pack, then the render, both enqueued on the capture stream and on no other
    assert [n for n, _ in launches] == [f"mpiv_pack_planes{sfx}", f"mpiv_render_packed{sfx}_tgt"], launches
    assert {q for _, q in launches} == {S.cuda_stream}, launches
    for k in (0, 1, 0):
        for dst, srct in zip((m, h), sets[k]):
            dst.copy_(srct)
        pk.zero_()
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(out, want[k], f"replay with data set {k}")


def test_drop_in_under_capture(dev):
    """mpi_render_view_torch2 with device cameras captures (inverse(k_t) memoised by the warm-up, written into
    the graph as a constant); with host poses, or host source intrinsics (read live: their upload would be
    captured), it raises before anything is launched."""
    B, (Hs, Ws), P, size = tc.CASES["tb"]
    x = tc.mpi("tb")[:1].to(dev).expand(B, Hs, Ws, P, 4)
    pose, depths, ks, kt = (c.to(dev) for c in tc.cameras("tb"))
    want = chain_one_mpi(x[0], tc.golden_homs("tb").to(dev), size).cpu().numpy()
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):
        mvu.mpi_render_view_torch2(x, pose, depths, ks, kt, *size)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    host_pose, host_ks = pose.cpu(), ks.cpu()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        out = mvu.mpi_render_view_torch2(x, pose, depths, ks, kt, *size)
        with pytest.raises(RuntimeError, match="host"):
            mvu.mpi_render_view_torch2(x, host_pose, depths, ks, kt, *size)
        with pytest.raises(RuntimeError, match="src_intrinsics is a host"):
            mvu.mpi_render_view_torch2(x, pose, depths, host_ks, kt, *size)
    graph.replay()
    torch.cuda.synchronize()
    assert_bits(out, want, "replay")
