#!/usr/bin/env python3
"""Golden fixtures for the per-point geometry helpers and the frame codecs at the shapes where a kernel
can go wrong: both sides of ATen's small-matmul threshold, both sides of a 256-thread block, k = 1..3,
zero denominators and non-finite values.  Runs the REFERENCE utils.py on the CPU (the import recipe of
tools/gen_goldens.py) with 8 torch threads; writes tests/golden/geometry.npz.  Test tooling only.

Inputs are seeded draws (the `*_inputs` functions below, which the tests import); the file stores their
sha256 (one JSON table, `shas`, keyed by case) and the reference's outputs:

    tp_<M>_<n>        transform_points_torch, points [M,1,n,3] and homographies [M,3,3] (M = 0: a [3,3]
                      homography and [1,n,3] points), randn operands: every product inexact; n = 1000 is
                      recorded as the output's digest (shas: tp_2_1000_out), which the tests hold the
                      restatement to before they compare with it
    p2c_<B>_<n>       pixel2cam_torch (homogeneous), K with skew, general pixel_coords; the non-homogeneous
                      call is asserted to equal its first three rows and recorded as a digest (shas: _h0)
    c2p_<B>_<n>       cam2pixel_torch, full 4x4 proj, general fourth row; from n = 24 up the last point of
                      the last batch element has z + 1e-10 == 0 (asserted: an infinity there, z < 0 elsewhere)
                      _ki is the reference's torch.inverse(K) (LAPACK's bits differ between hosts)
    pc_<Ht>x<Wt>_*    transform_plane_imgs_torch on [L,B] = [2,2] planes: _hom (the reference's
                      inv_homography_torch, from which the w == 0 points are built), _coords (utils.py:178-188
                      restated with the reference's own functions) and _out (the sampled planes)
    nh_<k>_<n>_*      normalize_homogeneous_torch: _out, _w (the w column after the call) and shas: _after (the
                      input after the call; asserted: only w == 0 rows are rewritten)
    pre_<n>, dep_<n>  preprocess_image_torch / deprocess_image_torch (n = 65537 is a ramp of period 251, so
                      the outputs compress); special values in the first and the last 16 elements
    bd_render, bd_warp, bd_sweep   the smallest frames inside the fused kernels' contract (5x9 = 45 pixels):
                      mpi_render_view_torch at 5x9xP5 with a 6 degree rotation about a general axis (a rotation
                      about y leaves one inexact product per row, and the two chains coincide),
                      projective_inverse_warp_torch
                      at B = 2 and plane_sweep_torch with D = 3, rotated poses; bd_homs and bd_ki are the
                      reference's homographies and K^-1 (host-dependent through torch.inverse)

For every matmul shape the recorder asserts that the reference equals, bit for bit, the chain that
tests/geometry_cases.py's rule selects (plain products below 400 multiply-adds per batch element, the FMA
chain from there on; a homography without batch dimensions always FMA), and that every other stored
output equals that module's restatement.  A shape where MKL is irregular fails here.  One did and was
moved: the homography without batch dimensions at n = 1 is recorded at n = 11 instead.  That call is `mm`,
and MKL's sgemm of 10 or fewer points by a 3x3 matrix matches neither chain on this CPU (20 seeds each, n =
1..10); from n = 11 up it is the FMA chain.  The recorder also prints how often the always-FMA
arithmetic of the fused kernels differs from the reference below 45 pixels (quoted in DESIGN.md).

Usage:  python tools/gen_goldens_geometry.py
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from mpi_vision_amd import configs  # noqa: E402  (pure-python workload definitions)

TP_BATCHED = [(M, n) for M in (1, 2, 6) for n in (1, 4, 44, 45, 64)] + [(2, n) for n in (255, 256, 257, 1000)]
TP_UNBATCHED = [(0, n) for n in (11, 20, 45)]
TP = TP_BATCHED + TP_UNBATCHED
HW = {1: (1, 1), 24: (4, 6), 25: (5, 5), 44: (4, 11), 45: (5, 9), 257: (1, 257)}
P2C = [(B, n) for B in (1, 2) for n in (1, 44, 45, 257)]
C2P = [(B, n) for B in (1, 2) for n in (1, 24, 25, 257)]
PC = [(4, 11), (5, 9), (1, 9), (45, 1)]
NH = [(k, n) for k in (1, 2, 3) for n in (1, 255, 256, 257)]
CODEC_N = (1, 255, 256, 257, 65537)
NH_W = (0.0, -0.0, 1e-40, float("inf"), float("-inf"), float("nan"))
SWEEP_DEPTHS = [1.0, 2.5, 7.0]
TP_DIGEST_ONLY = (1000,)


def sha(*ts) -> str:
    h = hashlib.sha256()
    for t in ts:
        a = t.detach().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
        h.update(a.tobytes())
    return h.hexdigest()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _skew_K(g, B):
    """[B,3,3] intrinsics with a non-zero skew."""
    r = torch.rand((B, 5), generator=g)
    K = torch.zeros((B, 3, 3))
    K[:, 0, 0], K[:, 0, 1], K[:, 0, 2] = 35 + 10 * r[:, 0], 0.7 + r[:, 1], 20 + 3 * r[:, 2]
    K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = 33 + 10 * r[:, 3], 14 + 3 * r[:, 4], 1.0
    return K


def rot_axis(deg, axis):
    """Rotation by `deg` degrees about the unit vector `axis` (Rodrigues, float64 lists): no coordinate axis
    is kept, so every row of a homography built from it has three inexact products."""
    import math
    (x, y, z), c, s = axis, math.cos(math.radians(deg)), math.sin(math.radians(deg))
    C = 1 - c
    return [[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
            [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
            [z * x * C - y * s, z * y * C + x * s, c + z * z * C]]


def tp_inputs(M, n):
    """(points, homography): [M,1,n,3] and [M,3,3], or [1,n,3] and [3,3] for M = 0."""
    g = _gen(100000 + 10000 * M + n)
    if M == 0:
        return torch.randn((1, n, 3), generator=g) * 10, torch.randn((3, 3), generator=g)
    return torch.randn((M, 1, n, 3), generator=g) * 10, torch.randn((M, 3, 3), generator=g)


def p2c_inputs(B, n):
    """(depth [B,H,W], pixel_coords [B,3,H,W], K [B,3,3] with skew)."""
    g = _gen(200000 + 10000 * B + n)
    H, W = HW[n]
    return (torch.rand((B, H, W), generator=g) * 10 + 0.5, torch.randn((B, 3, H, W), generator=g) * 20,
            _skew_K(g, B))


def c2p_inputs(B, n):
    """(cam [B,4,H,W], proj [B,4,4]); from n = 24 up the last point of the last batch element projects to
    z == -1e-10 exactly."""
    g = _gen(300000 + 10000 * B + n)
    H, W = HW[n]
    cam, proj = torch.randn((B, 4, H, W), generator=g) * 5, torch.randn((B, 4, 4), generator=g)
    if n >= 24:
        proj[B - 1, 2, 3] = 1.0
        cam[B - 1, :, H - 1, W - 1] = torch.tensor([0.0, 0.0, 0.0, -1e-10])
    return cam, proj


def pc_cameras(Ht, Wt):
    """(k_s, k_t, rot, t, n_hat, a) in transform_plane_imgs_torch's [L,B,...] shapes, L = B = 2: batch
    element 0 a general rotation, element 1 a rotation about z with t_z = 0 (an affine homography: w = z)."""
    g = _gen(400000 + 100 * Ht + Wt)
    L = B = 2
    k_s, k_t = _skew_K(g, B), _skew_K(g, B)
    rot = configs.f32([rot_axis(9.0, (0.6, 0.64, 0.48)), rot_axis(17.0, (0.0, 0.0, 1.0))])
    t = configs.f32([[[0.05], [-0.02], [0.03]], [[0.04], [0.01], [0.0]]])
    rep = lambda x: x.unsqueeze(0).repeat((L,) + (1,) * x.dim())  # noqa: E731
    n_hat = torch.tensor([0.0, 0.0, 1.0]).reshape(1, 1, 1, 3).repeat(L, B, 1, 1)
    a = -configs.f32([4.0, 1.5]).reshape(L, 1, 1, 1).repeat(1, B, 1, 1)
    return rep(k_s), rep(k_t), rep(rot), rep(t), n_hat, a


def pc_inputs(Ht, Wt, hom):
    """(imgs [2,2,6,7,3], pixel_coords_trg [2,2,Ht,Wt,3]) for the homographies `hom` [2,2,3,3] of
    pc_cameras (the golden's _hom).  Point 0 of every plane is (h7, -h6, 0): w == 0 under the plain chain
    (the two products cancel), a rounding error under the FMA chain.  Point 1 and the last point have
    z == 0: w == +0 exactly where the homography is affine."""
    g = _gen(410000 + 100 * Ht + Wt)
    imgs = torch.rand((2, 2, 6, 7, 3), generator=g)
    pts = torch.rand((2, 2, Ht, Wt, 3), generator=g) * torch.tensor([6.0, 5.0, 0.2]) + torch.tensor([0.0, 0.0, 0.9])
    flat = pts.reshape(2, 2, Ht * Wt, 3)
    hom = torch.as_tensor(hom)
    flat[:, :, 0, 0], flat[:, :, 0, 1], flat[:, :, 0, 2] = hom[:, :, 2, 1], -hom[:, :, 2, 0], 0.0
    flat[:, :, 1, 2] = 0.0
    flat[:, :, -1, 2] = 0.0
    return imgs, flat.reshape(2, 2, Ht, Wt, 3).clone()


def nh_inputs(k, n):
    """points [n, k+1]: w in {+0, -0, a subnormal, +Inf, -Inf, NaN} in the first and the last six rows."""
    g = _gen(500000 + 1000 * k + n)
    pts = torch.randn((n, k + 1), generator=g)
    if n == 1:
        pts[0, k] = NH_W[(0, 1, 5)[k - 1]]
    else:
        pts[:6, k] = torch.tensor(NH_W)
        pts[-6:, k] = torch.tensor(NH_W[::-1])
    return pts


def _dep_specials():
    f = np.float32
    up, dn = f(np.inf), f(-np.inf)
    x256, x31 = f(2 * 256 / 255 - 1), f(2.0 ** 32 / 255)
    head = [np.nan, np.inf, -np.inf, 3e9, -3e9, -1.0, np.nextafter(f(-1), up), np.nextafter(f(-1), dn), 1.0,
            np.nextafter(f(1), up), x256, np.nextafter(x256, dn), x31, np.nextafter(x31, up), -x31, -1.004]
    tail = [np.nextafter(f(1), dn), np.nextafter(x256, up), np.nextafter(x31, dn), np.nextafter(-x31, up),
            np.nextafter(-x31, dn), -1.01, -1.5, 1e30, -1e30, np.nan, -3e9, 3e9, np.inf, -np.inf, -1.0078, 1.0]
    return torch.tensor(np.array(head, f)), torch.tensor(np.array(tail, f))


def codec_inputs(n):
    """(preprocess input in [0,1], deprocess input in [-1,1] with the special values at both ends)."""
    g = _gen(600000 + n)
    if n > 1000:  # a ramp whose period divides no block size
        i = torch.arange(n, dtype=torch.float32) % 251
        pre, dep = i / 255, i / 125 - 1
    else:
        pre, dep = torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1
    head, tail = _dep_specials()
    if n >= 32:
        dep[:16], dep[-16:] = head, tail
    else:
        dep[0] = 3e9
    return pre, dep


def boundary_inputs():
    """The 5x9 frames (45 pixels) of the fused kernels: rotated poses, seeded images."""
    g = _gen(700045)
    H, W, P = 5, 9, 5
    K2 = configs.f32([configs.intrinsics_matrix(6.0, 6.5, 4.5, 2.5), configs.intrinsics_matrix(7.0, 6.0, 4.0, 2.0)])
    pose2 = configs.f32([configs.pose_from(rot_axis(6.0, (0.6, 0.64, 0.48)), (0.05, -0.02, 0.03)),
                         configs.pose_from(rot_axis(-4.0, (0.48, 0.6, 0.64)), (-0.1, 0.04, 0.02))])
    return {
        "mpi": torch.rand((1, H, W, P, 4), generator=g), "planes": configs.f32([10.0, 5.0, 2.5, 1.6, 1.0]),
        "K": K2[:1].clone(), "pose": pose2[:1].clone(),
        "img": torch.rand((2, H, W, 3), generator=g), "depth": torch.rand((2, H, W), generator=g) * 5 + 1,
        "K2": K2, "pose2": pose2,
    }


def _ref_plane_coords(ref, pts, hom):
    """utils.py:178-188 with the reference's own functions."""
    c = ref.normalize_homogeneous_torch(ref.transform_points_torch(pts, hom))
    return c / torch.Tensor([pts.shape[-3] - 1, pts.shape[-2] - 1])


def _must(why, what):
    assert why is None, f"{what}: {why}"


def fused_counts(ref):
    """Reference against the fused kernels' always-FMA arithmetic below and at the 45-pixel contract."""
    import geometry_cases as gc
    from mpi_vision_amd import _host
    from oracle import oracle
    b = boundary_inputs()
    lines = []
    for Ht, Wt in ((2, 3), (4, 6), (5, 5), (4, 11), (5, 9)):
        depth = torch.full((1, Ht, Wt), 2.5)
        pix = ref.meshgrid_abs_torch(1, Ht, Wt)
        ki, proj = _host.psv_matrices(b["K"], b["K"], b["pose"])
        want = ref.cam2pixel_torch(ref.pixel2cam_torch(depth, pix, b["K"]), proj.reshape(1, 4, 4)).numpy()
        cam = gc.pixel2cam(depth.reshape(1, -1).numpy(), pix.reshape(1, 3, -1).numpy(), ki.reshape(1, 3, 3).numpy(),
                           True, False)
        got = gc.cam2pixel(cam, proj.reshape(1, 4, 4).numpy(), False).reshape(1, Ht, Wt, 2)
        lines.append(f"projection {Ht}x{Wt} ({Ht * Wt} px): {gc.ndiff(got, want)} of {want.size} pixel coordinates differ")
    for H, W in ((4, 5), (4, 11), (5, 9)):
        mpi = torch.rand((1, H, W, 5, 4), generator=_gen(710000 + 100 * H + W))
        K = configs.f32([configs.intrinsics_matrix(6.0, 6.5, W / 2, H / 2)])
        want = ref.mpi_render_view_torch(mpi, b["pose"], b["planes"], K).numpy()
        homs = _host.render_homographies(b["pose"], b["planes"], K, 1)
        got = oracle.render(mpi.numpy(), homs.numpy())
        d = np.abs(got.astype(np.float64) - want)
        pts = ref.meshgrid_abs_torch(1, H, W).permute(0, 2, 3, 1).unsqueeze(0).repeat(5, 1, 1, 1, 1)
        hom = homs.reshape(1, 5, 3, 3).permute(1, 0, 2, 3).contiguous()
        cref = _ref_plane_coords(ref, pts, hom).numpy()
        cfma = gc.plane_coords(pts.reshape(5, 1, H * W, 3).numpy(), hom.numpy(), H, W, False).reshape(cref.shape)
        lines.append(f"render {H}x{W}x5 ({H * W} px): {gc.ndiff(cfma, cref)} of {cref.size} sample coordinates and "
                     f"{gc.ndiff(got, want)} of {want.size} frame values differ, max |diff| {d.max():.3g}")
    return lines


def main():
    import geometry_cases as gc
    from gen_goldens import OUT, homographies, load_reference
    torch.set_num_threads(8)
    ref = load_reference()
    rec, shas = {}, {}

    for M, n in TP:
        pts, H = tp_inputs(M, n)
        out = ref.transform_points_torch(pts, H).numpy()
        plain = gc.tp_plain(n, M > 0)
        _must(gc.same(gc.transform_points(pts.numpy(), H.numpy()[..., None, :, :] if M else H.numpy(), plain), out),
              f"tp M={M} n={n}: the reference is not the {'plain' if plain else 'FMA'} chain")
        shas[f"tp_{M}_{n}"] = sha(pts, H)
        if n in TP_DIGEST_ONLY:  # 24 KB of incompressible floats: the restatement, held to this digest
            shas[f"tp_{M}_{n}_out"] = sha(out)
        else:
            rec[f"tp_{M}_{n}"] = out

    for B, n in P2C:
        depth, pix, K = p2c_inputs(B, n)
        out = ref.pixel2cam_torch(depth, pix, K).numpy()
        out3 = ref.pixel2cam_torch(depth, pix, K, is_homogeneous=False).numpy()
        assert out3.shape[1] == 3 and gc.same(out3, out[:, :3]) is None and (out[:, 3] == 1).all()
        ki = torch.inverse(K).numpy()
        plain = gc.p2c_plain(n)
        got = gc.pixel2cam(depth.reshape(B, n).numpy(), pix.reshape(B, 3, n).numpy(), ki, True, plain)
        _must(gc.same(got.reshape(out.shape), out), f"p2c B={B} n={n}: the reference is not the "
              f"{'plain' if plain else 'FMA'} chain")
        rec[f"p2c_{B}_{n}"], shas[f"p2c_{B}_{n}"], shas[f"p2c_{B}_{n}_h0"] = out, sha(depth, pix, K), sha(out3)
        rec[f"p2c_{B}_{n}_ki"] = ki  # torch.inverse is host-dependent: the reference's bits

    for B, n in C2P:
        cam, proj = c2p_inputs(B, n)
        out = ref.cam2pixel_torch(cam, proj).contiguous().numpy()
        plain = gc.c2p_plain(n)
        _must(gc.same(gc.cam2pixel(cam.reshape(B, 4, n).numpy(), proj.numpy(), plain).reshape(out.shape), out),
              f"c2p B={B} n={n}: the reference is not the {'plain' if plain else 'FMA'} chain")
        if n >= 24:
            z = gc.chain(proj.numpy(), cam.reshape(B, 4, n).numpy(), plain)[:, 2]
            assert np.isinf(out[B - 1, -1, -1]).all() and z[B - 1, -1] + gc.EPS_Z == 0 and (z < 0).any()
        rec[f"c2p_{B}_{n}"], shas[f"c2p_{B}_{n}"] = out, sha(cam, proj)

    for Ht, Wt in PC:
        cams = pc_cameras(Ht, Wt)
        hom = ref.inv_homography_torch(*cams)
        imgs, pts = pc_inputs(Ht, Wt, hom)
        coords = _ref_plane_coords(ref, pts.clone(), hom).numpy()
        out = ref.transform_plane_imgs_torch(imgs, pts.clone(), *cams).numpy()
        n = Ht * Wt
        plain = gc.tp_plain(n, True)
        got = gc.plane_coords(pts.reshape(2, 2, n, 3).numpy(), hom.numpy(), Ht, Wt, plain)
        _must(gc.same(got.reshape(coords.shape), coords), f"pc {Ht}x{Wt}: the reference is not the "
              f"{'plain' if plain else 'FMA'} chain")
        w = ref.transform_points_torch(pts.clone(), hom)[..., 2].reshape(2, 2, n)
        assert bool((w[:, 1, 1] == 0).all()) and bool((w[:, 1, -1] == 0).all()), "the affine planes' z == 0 points"
        assert bool((w[:, 0, 0] == 0).all()) == plain, "(h7, -h6, 0) cancels under the plain chain only"
        if Ht == 1 or Wt == 1:
            assert not np.isfinite(coords).all() and np.isfinite(coords).any()
        tag = f"pc_{Ht}x{Wt}"
        rec[tag + "_hom"], rec[tag + "_coords"], rec[tag + "_out"] = hom.numpy(), coords, out
        shas[tag] = sha(imgs, pts, *cams)

    for k, n in NH:
        pts = nh_inputs(k, n)
        work = pts.clone()
        out = ref.normalize_homogeneous_torch(work).numpy()
        want_out, want_after = gc.normalize_homogeneous(pts.numpy())
        _must(gc.same(out, want_out), f"nh k={k} n={n} out")
        _must(gc.same(work.numpy(), want_after), f"nh k={k} n={n}: the input after the call")
        zero = (pts[:, k] == 0).numpy()
        assert zero.any() or n == 1
        assert gc.same(work.numpy()[~zero], pts.numpy()[~zero]) is None, "only w == 0 rows are rewritten"
        assert (work.numpy()[zero, k] == gc.EPS_W).all() and gc.same(work.numpy()[:, :k], pts.numpy()[:, :k]) is None
        tag = f"nh_{k}_{n}"
        rec[tag + "_out"], rec[tag + "_w"] = out, work.numpy()[:, k].copy()
        shas[tag + "_after"], shas[tag] = sha(work), sha(pts)

    for n in CODEC_N:
        pre, dep = codec_inputs(n)
        pout, dout = ref.preprocess_image_torch(pre).numpy(), ref.deprocess_image_torch(dep).numpy()
        _must(gc.same(pout, gc.preprocess(pre.numpy())), f"preprocess n={n}")
        assert dout.dtype == np.uint8 and np.array_equal(dout, gc.deprocess_u8(dep.numpy())), f"deprocess n={n}"
        rec[f"pre_{n}"], rec[f"dep_{n}"], shas[f"codec_{n}"] = pout, dout, sha(pre, dep)
    _, dep = codec_inputs(257)
    v = ((dep.numpy() + np.float32(1)) / np.float32(2)) * np.float32(255)
    for edge in (0.0, 255.0, 256.0, 2.0 ** 31, -2.0 ** 31):  # at the edge or one ulp from it
        e = np.float32(edge)
        near = (v == e) | (v == np.nextafter(e, np.float32(np.inf))) | (v == np.nextafter(e, np.float32(-np.inf)))
        assert near[:16].any() or near[-16:].any(), f"no deprocess input scales to within 1 ulp of {edge}"

    b = boundary_inputs()
    rec["bd_render"] = ref.mpi_render_view_torch(b["mpi"], b["pose"], b["planes"], b["K"]).numpy()
    rec["bd_warp"] = ref.projective_inverse_warp_torch(b["img"], b["depth"], b["pose2"], b["K2"]).numpy()
    rec["bd_sweep"] = ref.plane_sweep_torch(b["img"], SWEEP_DEPTHS, b["pose2"], b["K2"]).numpy()
    # what the reference's host made of torch.inverse(K) (host-dependent bits): the render's homographies
    # [P,B,3,3] and the warps' K^-1 [2,3,3]; with them the kernels reproduce the goldens on any host
    rec["bd_homs"] = homographies(ref, b["pose"], b["planes"], b["K"]).numpy()
    rec["bd_ki"] = torch.inverse(b["K2"]).numpy()
    shas["bd"] = sha(*[b[k] for k in sorted(b)])
    for k in ("bd_render", "bd_warp", "bd_sweep"):
        assert np.isfinite(rec[k]).all() and (rec[k] != 0).mean() > 0.3, (k, float((rec[k] != 0).mean()))

    rec["shas"] = np.array(json.dumps(shas, sort_keys=True))
    path = os.path.join(OUT, "geometry.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:  # np.savez_compressed with fixed timestamps:
        for k, v in rec.items():                                  # the same bytes on every run
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(rec)} arrays, sha256 "
          f"{hashlib.sha256(open(path, 'rb').read()).hexdigest()[:16]}")
    for line in fused_counts(ref):
        print(line)


if __name__ == "__main__":
    main()
