#!/usr/bin/env python3
"""Golden fixtures for the render's CAMERA gradients: the reference's autograd gradient of
`mpi_render_view_torch` (utils.py:267-294) with respect to tgt_pose, planes and intrinsics,
computed by running the reference's utils.py on CPU.  Test tooling only (see gen_goldens.py for
how the reference is imported); writes tests/golden/camgrad.npz.

Two intermediate gradients are recorded on the way: d frame / d homographies (the output of
inv_homography_torch, utils.py:44-67) and, per pixel, d frame / d (u, v, w) (the output of
transform_points_torch, utils.py:69-88).  The reference forms its divisor with an in-place
`den +=` on a view, which retain_grad does not survive, so both functions are wrapped with an
identity autograd.Function that clones its input and records the incoming gradient.

Per case: pose, K, depths, dout; the reference's dH [B,P,9], dpose, dplanes, dK, dmpi; and
S64 = sum(d_r * c), A = sum(|d_r * c|) over the frame, both float64 [B,P,9], formed in float64 from
the reference's own fp32 per-pixel (du, dv, dw) and c in (x, y, 1) -- the reference value and the
scale of the standard error bound of an fp32 sum of N = H*W rounded products in any order,
gamma_N * A with gamma_N = N u / (1 - N u), u = 2^-24.  The generator asserts that the reference's own
dH is inside that bound.  The MPIs are regenerated from their seeds (configs.synthetic_mpi).

Cameras have power-of-two focal lengths and dyadic principal points: their inverses are exact on any
host (LAPACK's inverse is host-dependent otherwise), so the chain from dH to dpose,
dplanes and dK reproduces bit for bit wherever the tests run.

Usage:  python tools/gen_goldens_camgrad.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from gen_goldens import OUT, f32, load_reference, rand_pose  # noqa: E402
from mpi_vision_amd import configs  # noqa: E402

# name -> (B, H, W, P, MPI seed, broadcast); tests/test_camgrad*.py regenerate the MPIs from these
CASES = {
    "ca": (2, 23, 35, 5, 41, False),
    "cb": (1, 24, 32, 17, 42, False),
    "cl": (1, 32, 96, 9, 43, False),
    "cf": (1, 36, 48, 5, 44, False),
    "cbc": (3, 23, 35, 4, 45, True),
    "c1": (8, 24, 32, 5, 46, False),
}


class Tap(torch.autograd.Function):
    """Identity that clones its input and records the gradient that comes back."""

    @staticmethod
    def forward(ctx, x, store, key):
        ctx.store, ctx.key = store, key
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.store[ctx.key] = g.detach().clone()
        return g, None, None


def tapped(ref, store):
    """Wrap the reference's inv_homography_torch and transform_points_torch outputs with Tap (the
    module's other functions look them up as globals at call time)."""
    inv_h, tp = ref.inv_homography_torch, ref.transform_points_torch

    def inv_homography_torch(*a):
        return Tap.apply(inv_h(*a), store, "dH")

    def transform_points_torch(points, homography):
        out = tp(points, homography)
        store["uvw"] = out.detach().clone()
        return Tap.apply(out, store, "duvw")

    ref.inv_homography_torch, ref.transform_points_torch = inv_homography_torch, transform_points_torch
    return inv_h, tp


def tap_counts(uvw, H, W):
    """Per (plane, view, y, x): in-image taps of the sample (float64 restatement of the forward's
    position), and whether the position is at least 1e-3 away from every integer (a robust count)."""
    u, v, w = (uvw[..., k].double() for k in range(3))
    px = (u / w / (H - 1) * 2) * (W / 2) - 0.5  # the reference's swapped normalisation
    py = (v / w / (W - 1) * 2) * (H / 2) - 0.5
    fx, fy = torch.floor(px), torch.floor(py)
    nx = ((fx >= 0) & (fx < W)).long() + ((fx + 1 >= 0) & (fx + 1 < W)).long()
    ny = ((fy >= 0) & (fy < H)).long() + ((fy + 1 >= 0) & (fy + 1 < H)).long()
    robust = ((px - fx) > 1e-3) & ((px - fx) < 1 - 1e-3) & ((py - fy) > 1e-3) & ((py - fy) < 1 - 1e-3)
    return nx * ny, robust


def run(ref, name, K, poses, depths, g, dout_fn=None):
    B, H, W, P, seed, broadcast = CASES[name]
    store = {}
    mpi = configs.synthetic_mpi(1 if broadcast else B, H, W, P, seed)
    leaf = mpi.clone().requires_grad_(True)
    inp = leaf.expand(B, H, W, P, 4) if broadcast else leaf
    pose, planes, Kl = (x.clone().requires_grad_(True) for x in (poses, depths, K))
    saved = tapped(ref, store)
    try:
        res = ref.mpi_render_view_torch(inp, pose, planes, Kl)
        dout = dout_fn(store["uvw"]) if dout_fn else torch.rand(res.shape, generator=g) * 2 - 1
        res.backward(dout)
    finally:
        ref.inv_homography_torch, ref.transform_points_torch = saved
    dH = store["dH"].permute(1, 0, 2, 3).reshape(B, P, 9).contiguous()
    d3 = store["duvw"].reshape(P, B, H, W, 3).double()  # the reference's fp32 (du, dv, dw), exactly
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64),
                            indexing="ij")
    c = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)  # [H, W, 3]
    prod = d3.unsqueeze(-1) * c.reshape(1, 1, H, W, 1, 3)  # [P,B,H,W,r,c]: exact in float64
    S64 = prod.sum(dim=(2, 3)).permute(1, 0, 2, 3).reshape(B, P, 9)
    A = prod.abs().sum(dim=(2, 3)).permute(1, 0, 2, 3).reshape(B, P, 9)
    N = H * W
    gamma = N * 2.0 ** -24 / (1 - N * 2.0 ** -24)
    err = (dH.double() - S64).abs()
    assert bool((err <= gamma * A).all()), f"{name}: the reference's dH is outside gamma_N * A"
    assert bool(torch.isfinite(dH).all()) and float(A.max()) > 0
    for t, what in ((pose.grad, "dpose"), (planes.grad, "dplanes"), (Kl.grad, "dK")):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, f"{name}: {what}"
    ratio = float((err / (A * 2.0 ** -24).clamp_min(1e-300)).max())
    counts, _ = tap_counts(store["uvw"].reshape(P, B, H, W, 3), H, W)
    print(f"{name}: reference worst |dH - S64| = {ratio:.3f} x 2^-24 A (bound {gamma * 2 ** 24:.0f}), "
          f"samples with no tap inside: {float((counts == 0).double().mean()):.3f}")
    return {f"{name}_pose": poses.numpy(), f"{name}_K": K.numpy(), f"{name}_depths": depths.numpy(),
            f"{name}_dout": dout.numpy(), f"{name}_dH": dH.numpy(), f"{name}_dpose": pose.grad.numpy(),
            f"{name}_dplanes": planes.grad.numpy(), f"{name}_dK": Kl.grad.numpy(),
            f"{name}_dmpi": leaf.grad.numpy(), f"{name}_S64": S64.numpy(), f"{name}_A": A.numpy()}


def single_pixel_dout(g, B, H, W, P, pix_out):
    """dout for `c1`: view i is non-zero at one pixel only.  The eight pixels: two frame corners, an
    edge, two interior pixels, one whose sample (of some plane) has exactly one tap in the image, one
    with exactly two, and one with none in any plane."""

    def fn(uvw):
        counts, robust = tap_counts(uvw.reshape(P, B, H, W, 3), H, W)
        counts, robust = counts[:, 0], robust[:, 0]  # every view shares the pose
        ok = robust.all(dim=0)

        def find(mask, what):
            idx = torch.nonzero(mask & ok)
            assert len(idx), f"c1: no pixel with {what}"
            y, x = idx[len(idx) // 2].tolist()
            return x, y

        pix = [(0, 0), (W - 1, H - 1), (W // 3, 0), (10, 12), (17, 7),
               find((counts == 1).any(dim=0), "one tap inside"), find((counts == 2).any(dim=0), "two taps inside"),
               find((counts == 0).all(dim=0), "no tap inside")]
        assert (counts[:, pix[3][1], pix[3][0]] == 4).all()
        dout = torch.zeros((B, H, W, 3))
        for i, (x, y) in enumerate(pix):
            dout[i, y, x] = torch.rand(3, generator=g) * 2 - 1
        pix_out.extend(pix)
        return dout

    return fn


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    g = torch.Generator().manual_seed(177)
    out = {}
    small = lambda: rand_pose(g, 0.05, 0.1)  # noqa: E731
    K = lambda *a, n=1: f32([configs.intrinsics_matrix(*a)] * n)  # noqa: E731
    out.update(run(ref, "ca", f32([configs.intrinsics_matrix(32, 32, 17.5, 11.5),
                                   configs.intrinsics_matrix(64, 32, 16, 12)]),
                   f32([configs.pose_from(configs.rot_y(2.0), (0.06, -0.03, 0.05)), small()]),
                   f32(ref.inv_depths(1, 100, 5)), g))
    out.update(run(ref, "cb", K(32, 32, 16, 12), f32([small()]), f32(ref.inv_depths(1, 100, 17)), g))
    out.update(run(ref, "cl", K(64, 64, 48, 16), f32([small()]), f32(ref.inv_depths(1, 100, 9)), g))
    out.update(run(ref, "cf", K(32, 32, 24, 18), f32([rand_pose(g, 0.8, 1.5)]), f32(ref.inv_depths(0.5, 10, 5)), g))
    out.update(run(ref, "cbc", K(32, 32, 17.5, 11.5, n=3), f32([small() for _ in range(3)]),
                   f32(ref.inv_depths(1, 100, 4)), g))
    B, H, W, P = CASES["c1"][:4]
    pix = []
    out.update(run(ref, "c1", K(32, 32, 16, 12, n=B), f32([small()] * B), f32(ref.inv_depths(1, 100, P)), g,
                   dout_fn=single_pixel_dout(g, B, H, W, P, pix)))
    out["c1_pixels"] = np.array(pix, dtype=np.int64)  # (x, y) of view i's only non-zero dout pixel
    # c1: every sum has one non-zero term, so the reference's dH is that product exactly
    d = torch.from_numpy(out["c1_dH"])
    assert bool((d == torch.from_numpy(out["c1_S64"]).float()).all()), "c1: dH is not the single rounded product"
    live = d.abs().sum(dim=(1, 2)).gt(0).tolist()  # (a corner of this frame may have no tap inside either)
    print("c1 pixels (x, y):", pix, "views with a non-zero dH:", live)
    assert not live[7] and live[0] and all(live[2:7])
    path = os.path.join(OUT, "camgrad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
