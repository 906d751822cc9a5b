#!/usr/bin/env python3
"""Golden fixtures for the inverse warp's gradients: the reference's autograd gradient of
`projective_inverse_warp_torch` (utils.py:409-450) and `projective_inverse_warp_torch2`
(utils.py:725-769) with respect to the source image, the depth map, the pose and the intrinsics,
computed by running the reference's utils.py on CPU.  Test tooling only (see gen_goldens.py for how
the reference is imported); writes tests/golden/warpgrad.npz.

Inputs: the images, depth maps and poses of tests/golden/warp.npz (a depth-0 pixel and a
negative-depth block among them) with cameras of power-of-two focal lengths and dyadic principal
points, whose inverses are exact on any host, so the chain from dki / dproj to dpose
and dK reproduces bit for bit wherever the tests run.  A fourth case, `w1`, has a dout that is
non-zero at one pixel per view (an interior pixel, a frame corner, a pixel with exactly one corner
inside the source, one with none): every frame sum then has one term.

Intermediates are tapped without touching the reference: its module looks its functions and `torch`
up at call time, so pixel2cam_torch / cam2pixel_torch are wrapped with an identity that records the
gradient coming back, and the module's `torch` is a proxy whose matmul and inverse do the same for
their results.  Per case <c>:

    <c>_K (or _Ks, _Kt, _tgt), _dout      the inputs (images, depth maps and poses: warp.npz's; w1
                                          carries its own, one view of img and depth for the four)
    <c>_ki [B,9], _proj [B,16]                                      inverse(K_tgt), K4_src @ pose
    <c>_dimg, _ddepth, _dpose, _dK (or _dKs, _dKt)                  the reference's gradients
    <c>_dpix [B,Ht,Wt,2]      gradient at cam2pixel_torch's output
    <c>_dcam [B,4,Ht,Wt]      gradient at pixel2cam_torch's output
    <c>_duvw [B,4,N]          gradient at the proj @ cam product
    <c>_dki [B,9], _dproj [B,16]   gradients of inverse(K) and of K4 @ pose
    <c>_dki_S64, _dki_A, _dproj_S64, _dproj_A
                              float64 sums of the reference's own fp32 per-pixel factors' products
                              and of their magnitudes (as camgrad.npz)

The generator asserts that the reference's own dki / dproj lie inside gamma_N * A, and that at least
half of every full case's pixels have ddepth != 0 and half of its texels dimg != 0.

Usage:  python tools/gen_goldens_warpgrad.py
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
from gen_goldens_camgrad import Tap  # noqa: E402
from mpi_vision_amd import configs  # noqa: E402

FULL = ["piw", "piw4", "piw2"]


class TorchProxy:
    """The reference module's `torch`: matmul and inverse record their results and tap the gradients
    that come back (keys mm0, mm1, ... and inv0 in call order); everything else is torch's."""

    def __init__(self, store):
        self._store, self._n = store, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def matmul(self, a, b):
        key = f"mm{self._n}"
        self._n += 1
        out = torch.matmul(a, b)
        self._store[key] = out.detach().clone()
        return Tap.apply(out, self._store, "d" + key)

    def inverse(self, a):
        out = torch.inverse(a)
        self._store["inv0"] = out.detach().clone()
        return Tap.apply(out, self._store, "dinv0")


def tapped(ref, store):
    p2c, c2p, t = ref.pixel2cam_torch, ref.cam2pixel_torch, ref.torch

    def pixel2cam_torch(*a, **k):
        out = p2c(*a, **k)
        store["cam"] = out.detach().clone()
        return Tap.apply(out, store, "dcam")

    def cam2pixel_torch(*a, **k):
        out = c2p(*a, **k)
        store["pix"] = out.detach().clone()
        return Tap.apply(out, store, "dpix")

    ref.pixel2cam_torch, ref.cam2pixel_torch, ref.torch = pixel2cam_torch, cam2pixel_torch, TorchProxy(store)
    return p2c, c2p, t


def sums(d, c):
    """float64 sum over the pixels of d_r * c_k and of its magnitude: d [B,R,N], c [B,K,N] -> [B,R*K]."""
    prod = d.double().unsqueeze(2) * c.double().unsqueeze(1)  # exact in float64
    B = d.shape[0]
    return prod.sum(-1).reshape(B, -1), prod.abs().sum(-1).reshape(B, -1)


def run(ref, name, img, depth, pose, Ks, Kt, tgt, g, dout_fn=None):
    store = {}
    two = Kt is not None
    leaves = [x.clone().requires_grad_(True) for x in ((img, depth, pose, Ks, Kt) if two else (img, depth, pose, Ks))]
    saved = tapped(ref, store)
    try:
        if two:
            res = ref.projective_inverse_warp_torch2(*leaves, *tgt)
        else:
            res = ref.projective_inverse_warp_torch(*leaves)
        dout = dout_fn(store) if dout_fn else torch.rand(res.shape, generator=g) * 2 - 1
        res.backward(dout)
    finally:
        ref.pixel2cam_torch, ref.cam2pixel_torch, ref.torch = saved
    B, Ht, Wt = depth.shape
    N = Ht * Wt
    # call order: Ki @ pixels (pixel2cam), K4 @ pose, proj @ cam (cam2pixel)
    proj = store["mm1"]
    dray, dproj, duvw = store["dmm0"], store["dmm1"], store["dmm2"]
    ki, dki = store["inv0"], store["dinv0"]
    cam = store["cam"].reshape(B, 4, N)
    ys, xs = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(N)], 0).expand(B, 3, N)
    out = {f"{name}_dout": dout, f"{name}_ki": ki.reshape(B, 9), f"{name}_proj": proj.reshape(B, 16),
           f"{name}_dimg": leaves[0].grad, f"{name}_ddepth": leaves[1].grad, f"{name}_dpose": leaves[2].grad,
           f"{name}_dpix": store["dpix"], f"{name}_dcam": store["dcam"], f"{name}_duvw": duvw,
           f"{name}_dki": dki.reshape(B, 9), f"{name}_dproj": dproj.reshape(B, 16)}
    if dout_fn is not None:  # (the full cases' images, depth maps and poses are warp.npz's)
        out.update({f"{name}_img": img[:1], f"{name}_depth": depth[:1], f"{name}_pose": pose})
    if two:
        out.update({f"{name}_Ks": Ks, f"{name}_Kt": Kt, f"{name}_tgt": torch.tensor(tgt),
                    f"{name}_dKs": leaves[3].grad, f"{name}_dKt": leaves[4].grad})
    else:
        out.update({f"{name}_K": Ks, f"{name}_dK": leaves[3].grad})
    gamma = N * 2.0 ** -24 / (1 - N * 2.0 ** -24)
    for what, d, c, got in (("dki", dray, pc, dki.reshape(B, 9)), ("dproj", duvw, cam, dproj.reshape(B, 16))):
        fin = torch.isfinite(d).all(dim=1, keepdim=True) & torch.isfinite(c).all(dim=1, keepdim=True)
        if dout_fn is None and not bool(fin.all()):
            print(f"{name}: {int((~fin).sum())} pixels with non-finite {what} factors (sums not bounded)")
        S64, A = sums(d, c)
        out[f"{name}_{what}_S64"], out[f"{name}_{what}_A"] = S64, A
        if bool(torch.isfinite(S64).all()):
            err = (got.double() - S64).abs()
            assert bool((err <= gamma * A).all()), f"{name}: the reference's {what} is outside gamma_N * A"
            print(f"{name}: reference worst |{what} - S64| = "
                  f"{float((err / (A * 2.0 ** -24).clamp_min(1e-300)).max()):.3f} x 2^-24 A (bound {gamma * 2 ** 24:.0f})")
    fd = float((leaves[1].grad != 0).double().mean())
    fi = float((leaves[0].grad.abs().sum(-1) != 0).double().mean())
    print(f"{name}: pixels with ddepth != 0: {fd:.2f}, texels with dimg != 0: {fi:.2f}")
    if dout_fn is None:
        assert fd >= 0.5 and fi >= 0.5, f"{name}: too few live pixels / texels"
    for k in ("dpose", "dK", "dKs", "dKt"):
        if f"{name}_{k}" in out:
            assert out[f"{name}_{k}"] is not None and float(out[f"{name}_{k}"].abs().max()) > 0, f"{name}: {k}"
    return {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def corner_counts(pix, Hs, Ws):
    """Per target pixel: in-image corners of its sample (float64 restatement of the forward's position
    from cam2pixel_torch's output [B,Ht,Wt,2]) and whether the position is robustly off the lattice."""
    px = ((pix[..., 0].double() + 0.5) / Hs * 2) * (Ws / 2) - 0.5  # the reference's swapped [height, width]
    py = ((pix[..., 1].double() + 0.5) / Ws * 2) * (Hs / 2) - 0.5
    fx, fy = torch.floor(px), torch.floor(py)
    nx = ((fx >= 0) & (fx < Ws)).long() + ((fx + 1 >= 0) & (fx + 1 < Ws)).long()
    ny = ((fy >= 0) & (fy < Hs)).long() + ((fy + 1 >= 0) & (fy + 1 < Hs)).long()
    robust = ((px - fx) > 1e-3) & ((px - fx) < 1 - 1e-3) & ((py - fy) > 1e-3) & ((py - fy) < 1 - 1e-3)
    return nx * ny, robust


def single_pixel_dout(g, B, Hs, Ws, Ht, Wt, C, pix_out):
    """dout for `w1`: view i is non-zero at one pixel only: an interior sample, a frame corner, a
    sample with exactly one corner inside the source, and one with none."""

    def fn(store):
        counts, robust = corner_counts(store["pix"], Hs, Ws)
        counts, robust = counts[0], robust[0]  # every view shares camera and depth map

        def find(mask, what):
            idx = torch.nonzero(mask & robust)
            assert len(idx), f"w1: no pixel with {what}"
            y, x = idx[len(idx) // 2].tolist()
            return x, y

        pix = [find(counts == 4, "four corners inside"), (0, 0), find(counts == 1, "one corner inside"),
               find(counts == 0, "no corner inside")]
        dout = torch.zeros((B, Ht, Wt, C))
        for i, (x, y) in enumerate(pix):
            dout[i, y, x] = torch.rand(C, generator=g) * 2 - 1
        pix_out.extend(pix)
        return dout

    return fn


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    w = np.load(os.path.join(OUT, "warp.npz"))
    g = torch.Generator().manual_seed(277)
    t = lambda k: torch.from_numpy(w[k])  # noqa: E731
    K = lambda *cams: f32([configs.intrinsics_matrix(*c) for c in cams])  # noqa: E731
    out = {}
    out.update(run(ref, "piw", t("piw_img"), t("piw_depth"), t("piw_pose"),
                   K((32.0, 32.0, 22.0, 15.0), (32.0, 64.0, 21.0, 14.5)), None, None, g))
    out.update(run(ref, "piw4", t("piw4_img"), t("piw4_depth"), t("piw4_pose"), K((32.0, 32.0, 12.0, 12.0)),
                   None, None, g))
    Ht, Wt = (int(v) for v in w["piw2_tgt"])
    out.update(run(ref, "piw2", t("piw2_img"), t("piw2_depth"), t("piw2_pose"),
                   K((32.0, 32.0, 24.0, 18.0), (64.0, 64.0, 23.0, 17.0)),
                   K((64.0, 64.0, 35.0, 14.0), (64.0, 32.0, 34.0, 13.5)), (Ht, Wt), g))
    # w1: four views of one camera and one (positive, finite) depth map; one live dout pixel each
    B, Hs, Ws, C = 4, 24, 32, 3
    img = torch.rand((1, Hs, Ws, C), generator=g).expand(B, Hs, Ws, C).contiguous()
    depth = (torch.rand((1, Hs, Ws), generator=g) * 6 + 0.8).expand(B, Hs, Ws).contiguous()
    pose = f32([rand_pose(g, 0.1, 0.3)] * B)
    pix = []
    out.update(run(ref, "w1", img, depth, pose, K(*[(32.0, 32.0, 16.0, 12.0)] * B), None, None, g,
                   dout_fn=single_pixel_dout(g, B, Hs, Ws, Hs, Ws, C, pix)))
    out["w1_pixels"] = np.array(pix, dtype=np.int64)  # (x, y) of view i's only non-zero dout pixel
    for what in ("dki", "dproj"):  # one non-zero term per sum: the reference's value is that product exactly
        d = torch.from_numpy(out[f"w1_{what}"])
        assert bool((d == torch.from_numpy(out[f"w1_{what}_S64"]).float()).all()), f"w1: {what} is not one product"
    live = [bool(np.abs(out["w1_dproj"][i]).sum() > 0) for i in range(B)]
    print("w1 pixels (x, y):", pix, "views with a non-zero dproj:", live)
    assert live[0] and live[2] and not live[3]
    path = os.path.join(OUT, "warpgrad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
