#!/usr/bin/env python3
"""Golden fixtures for the plane sweep's gradients: the reference's autograd gradient of
`plane_sweep_torch` (utils.py:452-471), `plane_sweep_torch_one2` (utils.py:771-799) and
`format_network_input_torch` (utils.py:473-498) with respect to the source image(s), the plane depths
(`depth_planes` as a leaf tensor), the pose(s) and the intrinsics, computed by running the reference's
utils.py on CPU.  Test tooling only (see gen_goldens.py for how the reference is imported); writes
tests/golden/psvgrad.npz.

The reference's sweep is D calls of projective_inverse_warp_torch[2] and a torch.cat, so every call is
wrapped: its image and its constant depth map pass through an identity that records the gradient coming
back (the per-depth d img and the per-pixel d depth), and its intermediates are tapped as
gen_goldens_warpgrad.py taps the inverse warp's.  All cameras have power-of-two focal lengths and dyadic
principal points (exact inverses on any host); images and dout are multiples of 1/256 and 1/128.

Cases: psv (B=2, two cameras, 30x44, C=3, D=6, one depth repeated), psv1 (psv's inputs, its first depth
and the first C channels of its dout), psv33 (B=1, 24x32, C=1, D=33), one2 (plane_sweep_torch_one2, source
36x48, target 20x28, C=5, D=3), fni (format_network_input_torch, B=1, 24x32, S=2 sources, D=4).
Per case <c> (fni: a leading source axis S on the per-source entries):

    <c>_img, _depths, _pose, _K (or _Ks, _Kt, _tgt), _dout           the inputs
        (fni: _ref, _src, _ref_pose, _src_poses, _K, _depths, _dout)
    <c>_dimg, _ddepths, _dpose, _dK (or _dKs, _dKt)                  the reference's gradients
        (fni: _dref, _dsrc, _dref_pose, _dsrc_poses, _dK, _ddepths)
    <c>_dimg_d [D,B,Hs,Ws,C]     the per-depth image gradients
    <c>_ddepth_d [D,B,Ht,Wt]     the per-depth per-pixel depth gradients
    <c>_ki [B,9], _proj [B,16]   inverse(K_tgt), K4_src @ pose
    <c>_dki [B,9], _dproj [B,16] the per-depth gradients of inverse(K) and K4 @ pose, added in descending d
    <c>_dki_S64, _dki_A, _dproj_S64, _dproj_A, _ddepths_S64, _ddepths_A
                                 float64 sums of the reference's own fp32 per-pixel terms and of their
                                 magnitudes, over all depths (dki, dproj) or all views (ddepths)

The generator asserts, for every case: the descending-d fold of dimg_d equals dimg bit for bit (and the
taps change no bit of it); the ascending fold differs from it in at least 1 % of the elements (D > 1); at
least half of the texels have dimg != 0; the reference's own sums lie inside gamma_N * A.

Usage:  python tools/gen_goldens_psvgrad.py
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
from gen_goldens_warpgrad import sums, tapped  # noqa: E402
from mpi_vision_amd import configs  # noqa: E402

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def wrap_warps(ref, stores):
    """Every projective_inverse_warp_torch[2] call of the sweep gets a store of its own, appended to
    `stores` in call order."""
    piw, piw2 = ref.projective_inverse_warp_torch, ref.projective_inverse_warp_torch2

    def wrap(fn):
        def inner(img, depth, *rest, **kw):
            store = {}
            stores.append(store)
            saved = tapped(ref, store)
            try:
                return fn(Tap.apply(img, store, "dimg"), Tap.apply(depth, store, "ddepth"), *rest, **kw)
            finally:
                ref.pixel2cam_torch, ref.cam2pixel_torch, ref.torch = saved
        return inner

    ref.projective_inverse_warp_torch, ref.projective_inverse_warp_torch2 = wrap(piw), wrap(piw2)
    return piw, piw2


def fold(parts, descending):
    order = list(reversed(parts)) if descending else list(parts)
    acc = order[0]
    for p in order[1:]:
        acc = acc + p
    return acc


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def source_entries(name, stores, dimg, Ht, Wt, ddepths=None):
    """The per-depth taps of one source's D calls and the assertions on them; dimg [B,Hs,Ws,C] is the
    reference's gradient of that source, ddepths [D] that of its depths (when it has them alone)."""
    D = len(stores)
    dimg = dimg.contiguous()
    B = dimg.shape[0]
    N = Ht * Wt
    dimg_d = [s["dimg"] for s in stores]
    ddepth_d = [s["ddepth"].reshape(B, Ht, Wt) for s in stores]
    assert bits_equal(fold(dimg_d, True), dimg), f"{name}: the descending-d fold is not the reference's dimg"
    if D > 1:
        diff = float((fold(dimg_d, False).view(torch.int32) != dimg.view(torch.int32)).double().mean())
        print(f"{name}: the ascending fold differs from dimg in {100 * diff:.1f} % of the elements")
        assert diff >= 0.01, f"{name}: the two fold orders cannot be told apart"
    live = float((dimg.abs().sum(-1) != 0).double().mean())
    print(f"{name}: texels with dimg != 0: {live:.2f}")
    assert live >= 0.5, f"{name}: too few live texels"
    ys, xs = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(N)], 0).expand(B, 3, N)
    ki, proj = stores[0]["inv0"].reshape(B, 9), stores[0]["mm1"].reshape(B, 16)
    out = {"dimg_d": torch.stack(dimg_d), "ddepth_d": torch.stack(ddepth_d), "ki": ki, "proj": proj}
    tot = {}
    for what, dk, ck, gk, n in (("dki", "dmm0", None, "dinv0", 9), ("dproj", "dmm2", "cam", "dmm1", 16)):
        S64 = torch.zeros((B, n), dtype=torch.float64)
        A = torch.zeros((B, n), dtype=torch.float64)
        for s in stores:
            assert bits_equal(s["inv0"].reshape(B, 9), ki) and bits_equal(s["mm1"].reshape(B, 16), proj)
            c = pc if ck is None else s[ck].reshape(B, 4, N)
            s64, a = sums(s[dk], c)
            S64, A = S64 + s64, A + a
        got = fold([s[gk].reshape(B, n) for s in stores], True)
        out[what], out[what + "_S64"], out[what + "_A"] = got, S64, A
        tot[what] = (got, S64, A, D * N)
    S64 = torch.stack([m.double().sum() for m in ddepth_d])
    A = torch.stack([m.double().abs().sum() for m in ddepth_d])
    out["ddepths_S64"], out["ddepths_A"] = S64, A
    if ddepths is not None:
        tot["ddepths"] = (ddepths, S64, A, B * N)
    for what, (got, S64, A, n) in tot.items():
        assert bool(torch.isfinite(S64).all()), f"{name}: non-finite {what}"
        err = (got.double() - S64).abs()
        assert bool((err <= gamma(n) * A).all()), f"{name}: the reference's {what} is outside gamma_N * A"
        print(f"{name}: reference worst |{what} - S64| = {float((err / (A * U).clamp_min(1e-300)).max()):.3f} x 2^-24 A "
              f"(bound {gamma(n) / U:.0f})")
    return out


def quant(g, shape, levels, signed):
    """Multiples of 1 / levels in [0, 1) or [-1, 1)."""
    lo = -levels if signed else 0
    return torch.randint(lo, levels, shape, generator=g).float() / levels


def run(ref, name, fn, leaves, grads, dout, Ht, Wt, img_key="img"):
    """One plane sweep case: fn(ref, **leaves) -> volume; returns the npz entries."""
    plain = {k: v.clone().requires_grad_(k in grads) for k, v in leaves.items()}
    fn(ref, **plain).backward(dout)
    ts = {k: v.clone().requires_grad_(k in grads) for k, v in leaves.items()}
    stores = []
    saved = wrap_warps(ref, stores)
    try:
        res = fn(ref, **ts)
        assert tuple(res.shape) == tuple(dout.shape)
        res.backward(dout)
    finally:
        ref.projective_inverse_warp_torch, ref.projective_inverse_warp_torch2 = saved
    for k in grads:
        assert bits_equal(ts[k].grad, plain[k].grad), f"{name}: the taps changed d {k}"
        assert float(ts[k].grad.abs().max()) > 0 and bool(torch.isfinite(ts[k].grad).all()), f"{name}: d {k}"
    dimg = ts[img_key].grad
    if dimg.dim() == 3:
        dimg = dimg.unsqueeze(0)
    ent = source_entries(name, stores, dimg, Ht, Wt, ts["depths"].grad)
    out = {f"{name}_{k}": v for k, v in ent.items()}
    out.update({f"{name}_{k}": v for k, v in leaves.items()})
    out.update({f"{name}_d{k}": ts[k].grad for k in grads})
    out[f"{name}_dout"] = dout
    return {k: v.detach().numpy() for k, v in out.items()}


def run_fni(ref, name, leaves, dout, S, D):
    grads = list(leaves)
    call = lambda t: ref.format_network_input_torch(None, t["ref"], t["src"], t["ref_pose"], t["src_poses"],  # noqa: E731
                                                    t["depths"], t["K"])
    plain = {k: v.clone().requires_grad_() for k, v in leaves.items()}
    call(plain).backward(dout)
    ts = {k: v.clone().requires_grad_() for k, v in leaves.items()}
    stores = []
    saved = wrap_warps(ref, stores)
    try:
        res = call(ts)
        assert tuple(res.shape) == tuple(dout.shape)
        res.backward(dout)
    finally:
        ref.projective_inverse_warp_torch, ref.projective_inverse_warp_torch2 = saved
    for k in grads:
        assert bits_equal(ts[k].grad, plain[k].grad), f"{name}: the taps changed d {k}"
        assert float(ts[k].grad.abs().max()) > 0 and bool(torch.isfinite(ts[k].grad).all()), f"{name}: d {k}"
    assert len(stores) == S * D and bits_equal(ts["ref"].grad, dout[..., :3])
    _, H, W, _ = leaves["ref"].shape
    per = [source_entries(f"{name}[{i}]", stores[i * D:(i + 1) * D], ts["src"].grad[..., 3 * i:3 * i + 3], H, W)
           for i in range(S)]
    err = (ts["depths"].grad.double() - sum(p["ddepths_S64"] for p in per)).abs()
    assert bool((err <= gamma(S * H * W) * sum(p["ddepths_A"] for p in per)).all()), f"{name}: ddepths"
    out = {f"{name}_{k}": torch.stack([p[k] for p in per]) for k in per[0]}
    out.update({f"{name}_{k}": v for k, v in leaves.items()})
    out.update({f"{name}_d{k}": ts[k].grad for k in grads})
    out[f"{name}_dout"] = dout
    return {k: v.detach().numpy() for k, v in out.items()}


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    g = torch.Generator().manual_seed(452)
    K = lambda *cams: f32([configs.intrinsics_matrix(*c) for c in cams])  # noqa: E731
    out = {}

    # psv / psv1: two cameras, one depth repeated
    B, H, W, C = 2, 30, 44, 3
    img = quant(g, (B, H, W, C), 256, False)
    pose = f32([rand_pose(g, 0.08, 0.25), rand_pose(g, 0.08, 0.25)])
    Kc = K((32.0, 32.0, 22.0, 15.0), (32.0, 64.0, 21.0, 14.5))
    depths = torch.tensor([8.0, 4.0, 2.5, 2.5, 1.75, 1.25])
    dout = quant(g, (B, H, W, len(depths) * C), 128, True)
    sweep = lambda r, img, depths, pose, K: r.plane_sweep_torch(img, depths, pose, K)  # noqa: E731
    grads = ("img", "depths", "pose", "K")
    out.update(run(ref, "psv", sweep, {"img": img, "depths": depths, "pose": pose, "K": Kc}, grads, dout, H, W))
    one = run(ref, "psv1", sweep, {"img": img, "depths": depths[:1].clone(), "pose": pose, "K": Kc}, grads,
              dout[..., :C].contiguous(), H, W)
    for k in ("img", "pose", "K", "dout", "depths"):  # psv's own: the tests slice them
        assert np.array_equal(one[f"psv1_{k}"], out[f"psv_{k}"][..., :C] if k == "dout" else
                              out[f"psv_{k}"][:1] if k == "depths" else out[f"psv_{k}"])
        del one[f"psv1_{k}"]
    out.update(one)

    # psv33: the forward's two-pixels-per-lane staged kernel; 33 planes do not divide into equal groups
    B, H, W, C = 1, 24, 32, 1
    img = quant(g, (B, H, W, C), 256, False)
    depths = 1.0 / torch.linspace(1.0 / 9.0, 1.0, 33)
    dout = quant(g, (B, H, W, 33 * C), 128, True)
    out.update(run(ref, "psv33", sweep, {"img": img, "depths": depths, "pose": f32([rand_pose(g, 0.08, 0.25)]),
                                         "K": K((32.0, 32.0, 16.0, 12.0))}, grads, dout, H, W))

    # one2: plane_sweep_torch_one2, separate source and target cameras and sizes
    Hs, Ws, Ht, Wt, C = 36, 48, 20, 28, 5
    img = quant(g, (Hs, Ws, C), 256, False)
    depths = torch.tensor([6.0, 2.5, 1.5])
    dout = quant(g, (1, Ht, Wt, 3 * C), 128, True)
    one2 = lambda r, img, depths, pose, Ks, Kt: r.plane_sweep_torch_one2(img, depths, pose, Ks, Kt, Ht, Wt)  # noqa: E731
    ent = run(ref, "one2", one2, {"img": img, "depths": depths, "pose": f32(rand_pose(g, 0.08, 0.25)),
                                  "Ks": K((32.0, 32.0, 18.0, 24.0))[0], "Kt": K((32.0, 16.0, 14.0, 10.0))[0]},
              ("img", "depths", "pose", "Ks", "Kt"), dout, Ht, Wt)
    ent["one2_tgt"] = np.array([Ht, Wt], dtype=np.int64)
    out.update(ent)

    # fni: format_network_input_torch, two sources; a reference pose whose inverse is exact (identity
    # rotation, dyadic translation)
    B, H, W, S, D = 1, 24, 32, 2, 4
    ref_pose = torch.eye(4)[None].clone()
    ref_pose[0, :3, 3] = torch.tensor([0.125, -0.0625, 0.25])
    leaves = {"ref": quant(g, (B, H, W, 3), 256, False), "src": quant(g, (B, H, W, 3 * S), 256, False),
              "ref_pose": ref_pose, "src_poses": f32([[rand_pose(g, 0.08, 0.25), rand_pose(g, 0.08, 0.25)]]),
              "depths": torch.tensor([8.0, 3.0, 1.75, 1.25]), "K": K((32.0, 32.0, 16.0, 12.0))}
    out.update(run_fni(ref, "fni", leaves, quant(g, (B, H, W, 3 + S * D * 3), 128, True), S, D))

    path = os.path.join(OUT, "psvgrad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
