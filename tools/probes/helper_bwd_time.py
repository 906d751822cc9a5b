#!/usr/bin/env python3
"""Device time of the sampler's and the compositor's adjoints (helper_bwd.hip).

Sampler (4x224x224x3 and 1x1024x1024x3): mpiv_grid_sample_backward for d imgs + d coords beside
mpiv_inverse_warp_backward for d img + d depth at the same sample positions (the coordinates are the
warp's own (pixel + 0.5) / size), the two alternated in one process, the old entry measured twice per
round: the difference between its two measurements is the run-to-run spread the new entry is held to (it
runs the same sort and gather).  torch-ROCm's own grid_sample forward + backward is reported beside them.

Compositor (1024x1024, P = 32 and 128): over_composite forward + backward through the HIP entries against
torch autograd through the reference's formula on the device (what a caller ran before), their ratio, and
the backward's share of the HBM peak over its algorithmic bytes (3 * P * n * 16 B: every layer read twice
and its gradient written, plus the checkpoints written and read).

bench.py's method: launches back to back on preallocated inputs after at least 60 ms of warm-up
launches, HIP events on the launch stream.

    python tools/probes/helper_bwd_time.py [--out profiles/helper_bwd.jsonl] [--reps 5] [--n 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from bench import span_ms, warm  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402

SAMPLER_SHAPES = [(4, 224, 224, 3), (1, 1024, 1024, 3)]
OVER_SHAPES = [(1024, 1024, 32), (1024, 1024, 128)]
HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def med(xs):
    return round(float(np.median(xs)), 4)


def sampler(B, H, W, C, dev, stream, reps, n):
    g = torch.Generator(device=dev).manual_seed(9)
    img = torch.rand((B, H, W, C), generator=g, device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    depth = (1.0 + xx / W + 0.5 * yy / H).expand(B, H, W) + torch.rand((B, H, W), generator=g, device=dev)
    dout = torch.rand((B, H, W, C), generator=g, device=dev) * 2 - 1
    K = configs.f32([configs.intrinsics_matrix(0.9 * W, 0.9 * W, W / 2.0, H / 2.0)] * B)
    pose = configs.f32([configs.pose_from(configs.rot_y(2.0), (0.05, -0.02, 0.03))] * B)
    ki, proj = (t.to(dev) for t in _host.psv_matrices(K, K, pose))
    q = _lib._stream(dev)
    L = _lib.load()
    # the warp's own coordinates (cam2pixel of the same matrices; H == W, so its x / H is x / W)
    pc = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, device=dev)], 0).expand(B, 3, H * W).contiguous()
    cam = torch.empty((B, 4, H, W), device=dev)
    _lib._call("mpiv_pixel2cam", depth.contiguous(), pc, ki, B, H * W, 1, cam, q)
    coords = ((_lib.cam2pixel(cam, proj) + 0.5) / torch.tensor([float(H), float(W)], device=dev)).contiguous()
    same = bool(torch.equal(_lib.bilinear_sample(img, coords, True), _lib.inverse_warp_depthmap(img, depth, ki, proj, H, W)))
    ws = torch.empty(max(L.mpiv_inverse_warp_backward_workspace_size(B, H, W, C, H, W),
                         L.mpiv_grid_sample_backward_workspace_size(B, C, H, W, H, W)), dtype=torch.uint8, device=dev)
    dimg, ddepth, dco = torch.empty((B, H, W, C), device=dev), torch.empty((B, H, W), device=dev), torch.empty((B, H, W, 2), device=dev)
    si, sd, so = _lib._strides(img), _lib._strides(depth), _lib._strides(dout)
    si4, so4, sc = _lib._strides(img, (0, 3, 1, 2)), _lib._strides(dout, (0, 3, 1, 2)), _lib._strides(coords)

    def old():
        _lib._call("mpiv_inverse_warp_backward", img, si, B, H, W, C, ki, proj, depth, sd, H, W, dout, so, ddepth, dimg,
                   None, None, ws, ws.numel(), q)

    def new():
        _lib._call("mpiv_grid_sample_backward", img, si4, B, C, H, W, coords, sc, H, W, dout, so4, dimg, dco, ws,
                   ws.numel(), q)

    old()
    want = dimg.clone()
    new()
    same_dimg = bool(torch.equal(want.view(torch.int32), dimg.view(torch.int32)))
    grid = (-1 + 2 * coords).requires_grad_()
    leaf = img.permute(0, 3, 1, 2).contiguous().requires_grad_()
    dnchw = dout.permute(0, 3, 1, 2).contiguous()

    def torch_fb():
        r = F.grid_sample(leaf, grid, align_corners=False)
        torch.autograd.grad(r, (leaf, grid), dnchw)

    for fn in (old, new, torch_fb):
        warm(fn, stream, min_ms=60)
    a, b, a2, t = [], [], [], []
    for _ in range(reps):  # alternated: old, new, old again
        a.append(span_ms(old, n, stream))
        b.append(span_ms(new, n, stream))
        a2.append(span_ms(old, n, stream))
        t.append(span_ms(torch_fb, n, stream))
    spread = max(abs(x - y) for x, y in zip(a, a2))
    old_ms = med(a + a2)
    return {"what": "sampler", "shape": [B, H, W, C], "same_forward_bits": same, "same_dimg_bits": same_dimg,
            "grid_sample_backward_ms": med(b), "grid_sample_backward_reps": [round(x, 4) for x in b],
            "inverse_warp_backward_ms": old_ms, "inverse_warp_backward_reps": [round(x, 4) for x in a + a2],
            "old_entry_spread_ms": round(spread, 4), "new_minus_old_ms": round(med(b) - old_ms, 4),
            "within_spread": bool(med(b) <= old_ms + spread),
            "torch_grid_sample_fwd_bwd_ms": med(t), "workspace_bytes": ws.numel()}


def compositor(H, W, P, dev, stream, reps, n):
    g = torch.Generator(device=dev).manual_seed(11)
    npx = H * W
    layers = [torch.rand((1, H, W, 4), generator=g, device=dev) for _ in range(P)]
    dout = torch.rand((1, H, W, 3), generator=g, device=dev) * 2 - 1
    q = _lib._stream(dev)
    L = _lib.load()
    need = L.mpiv_over_composite_backward_workspace_size(P, npx)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    ptrs = torch.tensor([t.data_ptr() for t in layers], dtype=torch.int64).to(dev)
    out = torch.empty((1, H, W, 3), device=dev)
    dlayers = torch.empty((P, 1, H, W, 4), device=dev)
    dst = (_lib.ctypes.c_int64 * 2)(3, 1)

    def fwd():
        _lib._call("mpiv_over_composite", ptrs, P, npx, 4, 1, out, q)

    def bwd():
        _lib._call("mpiv_over_composite_backward", ptrs, P, npx, 4, 1, dout, dst, dlayers, ws, ws.numel(), q)

    def ours():
        fwd()
        bwd()

    leaves = [t.clone().requires_grad_() for t in layers]

    def torch_fb():
        for i, t in enumerate(leaves):
            rgb, alpha = t[..., 0:3], t[..., 3:]
            o = rgb if i == 0 else rgb * alpha + o * (1.0 - alpha)  # noqa: F821
        return torch.autograd.grad(o, leaves, dout)

    bwd()
    same = all(bool(torch.equal(a, b)) for a, b in zip(torch_fb(), dlayers)) if P <= 32 else None
    for fn in (bwd, ours, torch_fb):
        warm(fn, stream, min_ms=60)
    tb, to, tt = [], [], []
    for _ in range(reps):
        tb.append(span_ms(bwd, n, stream))
        to.append(span_ms(ours, n, stream))
        tt.append(span_ms(torch_fb, max(n // 4, 3), stream))
    nbytes = 3 * P * npx * 16 + 2 * need
    return {"what": "compositor", "shape": [H, W, P], "equals_torch_device_autograd": same,
            "backward_ms": med(tb), "backward_reps": [round(x, 4) for x in tb], "forward_backward_ms": med(to),
            "torch_autograd_fwd_bwd_ms": med(tt), "torch_reps": [round(x, 4) for x in tt],
            "speedup_vs_torch": round(med(tt) / med(to), 2), "algorithmic_bytes": nbytes, "workspace_bytes": need,
            "backward_gbs": round(nbytes / (med(tb) * 1e-3) / 1e9, 1),
            "backward_share_of_hbm_peak": round(nbytes / (med(tb) * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    tail = {"build_id": _lib.load().mpiv_build_id().decode(), "device": torch.cuda.get_device_name(dev),
            "method": f"median of {a.reps} spans of {a.n} back-to-back launches after >= 60 ms of warm-up launches, "
                      "HIP events; sampler entries alternated old, new, old"}
    lines = [json.dumps({**sampler(*s, dev, stream, a.reps, a.n), **tail}) for s in SAMPLER_SHAPES]
    lines += [json.dumps({**compositor(*s, dev, stream, a.reps, a.n), **tail}) for s in OVER_SHAPES]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
