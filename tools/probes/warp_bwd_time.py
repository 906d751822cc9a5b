#!/usr/bin/env python3
"""Device time of the depth-map inverse warp and its adjoint (warp_bwd.hip): the forward, the backward
with only d depth, with d depth + dki + dproj, and with everything, and beside them torch's own
grid_sample forward + backward on the device at the same coordinates (what a user had before: float
atomics, no fixed order).  bench.py's method: the entry points launched back to back on preallocated
inputs after at least 60 ms of warm-up launches, HIP events on the launch stream.

    python tools/probes/warp_bwd_time.py [--out profiles/warp_bwd.jsonl] [--reps 5] [--n 20]

One JSON line per shape (224x224x3 at B = 4, the notebook's; 1024x1024x3 at B = 1)."""
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

SHAPES = [(4, 224, 224, 3), (1, 1024, 1024, 3)]


def measure(B, H, W, C, dev, stream, reps, n):
    g = torch.Generator(device=dev).manual_seed(9)
    img = torch.rand((B, H, W, C), generator=g, device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    depth = (1.0 + xx / W + 0.5 * yy / H).expand(B, H, W) + torch.rand((B, H, W), generator=g, device=dev)
    dout = torch.rand((B, H, W, C), generator=g, device=dev) * 2 - 1
    K = configs.f32([configs.intrinsics_matrix(0.9 * W, 0.9 * W, W / 2.0, H / 2.0)] * B)
    pose = configs.f32([configs.pose_from(configs.rot_y(2.0), (0.05, -0.02, 0.03))] * B)
    ki, proj = (t.to(dev) for t in _host.psv_matrices(K, K, pose))
    out = _lib.inverse_warp_depthmap(img, depth, ki, proj, H, W)
    live = float((out.abs().sum(-1) != 0).float().mean())
    L = _lib.load()
    ws = torch.empty(L.mpiv_inverse_warp_backward_workspace_size(B, H, W, C, H, W), dtype=torch.uint8, device=dev)
    o = {k: torch.empty(s, device=dev) for k, s in (("ddepth", (B, H, W)), ("dimg", (B, H, W, C)), ("dki", (B, 9)),
                                                    ("dproj", (B, 16)))}
    q = _lib._stream(dev)
    si, sd, so = _lib._strides(img), _lib._strides(depth), _lib._strides(dout)

    def bwd(*names):
        ptr = [o[k] if k in names else None for k in ("ddepth", "dimg", "dki", "dproj")]
        return lambda: _lib._call("mpiv_inverse_warp_backward", img, si, B, H, W, C, ki, proj, depth, sd, H, W, dout,
                                  so, *ptr, ws, ws.numel(), q)

    # torch's own sampler at the same coordinates (cam2pixel of the same matrices)
    pc = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, device=dev)], 0).expand(B, 3, H * W).contiguous()
    cam = torch.empty((B, 4, H, W), device=dev)
    _lib._call("mpiv_pixel2cam", depth.contiguous(), pc, ki, B, H * W, 1, cam, q)
    pix = _lib.cam2pixel(cam, proj)
    grid = (-1 + 2 * (pix + 0.5) / torch.tensor([float(H), float(W)], device=dev)).requires_grad_()
    leaf = img.permute(0, 3, 1, 2).contiguous().requires_grad_()
    dnchw = dout.permute(0, 3, 1, 2).contiguous()

    def torch_fb():
        r = F.grid_sample(leaf, grid, align_corners=False)
        torch.autograd.grad(r, (leaf, grid), dnchw)

    res = {}
    for name, fn in (("forward_ms", lambda: _lib._call("mpiv_inverse_warp", img, si, B, H, W, C, ki, proj, depth, sd, H,
                                                        W, out, q)),
                     ("backward_ddepth_ms", bwd("ddepth")),
                     ("backward_ddepth_cam_ms", bwd("ddepth", "dki", "dproj")),
                     ("backward_dimg_ms", bwd("dimg")),
                     ("backward_all_ms", bwd("ddepth", "dimg", "dki", "dproj")),
                     ("torch_grid_sample_fwd_bwd_ms", torch_fb)):
        warm(fn, stream, min_ms=60)
        r = [span_ms(fn, n, stream) for _ in range(reps)]
        res[name] = round(float(np.median(r)), 4)
        res[name + "_reps"] = [round(x, 4) for x in r]
    return {"shape": [B, H, W, C], "live_pixels": round(live, 3), "workspace_bytes": ws.numel(), **res,
            "build_id": L.mpiv_build_id().decode(), "device": torch.cuda.get_device_name(dev),
            "method": f"median of {reps} spans of {n} back-to-back launches after >= 60 ms of warm-up launches, "
                      "HIP events"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = [json.dumps(measure(*s, dev, stream, a.reps, max(a.n, 20))) for s in SHAPES]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
