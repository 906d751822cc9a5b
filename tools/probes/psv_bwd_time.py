#!/usr/bin/env python3
"""Device time of the plane sweep's adjoint (psv_bwd.hip, mpiv_plane_sweep_backward): d img only, the
cameras only (dki + dproj), and everything (d img, ddepths, dki, dproj), beside the route there was before
it -- D calls of mpiv_inverse_warp_backward on constant depth maps (stride-0 views of the depth list, no
copies) and dout's channel slices, plus the D - 1 adds of the per-depth results -- and, for scale, torch's
own grid_sample autograd over one leaf on the device (float atomics, no fixed order).
warp_bwd_time.py's method: the calls launched back to back on preallocated inputs after at least 60 ms of
warm-up launches, HIP events on the launch stream, the median of the spans; every span is recorded, so the
run-to-run spread of each variant can be read beside its median.

    python tools/probes/psv_bwd_time.py [--out profiles/psv_bwd.jsonl] [--reps 5]

One JSON line per shape: the notebook's (B = 4, 224x224x3, D = 10) and one config-3 source (1024x768x3,
D = 64)."""
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
from mpi_vision_amd.utils import inv_depths  # noqa: E402

SHAPES = [(4, 224, 224, 3, 10, 20), (1, 768, 1024, 3, 64, 5)]  # B, H, W, C, D, launches per span


def measure(B, H, W, C, D, n, dev, stream, reps):
    g = torch.Generator(device=dev).manual_seed(9)
    img = torch.rand((B, H, W, C), generator=g, device=dev)
    depths = torch.tensor(inv_depths(1.0, 100.0, D), dtype=torch.float32, device=dev)
    dout = torch.rand((B, H, W, D * C), generator=g, device=dev) * 2 - 1
    K = configs.f32([configs.intrinsics_matrix(0.9 * W, 0.9 * W, W / 2.0, H / 2.0)] * B)
    pose = configs.f32([configs.pose_from(configs.rot_y(2.0), (0.05, -0.02, 0.03))] * B)
    ki, proj = (t.to(dev) for t in _host.psv_matrices(K, K, pose))
    vol = _lib.plane_sweep(img, depths, ki, proj, H, W)
    live = float((vol.reshape(B, H, W, D, C).abs().sum(-1) != 0).float().mean())
    del vol
    L = _lib.load()
    q = _lib._stream(dev)
    full = L.mpiv_plane_sweep_backward_workspace_size(B, H, W, C, H, W, D)
    least = L.mpiv_plane_sweep_backward_workspace_size_min(B, H, W, C, H, W, D)
    ws = torch.empty(full, dtype=torch.uint8, device=dev)
    ws8 = ws[:least + 7 * ((full - least) // max(D - 1, 1)) + 4096]  # room for groups of 8 planes
    o = {k: torch.empty(s, device=dev) for k, s in (("dimg", (B, H, W, C)), ("ddepths", (D,)), ("dki", (B, 9)),
                                                    ("dproj", (B, 16)))}
    si, so = _lib._strides(img), _lib._strides(dout)

    def psv(names, w=ws):
        ptr = [o[k] if k in names else None for k in ("dimg", "ddepths", "dki", "dproj")]
        return lambda: _lib._call("mpiv_plane_sweep_backward", img, si, B, H, W, C, ki, proj, depths, D, H, W, dout, so,
                                  *ptr, w, w.numel(), q)

    # the route before: one inverse-warp adjoint per depth, the results added in descending d
    wws = torch.empty(L.mpiv_inverse_warp_backward_workspace_size(B, H, W, C, H, W), dtype=torch.uint8, device=dev)
    maps = [depths[d].expand(B, H, W) for d in range(D)]
    slices = [dout[..., d * C:(d + 1) * C] for d in range(D)]
    sm, ss = _lib._strides(maps[0]), _lib._strides(slices[0])
    acc = {k: torch.empty_like(o[k]) for k in ("dimg", "dki", "dproj")}
    tmp = {k: torch.empty_like(o[k]) for k in ("dimg", "dki", "dproj")}
    dd_maps = torch.empty((B, H, W), device=dev)
    dd_acc = torch.empty((D,), device=dev)

    def loop(names):
        def run():
            for d in range(D - 1, -1, -1):
                dst = acc if d == D - 1 else tmp
                ptr = [dd_maps if "ddepths" in names else None] + [dst[k] if k in names else None for k in ("dimg", "dki", "dproj")]
                _lib._call("mpiv_inverse_warp_backward", img, si, B, H, W, C, ki, proj, maps[d], sm, H, W, slices[d], ss,
                           *ptr, wws, wws.numel(), q)
                if "ddepths" in names:
                    torch.sum(dd_maps, dim=(0, 1, 2), out=dd_acc[d])
                if d != D - 1:
                    for k in ("dimg", "dki", "dproj"):
                        if k in names:
                            acc[k].add_(tmp[k])
        return run

    # torch's own sampler over one leaf at the same coordinates
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, device=dev)], 0).expand(B, 3, H * W).contiguous()
    grids = []
    for d in range(D):
        cam = torch.empty((B, 4, H, W), device=dev)
        _lib._call("mpiv_pixel2cam", maps[d].contiguous(), pc, ki, B, H * W, 1, cam, q)
        grids.append(-1 + 2 * (_lib.cam2pixel(cam, proj) + 0.5) / torch.tensor([float(H), float(W)], device=dev))
    del pc
    leaf = img.permute(0, 3, 1, 2).contiguous().requires_grad_()
    dnchw = dout.permute(0, 3, 1, 2).contiguous()

    def torch_fb():
        r = torch.cat([F.grid_sample(leaf, gr, align_corners=False) for gr in grids], 1)
        torch.autograd.grad(r, leaf, dnchw)

    every = ("dimg", "ddepths", "dki", "dproj")
    res = {}
    for name, fn in (("psv_dimg_ms", psv(("dimg",))), ("psv_cam_ms", psv(("dki", "dproj"))), ("psv_all_ms", psv(every)),
                     ("psv_all_groups_of_8_ms", psv(every, ws8)),
                     ("loop_dimg_ms", loop(("dimg",))), ("loop_cam_ms", loop(("dki", "dproj"))), ("loop_all_ms", loop(every)),
                     ("torch_grid_sample_fwd_bwd_ms", torch_fb)):
        warm(fn, stream, min_ms=60)
        r = [span_ms(fn, n, stream) for _ in range(reps)]
        res[name] = round(float(np.median(r)), 4)
        res[name + "_reps"] = [round(x, 4) for x in r]
    return {"shape": [B, H, W, C], "D": D, "live_samples": round(live, 3), "workspace_bytes": full,
            "workspace_bytes_min": least, "workspace_bytes_groups_of_8": ws8.numel(), **res,
            "build_id": L.mpiv_build_id().decode(), "device": torch.cuda.get_device_name(dev),
            "method": f"median of {reps} spans of {n} back-to-back calls after >= 60 ms of warm-up calls, HIP events"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = []
    for s in SHAPES:
        lines.append(json.dumps(measure(*s, dev, stream, a.reps)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
