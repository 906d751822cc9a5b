#!/usr/bin/env python3
"""Timing probe for the camera gradient of the render backward (render_bwd_cam.hip), one shape per
process: (a) the backward with dhoms, (b) the fixed-MPI backward (dhoms only: no gather, check or
fallback) and (c) the plain backward, all with the forward's checkpoints and the caller's workspace,
measured in the same run.  Each figure is a span of back-to-back launches after a warm-up of at
least 60 ms of the same launches (as bench.warm does), three repetitions.  Also prints whether dhoms
of (a) and (b) are the same bits.

Usage (each shape under its own time limit; a 16-CPU budget is plenty, the probe is one thread):
    timeout -k 10 300 python tools/probes/camgrad_time.py --shape config4
    timeout -k 10 120 python tools/probes/camgrad_time.py --shape notebook
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mpi_vision_amd import _host, _lib, configs  # noqa: E402


def span_ms(fn, n):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(n):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / n


def warm(fn, seconds=0.06):
    t0 = time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["config4", "notebook"], default="config4")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    c = configs.config4()
    if args.shape == "config4":
        H, W, P = c["H"], c["W"], c["P"]
        K, depths = configs.f32([c["K"]]), configs.f32(c["depths"])
    else:  # the notebook's training shape: 224 x 224, 10 planes
        H, W, P = 224, 224, 10
        f = configs.focal_from_fov(W)
        K, depths = configs.f32([configs.intrinsics_matrix(f, f, W / 2.0, H / 2.0)]), configs.f32(configs.inv_depths(1, 100, P))
    g = torch.Generator(device=dev).manual_seed(0)
    mpi = torch.rand((1, H, W, P, 4), generator=g, device=dev)
    homs = _host.render_homographies(configs.f32(c["poses"][100:101]), depths, K, 1).to(dev)
    dout = torch.rand((1, H, W, 3), generator=g, device=dev) * 2 - 1
    L = _lib.load()
    ws = torch.empty(L.mpiv_render_backward_cam_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    _, ck = _lib.render_train(mpi, homs)
    legs = {
        "a_backward_with_dhoms_ms": lambda: _lib.render_backward(mpi, homs, dout, workspace=ws, ckpt=ck, want_dhoms=True),
        "b_fixed_mpi_dhoms_only_ms": lambda: _lib.render_backward(mpi, homs, dout, workspace=ws, ckpt=ck,
                                                                  want_dhoms=True, want_dmpi=False),
        "c_plain_backward_ms": lambda: _lib.render_backward(mpi, homs, dout, workspace=ws, ckpt=ck),
    }
    same = torch.equal(legs["a_backward_with_dhoms_ms"]()[1].view(torch.int32),
                       legs["b_fixed_mpi_dhoms_only_ms"]()[1].view(torch.int32))
    for rep in range(3):
        row = {"shape": [H, W, P], "rep": rep, "dhoms_same_bits": same}
        for name, fn in legs.items():
            warm(fn)
            row[name] = round(span_ms(fn, args.iters), 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
