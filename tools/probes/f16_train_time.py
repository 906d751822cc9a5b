#!/usr/bin/env python3
"""Timing probe for training through a half MPI, config 4 (1024 x 1024 x 128), one view, forward plus
backward through autograd, in one process:

  (a) the half route: mpi_render_view_f16's Function (_lib.RenderF16Function) on the half leaf -- the
      tensor read in place at 8 B per texel, a half gradient;
  (b) the only route a half caller had before it: x16.float() -> _lib.RenderFunction -> autograd rounds
      the fp32 gradient to half (both casts included);
  (c) for scale, the float route on a float leaf (no casts).

Each figure is a span of back-to-back steps after a warm-up of at least 60 ms of the same steps (as
bench.warm does), three repetitions, and the peak of allocated bytes over one step above what is
allocated before it (the leaf, homographies and dout).  Also reports the kernels' own times from the raw
entries on a caller's workspace (forward with checkpoints, backward with them) for half and float, and
whether (a)'s gradient is (b)'s bit for bit.

Usage:
    timeout -k 10 300 python tools/probes/f16_train_time.py
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
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=None, metavar=("H", "W", "P"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    c = configs.config4()
    H, W, P = args.shape or (c["H"], c["W"], c["P"])
    f = configs.focal_from_fov(W)
    K = configs.f32([c["K"]]) if not args.shape else configs.f32([configs.intrinsics_matrix(f, f, W / 2.0, H / 2.0)])
    depths = configs.f32(c["depths"]) if not args.shape else configs.f32(configs.inv_depths(1, 100, P))
    g = torch.Generator(device=dev).manual_seed(0)
    x16 = torch.rand((1, H, W, P, 4), generator=g, device=dev).half()
    homs = _host.render_homographies(configs.f32(c["poses"][100:101]), depths, K, 1).to(dev)
    dout = torch.rand((1, H, W, 3), generator=g, device=dev) * 2 - 1
    leaf16 = x16.clone().requires_grad_(True)

    def step_half():
        leaf16.grad = None
        _lib.RenderF16Function.apply(leaf16, homs).backward(dout)

    def step_cast():
        leaf16.grad = None
        _lib.RenderFunction.apply(leaf16.float(), homs).backward(dout)

    step_half()
    ga = leaf16.grad.clone()
    step_cast()
    same = torch.equal(ga.view(torch.int16), leaf16.grad.view(torch.int16))
    del ga
    head = {"shape": [H, W, P], "build_id": _lib.load().mpiv_build_id().decode(), "grad_same_bits": same,
            "a_half_peak_bytes": peak_extra(step_half), "b_cast_peak_bytes": peak_extra(step_cast)}
    print(json.dumps(head), flush=True)
    for rep in range(3):
        row = {"rep": rep}
        for name, fn in (("a_half_step_ms", step_half), ("b_cast_step_ms", step_cast)):
            warm(fn)
            row[name] = round(span_ms(fn, args.iters), 4)
        print(json.dumps(row), flush=True)
    leaf16.grad = None
    # (c) and the kernels alone: raw entries, caller's workspace, checkpoints from the forward
    L = _lib.load()
    ws = torch.empty(L.mpiv_render_backward_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    for name, src in (("half", x16), ("float", None)):
        if src is None:
            del leaf16, x16
            torch.cuda.empty_cache()
            src = torch.rand((1, H, W, P, 4), generator=g, device=dev)
        _, ck = _lib.render_train(src, homs)
        legs = {f"{name}_forward_ms": lambda: _lib.render_train(src, homs),
                f"{name}_backward_ms": lambda: _lib.render_backward(src, homs, dout, workspace=ws, ckpt=ck)}
        for rep in range(3):
            row = {"rep": rep}
            for leg, fn in legs.items():
                warm(fn)
                row[leg] = round(span_ms(fn, args.iters), 4)
            print(json.dumps(row), flush=True)
        del ck, src


if __name__ == "__main__":
    main()
