#!/usr/bin/env python3
"""Training forward / backward of one non-broadcast view through the narrow and the wide in-place
readers (render_chunk.hip issue_taps_*_wide): config 4 (1024x1024x128, below 2 GiB) with chunk_wide=0
and chunk_wide=1, and 1024x1024x136 (2.28 GB: wide only).  bench.py's training-leg method: the entry
points launched back to back on preallocated outputs after a warm-up, HIP events on the launch stream.

    python tools/bench_wide.py [--out profiles/wide_views.jsonl] [--reps 5] [--n 10]

One JSON line per (shape, setting)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import span_ms, warm  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402


def measure(P, wide, dev, stream, reps, n):
    c4 = configs.config4()
    H, W = c4["H"], c4["W"]
    g = torch.Generator(device=dev).manual_seed(7)
    mpi = torch.rand((1, H, W, P, 4), generator=g, device=dev)
    homs = _host.render_homographies(configs.f32(c4["poses"][100:101]), configs.f32(configs.inv_depths(1, 100, P)),
                                     configs.f32([c4["K"]]), 1).to(dev)
    dout = torch.rand((1, H, W, 3), generator=g, device=dev) * 2 - 1
    with _lib.debug(chunk_wide=wide):
        L = _lib.load()
        ws = torch.empty(L.mpiv_render_backward_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
        grad = torch.empty((1, H, W, P, 4), device=dev)
        out = torch.empty((1, H, W, 3), device=dev)
        ck = torch.empty((1, (P + 7) // 8, H, W, 4), device=dev)
        st = _lib._strides(mpi)
        q = _lib._stream(dev)
        fwd = lambda: _lib._call("mpiv_render_train", mpi, st, 1, H, W, P, homs, out, ck, q)  # noqa: E731
        bwd = lambda: _lib._call("mpiv_render_backward", mpi, st, 1, H, W, P, homs, dout, ck, grad, ws,  # noqa: E731
                                 ws.numel(), q)
        bwd_nock = lambda: _lib._call("mpiv_render_backward", mpi, st, 1, H, W, P, homs, dout, None, grad,  # noqa: E731
                                      ws, ws.numel(), q)
        res = {}
        for name, fn in (("forward_ms", fwd), ("backward_ms", bwd), ("backward_no_ckpt_ms", bwd_nock)):
            warm(fn, stream)
            r = [span_ms(fn, n, stream) for _ in range(reps)]
            res[name] = round(float(np.median(r)), 4)
            res[name + "_reps"] = [round(x, 4) for x in r]
        aborted = _lib.render_backward_status(ws, H, W, P)
    span = (H - 1) * W * P * 16 + (W - 1) * P * 16 + 128
    return {"shape": [H, W, P], "view_bytes": H * W * P * 16, "chunk_wide": wide,
            "readers": "wide" if wide or span >= 0x7FFFFF00 else "narrow", "aborted_views": aborted, **res,
            "method": f"median of {reps} spans of {n} back-to-back launches after a warm-up, HIP events"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = []
    for P, wide in ((128, 0), (128, 1), (136, 0)):
        lines.append(json.dumps(measure(P, wide, dev, stream, a.reps, a.n)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
