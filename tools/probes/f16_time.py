#!/usr/bin/env python3
"""Timing probe for the half-precision texel render beside the fp32 and u8 renders of the same
synthetic MPI (MPIV_LIB selects a probe build of the library).

Legs: the config-4 shape (1024x1024x128) at 1 view and at 125 views per launch, the config-2 shape
(576x1024x32) at 64 views (--legs c4_v<N>,c2_v<N>,... times other view counts; --unpack also times
the f16 -> float copy, mpiv_unpack_planes_f16; --tag labels the lines of a probe build).  Formats:
render_packed_f16 (the f16 kernel) on the fp32 synthetic MPI rounded to half, fp32 render_packed on that half MPI's exact float copy (so the frames must be identical, which is
checked), and the u8 kernel (route_float=False) on the same MPI quantised to bytes.  Method
(bench.py's): at least 60 ms of untimed back-to-back launches, then the mean of event-timed
back-to-back launches; three repeats, all printed.  One JSON line per leg, appended to --out."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from bench import event_ms, warm  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402

REPEATS = 3


def to_u8_packed(pf: torch.Tensor) -> torch.Tensor:
    """packed fp32 (rgb in [-1, 1), alpha in [0, 1]) -> packed u8 words, zero border."""
    b = torch.empty(pf.shape, dtype=torch.uint8, device=pf.device)
    for p in range(pf.shape[0]):  # plane by plane: the temporaries stay small
        q = pf[p].clone()
        q[..., :3].mul_(0.5).add_(0.5)
        b[p] = q.clamp_(0, 1).mul_(255).round_().to(torch.uint8)
    b[:, :2] = 0
    b[:, -2:] = 0
    b[:, :, :2] = 0
    b[:, :, -2:] = 0
    return b.view(torch.int32).squeeze(-1)


def leg(name, c, first, V, n, formats, dev, stream, unpack=False):
    H, W, P = c["H"], c["W"], c["P"]
    homs = _host.render_homographies(configs.f32(c["poses"][first:first + V]), configs.f32(c["depths"]),
                                     configs.f32([c["K"]] * V), V).reshape(V, P, 9).to(dev)
    pf = _lib.synth_mpi_packed(c["seed"], H, W, 0, P, dev)
    pk16 = pf.half()  # elementwise on the packed layout: the packed f16 MPI (the border stays +0)
    pk8 = to_u8_packed(pf) if "u8" in formats else None
    del pf
    fcopy = _lib.unpack_planes_f16(pk16) if "f32" in formats else None
    out = torch.empty((V, H, W, 3), device=dev)
    s = _lib._stream(dev)
    fns = {"f16": lambda: _lib._call("mpiv_render_packed_f16", pk16, H, W, P, homs, V, out, s),
           "f32": lambda: _lib._call("mpiv_render_packed", fcopy, H, W, P, homs, V, out, s),
           "u8": lambda: _lib._call("mpiv_render_packed_u8", pk8, H, W, P, homs, V, out, s)}
    res = {"leg": name, "H": H, "W": W, "P": P, "V": V, "launches_per_repeat": n,
           "lib": os.path.basename(os.environ.get("MPIV_LIB", "libmpiv.so")),
           "mpi_bytes": {"f16": pk16.numel() * 2, "f32": pk16.numel() * 4, "u8": pk16.numel()}}
    if unpack:  # the cost of the float route's copy, once per MPI
        fdst = fcopy if fcopy is not None else torch.empty(pk16.shape, dtype=torch.float32, device=dev)
        up = lambda: _lib._call("mpiv_unpack_planes_f16", pk16, H, W, P, fdst, s)  # noqa: E731
        res["unpack_f16_ms"] = []
        for _ in range(REPEATS):
            warm(up, stream)
            res["unpack_f16_ms"].append(round(event_ms(up, 20, stream), 4))
    frames = {}
    for f in formats:
        reps = []
        for _ in range(REPEATS):
            warm(fns[f], stream)
            reps.append(round(event_ms(fns[f], n, stream), 4))
            print(json.dumps({"leg": name, "format": f, "ms": reps[-1]}), flush=True)
        res[f + "_ms"] = reps
        res[f + "_route"] = _lib.route({"f16": "render_packed_f16", "f32": "render_packed",
                                        "u8": "render_packed_u8"}[f], H, W, P, V)[0]
        if f in ("f16", "f32"):
            frames[f] = out.clone()
    if len(frames) == 2:
        res["f16_equals_f32_bits"] = bool(torch.equal(frames["f16"].view(torch.int32), frames["f32"].view(torch.int32)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "f16_render.jsonl"))
    ap.add_argument("--formats", default="f16,f32,u8")
    ap.add_argument("--legs", default="c4_v1,c4_v125,c2_v64")
    ap.add_argument("--unpack", action="store_true")
    ap.add_argument("--tag", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    formats = args.formats.split(",")
    c4, c2 = configs.config4(), configs.config2()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    for name in args.legs.split(","):  # c4_v<N> / c2_v<N>: N views per launch (the crossover: --legs c4_v8,c4_v16,...)
        cfg, _, nv = name.partition("_v")
        c, V = {"c4": c4, "c2": c2}[cfg], int(nv)
        first = 7 if V == 1 else 0
        n = 20 if V * c["H"] * c["W"] * c["P"] < (1 << 32) else 4  # launches per repeat: 4 for multi-ms launches
        res = leg(name, c, first, V, n, formats, dev, stream, args.unpack)
        if args.tag:
            res["tag"] = args.tag
        torch.cuda.empty_cache()
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
