#!/usr/bin/env python3
"""Time the alpha-only plane-colour render beside the float render of the same frame, at the
config-4 shape (1024 x 1024 x 128, synthetic alpha; --shape H,W,P for a rehearsal at another size).

In one process, at 1 view and at 125 views per launch:
  (a) mpiv_render_packed_alpha on the packed alpha planes (4 B per texel) and the [P,3] colours
      (1/d, d, 1);
  (b) the way to the same frame without it: mpiv_render_packed on the packed float MPI whose RGB is
      the plane's colour (16 B per texel);
and once (c): constructing that float MPI from the alpha with torch ops and packing it (what (b)
costs before its first launch), beside packing the alpha for (a).

Method (bench.py's): at least 60 ms of untimed back-to-back launches, then the mean of 20 event-timed
back-to-back launches; REPEATS repeats, (a) and (b) alternating; every repeat is reported, the
medians are compared.  The frames of (a) and (b) must be bit-identical: the tool exits non-zero if
they are not.  One JSON line is appended to --out (profiles/planecolor.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import event_ms, warm  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402

REPEATS = 3
LAUNCHES = 20


def timed_once(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    r = fn()
    b.record(stream)
    b.synchronize()
    return r, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "planecolor.jsonl"))
    ap.add_argument("--shape", default=None, help="H,W,P instead of config 4's (rehearsals)")
    ap.add_argument("--views", default="1,125")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_planecolor: needs a ROCm device (there is no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = _lib._stream(dev)
    c = configs.config4()
    H, W, P = (int(x) for x in args.shape.split(",")) if args.shape else (c["H"], c["W"], c["P"])
    depths = configs.f32(c["depths"] if P == c["P"] else configs.inv_depths(1, 100, P))
    colors = torch.stack([1.0 / depths, depths, torch.ones_like(depths)], -1).to(dev)

    # synthetic alpha: the synthetic MPI's alpha channel, as the [H,W,P,1] tensor a caller holds
    pf = _lib.synth_mpi_packed(c["seed"], H, W, 0, P, dev)
    alpha = _lib.unpack_planes(pf)[..., 3:].contiguous()
    del pf
    torch.cuda.empty_cache()

    # (c) once each, after one untimed run (allocations, code objects)
    def construct():
        return torch.cat([colors[None, None].expand(H, W, P, 3), alpha], -1)

    _lib.pack_planes(construct())
    _lib.pack_planes_alpha(alpha)
    torch.cuda.synchronize()
    mpi, construct_ms = timed_once(construct, stream)
    pk_f, pack_float_ms = timed_once(lambda: _lib.pack_planes(mpi), stream)
    del mpi
    pk_a, pack_alpha_ms = timed_once(lambda: _lib.pack_planes_alpha(alpha), stream)
    torch.cuda.empty_cache()

    res = {"H": H, "W": W, "P": P, "launches_per_repeat": LAUNCHES,
           "mpi_bytes": {"alpha": pk_a.numel() * 4, "float": pk_f.numel() * 4},
           "construct_ms": round(construct_ms, 4), "pack_float_ms": round(pack_float_ms, 4),
           "pack_alpha_ms": round(pack_alpha_ms, 4)}
    ok = True
    for V in (int(v) for v in args.views.split(",")):
        first = 7 if V == 1 else 0
        homs = _host.render_homographies(configs.f32(c["poses"][first:first + V]), depths,
                                         configs.f32([c["K"]] * V), V).reshape(V, P, 9).to(dev)
        out = torch.empty((V, H, W, 3), device=dev)
        fns = {"alpha": lambda: _lib._call("mpiv_render_packed_alpha", pk_a, H, W, P, colors, homs, V, out, s),
               "float": lambda: _lib._call("mpiv_render_packed", pk_f, H, W, P, homs, V, out, s)}
        ms = {"alpha": [], "float": []}
        frames = {}
        for _ in range(REPEATS):
            for f in ("alpha", "float"):
                warm(fns[f], stream)
                ms[f].append(round(event_ms(fns[f], LAUNCHES, stream), 4))
                frames[f] = out.clone() if f not in frames else frames[f]
                print(json.dumps({"views": V, "kernel": f, "ms": ms[f][-1]}), flush=True)
        same = bool(torch.equal(frames["alpha"].view(torch.int32), frames["float"].view(torch.int32)))
        med = {f: statistics.median(ms[f]) for f in ms}
        res[f"v{V}"] = {"alpha_ms": ms["alpha"], "float_ms": ms["float"], "alpha_median_ms": med["alpha"],
                        "float_median_ms": med["float"], "frames_bit_identical": same,
                        "alpha_route": _lib.route("render_packed_alpha", H, W, P, V)[0],
                        "float_route": _lib.route("render_packed", H, W, P, V)[0],
                        # (c): (b)'s first frame, construction and pack included
                        "float_with_construct_and_pack_ms": round(med["float"] + construct_ms + pack_float_ms, 4),
                        "alpha_with_pack_ms": round(med["alpha"] + pack_alpha_ms, 4)}
        ok = ok and same
        del out, frames
        torch.cuda.empty_cache()
    if "v1" in res:
        res["one_view_alpha_no_slower"] = res["v1"]["alpha_median_ms"] <= res["v1"]["float_median_ms"]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)
    if not ok:
        sys.exit("bench_planecolor: the alpha and float frames differ")


if __name__ == "__main__":
    main()
