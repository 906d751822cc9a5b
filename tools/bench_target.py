#!/usr/bin/env python3
"""Time the fused render into a target camera of its own size (mpiv_render_packed_tgt and its u8 twin)
beside the only other route to the same frame: the unfused helper chain, warp_planes (the reference's
transform_plane_imgs_torch: P warped [V,4,Ht,Wt] planes and their sampling grids) + over_composite.

Case A: config 4's 1024 x 1024 x 128 float MPI (synthetic) into 2048 x 2048 (2x supersampling), 512 x 512
        (a preview) and a 256 x 256 crop window of the full-size frame, at 1, 8 and 64 views.
Case B: a 400 x 640 x 10 u8 MPI (the test MPI's shape, synthetic bytes) into 1080 x 1920 at 1 and 16
        views; the chain runs on u8.float() / 255.
--shape Hs,Ws,P scales case A down for a rehearsal.

Both intrinsics are expressed at the target's resolution (mpi_render_view_torch2's docstring): k_s is
the MPI's camera scaled to the target's size, k_t the target camera; for the crop k_t is the full-size
camera with its principal point shifted by the window's origin and k_s the MPI's camera scaled to the
window's size.

Method (bench.py's): untimed back-to-back launches first, then the mean of event-timed back-to-back
launches; REPEATS repeats, the two routes alternating; every repeat is reported and the medians
compared.  The chain is given device-resident homographies and a device-resident target grid (the
meshgrid is built and uploaded once, outside the timed calls), so a timed call is the helpers' device
work -- the per-plane copy of the grid, the point transform, the sampler, the compositor -- plus
over_composite's per-call table of P layer pointers, which the helper builds on the host and uploads
(P * 8 bytes).  It is skipped, with a note, where its tensors do not fit the device's free memory.  The
frames of the two routes must be bit-identical: the tool exits non-zero if they are not.  `bytes` is
what each route's tensors hold -- every byte is written and read at least once: the fused route the
packed MPI and the frame, the chain also the target points, the sampling grids and the warped planes
(and a per-view copy of the MPI where one MPI serves several views).  One JSON line is appended to
--out (profiles/target.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import event_ms, warm  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from mpi_vision_amd import utils as mvu  # noqa: E402

REPEATS = 3


def scaled(K, sy, sx):
    return [[K[0][0] * sx, 0.0, K[0][2] * sx], [0.0, K[1][1] * sy, K[1][2] * sy], [0.0, 0.0, 1.0]]


def target_grid(V, size, dev):
    """pixel_coords_trg [V,Ht,Wt,3] on the device (built on the host and uploaded: once per case)."""
    return mvu.meshgrid_abs_torch(V, *size).permute(0, 2, 3, 1).to(dev)


def chain(view, homs, size, grid):
    """view [Hs,Ws,P,4] float on the device, homs [V,P,9], grid [V,Ht,Wt,3] -> [V,Ht,Wt,3]."""
    V, P = homs.shape[:2]
    Hs, Ws = view.shape[:2]
    grid = grid[None].expand(P, V, *size, 3)
    hom = homs.reshape(V, P, 3, 3).permute(1, 0, 2, 3).contiguous()
    w = _lib.warp_planes(view.permute(2, 0, 1, 3)[:, None].expand(P, V, Hs, Ws, 4), grid, hom).permute(0, 1, 3, 4, 2)
    return _lib.over_composite([w[i] for i in range(P)])


def measure(tag, fused, view_float, packed_bytes, homs, size, dev, stream, skip_chain=False):
    V, P = homs.shape[:2]
    Hs, Ws = view_float.shape[:2]
    Ht, Wt = size
    frame = V * Ht * Wt * 12
    chain_bytes = P * V * Ht * Wt * (12 + 8 + 16) + (P * V * Hs * Ws * 16 if V > 1 else P * Hs * Ws * 16) + frame
    res = {"case": tag, "src": [Hs, Ws, P], "tgt": [Ht, Wt], "views": V,
           "bytes": {"fused": packed_bytes + frame, "chain": chain_bytes}}
    n_f = 20 if V * Ht * Wt <= (1 << 23) else 5
    ms = {"fused": [], "chain": []}
    fits = not skip_chain and chain_bytes * 1.25 < torch.cuda.mem_get_info(dev)[0]
    fns = {"fused": (fused, n_f)}
    if fits:
        grid = target_grid(V, size, dev)
        fns["chain"] = (lambda: chain(view_float, homs, size, grid), 3)
    else:
        res["chain_note"] = "the chain's tensors do not fit the device's free memory: not timed"
    frames = {}
    for _ in range(REPEATS):
        for f, (fn, n) in fns.items():
            if f == "fused":
                warm(fn, stream)
            else:
                fn()
            ms[f].append(round(event_ms(fn, n, stream), 4))
            if f not in frames:
                frames[f] = fn().clone()
            print(json.dumps({"case": tag, "tgt": [Ht, Wt], "views": V, "route": f, "ms": ms[f][-1]}), flush=True)
            torch.cuda.empty_cache()
    res["fused_ms"], res["fused_median_ms"] = ms["fused"], statistics.median(ms["fused"])
    ok = True
    if fits:
        res["chain_ms"], res["chain_median_ms"] = ms["chain"], statistics.median(ms["chain"])
        res["chain_over_fused"] = round(res["chain_median_ms"] / res["fused_median_ms"], 2)
        ok = bool(torch.equal(frames["fused"].view(torch.int32), frames["chain"].view(torch.int32)))
        res["frames_bit_identical"] = ok
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "target.jsonl"))
    ap.add_argument("--shape", default=None, help="Hs,Ws,P instead of config 4's (rehearsals)")
    ap.add_argument("--views", default="1,8,64")
    ap.add_argument("--cases", default="A,B")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_target: needs a ROCm device (there is no CPU path)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = _lib._stream(dev)
    results, all_ok = [], True

    if "A" in args.cases.split(","):
        c = configs.config4()
        Hs, Ws, P = (int(x) for x in args.shape.split(",")) if args.shape else (c["H"], c["W"], c["P"])
        K = scaled(c["K"], Hs / c["H"], Ws / c["W"])
        depths = configs.f32(c["depths"] if P == c["P"] else configs.inv_depths(1, 100, P))
        packed = _lib.synth_mpi_packed(c["seed"], Hs, Ws, 0, P, dev)
        view = _lib.unpack_planes(packed)  # the chain's [Hs,Ws,P,4] view of the same texels
        q = Hs // 4
        targets = [("2x", (2 * Hs, 2 * Ws), scaled(K, 2, 2), scaled(K, 2, 2)),
                   ("half", (Hs // 2, Ws // 2), scaled(K, 0.5, 0.5), scaled(K, 0.5, 0.5)),
                   ("crop", (q, q), scaled(K, q / Hs, q / Ws),
                    [[K[0][0], 0.0, K[0][2] - (Ws - q) / 2], [0.0, K[1][1], K[1][2] - (Hs - q) / 2], [0.0, 0.0, 1.0]])]
        for V in (int(v) for v in args.views.split(",")):
            first = 7 if V == 1 else 0
            for tag, size, ks, kt in targets:
                homs = _host.render_homographies(configs.f32(c["poses"][first:first + V]), depths, configs.f32([ks] * V), V,
                                                 tgt_intrinsics=configs.f32([kt] * V)).reshape(V, P, 9).to(dev)
                out = torch.empty((V,) + size + (3,), device=dev)

                def fused(out=out, homs=homs, size=size, V=V):
                    _lib._call("mpiv_render_packed_tgt", packed, Hs, Ws, P, homs, V, size[0], size[1], out, s)
                    return out
                r, ok = measure(f"A/{tag}", fused, view, packed.numel() * 4, homs, size, dev, stream)
                r["route"] = _lib.route("render_packed_tgt", Hs, Ws, P, V, *size)[0]
                results.append(r)
                all_ok = all_ok and ok
                del out
                torch.cuda.empty_cache()
        del packed, view
        torch.cuda.empty_cache()

    if "B" in args.cases.split(","):
        c1 = configs.config1_camera()
        Hs, Ws, P = c1["H"], c1["W"], c1["P"]
        size = (1080, 1920)
        g = torch.Generator().manual_seed(1)
        u8 = torch.randint(0, 256, (Hs, Ws, P, 4), generator=g, dtype=torch.uint8)
        u8[..., 0, 3] = 255
        view = (u8.float() / 255).to(dev)  # (the IEEE division, on the host: what the u8 kernel reproduces)
        u8 = u8.to(dev)
        packed = _lib.pack_planes_u8(u8)
        K = scaled(c1["K"], size[0] / Hs, size[1] / Ws)
        depths = configs.f32(c1["depths"])
        path = configs.sway_path(64)
        for V in (1, 16):
            homs = _host.render_homographies(configs.f32(path[:V]), depths, configs.f32([K] * V), V).reshape(V, P, 9).to(dev)
            out = torch.empty((V,) + size + (3,), device=dev)

            def fused(out=out, homs=homs, V=V):
                _lib._call("mpiv_render_packed_u8_tgt", packed, Hs, Ws, P, homs, V, size[0], size[1], out, s)
                return out
            r, ok = measure("B/u8", fused, view, packed.numel() * 4, homs, size, dev, stream)
            r["route"] = _lib.route("render_packed_u8_tgt", Hs, Ws, P, V, *size)[0]
            results.append(r)
            all_ok = all_ok and ok
            del out
            torch.cuda.empty_cache()

    res = {"results": results, "fused_faster_everywhere": all(r.get("chain_over_fused", 2.0) > 1.0 for r in results)}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)
    if not all_ok:
        sys.exit("bench_target: the fused and the chain's frames differ")


if __name__ == "__main__":
    main()
