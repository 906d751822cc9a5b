#!/usr/bin/env python3
"""Goldens for exact-lattice, huge / w == 0 / non-finite homographies and non-finite texels
(tests/lattice_cases.py): the REFERENCE utils.py run on CPU (imported as in gen_goldens.py) on crafted
3x3 matrices, through its own functions in its own call order -- transform_points_torch,
normalize_homogeneous_torch, the division by (H-1, W-1), bilinear_wrapper_torch (utils.py:176-195),
over_composite -- plus torch autograd with a seeded grad_output; plane_sweep_torch,
plane_sweep_torch_one2 and projective_inverse_warp_torch for the sweep; bilinear_wrapper_torch and
resampler_wrapper_torch on a boundary coordinate set.  Test tooling only.

Writes tests/golden/lattice.npz.  Inputs come from seeds (tests/lattice_cases.py), so the file holds
the matrices, the sha of every input and, per expected array, its NaN count, the sha of its bits
(NaNs canonicalised: a payload is not part of the contract) and 1024 sampled values -- the gradients
alone would be several MB in full.  The small sampler set is stored whole.

Usage:  python tools/gen_goldens_lattice.py"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from gen_goldens import load_reference, sha  # noqa: E402
import lattice_cases as lc  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "lattice.npz")
P = 4


def ref_planes(ref, mpi, homs):
    """The warped planes [P, B, H, W, 4] of mpi [B, H, W, P, 4] under homs [B, P, 9]
    (transform_plane_imgs_torch's body after inv_homography_torch, utils.py:178-192)."""
    B, H, W, Pn, _ = mpi.shape
    rgba = mpi.permute([3, 0, 1, 2, 4])
    pix = ref.meshgrid_abs_torch(B, H, W).permute([0, 2, 3, 1])
    pix = torch.unsqueeze(pix, 0).repeat([Pn, 1, 1, 1, 1])
    hm = homs.reshape(B, Pn, 3, 3).permute(1, 0, 2, 3).contiguous()
    pts = ref.transform_points_torch(pix, hm)
    pts = ref.normalize_homogeneous_torch(pts)
    pts = pts / torch.Tensor([H - 1, W - 1])
    return ref.bilinear_wrapper_torch(rgba, pts).permute([0, 1, 3, 4, 2])


def ref_render(ref, mpi, homs, p_end=None):
    s = ref_planes(ref, mpi, homs)
    return ref.over_composite([s[i] for i in range(s.shape[0] if p_end is None else p_end)])


def put(out, key, arr):
    a = np.ascontiguousarray(arr.detach().numpy() if isinstance(arr, torch.Tensor) else arr, np.float32)
    out[key + "_sha"] = np.array(lc.canon_sha(a))
    out[key + "_nan"] = np.array(int(np.isnan(a).sum()), np.int64)
    out[key + "_val"] = a.reshape(-1)[lc.sample_idx(a.size)]
    out[key + "_shape"] = np.array(a.shape, np.int64)


def render_cases(ref, out):
    for tag, shape in (("x", lc.X_SMALL), ("y", lc.Y_SMALL)):
        H, W = shape
        for kind in ("finite", "nonfinite"):
            tex = lc.texels(kind, H, W, P)
            out[f"{tag}_{kind}_mpi_sha"] = np.array(sha(tex))
            for fam in lc.FAMILIES + ["nonfinite_h"]:
                homs = lc.nonfinite_views(shape, P) if fam == "nonfinite_h" else lc.family(fam, shape)[None]
                homs = torch.from_numpy(np.ascontiguousarray(homs, np.float32))
                B = homs.shape[0]
                key = f"{tag}_{fam}_{kind}"
                out[f"{tag}_{fam}_H"] = homs.numpy()
                backward = kind == "finite" or fam in ("int_shift", "half_shift")
                leaf = tex[None].repeat(B, 1, 1, 1, 1).requires_grad_(backward)
                res = ref_render(ref, leaf, homs)
                put(out, key + "_out", res)
                with torch.no_grad():
                    put(out, key + "_back2", ref_render(ref, leaf, homs, p_end=2))
                if backward:
                    dout = lc.dout_for(res.shape)
                    out[f"{tag}_{fam}_dout_sha"] = np.array(sha(dout))
                    res.backward(dout)
                    put(out, key + "_grad", leaf.grad)


def sweep_cases(ref, out):
    K = torch.tensor(lc.SWEEP_K)
    poses = lc.sweep_poses()
    B = poses.shape[0]
    Hs, Ws = lc.SWEEP_SRC
    depths = lc.sweep_depths(9)
    out["sweep_depths"] = np.array(depths, np.float64)
    out["sweep_pose"] = poses.numpy()
    for kind in ("finite", "nonfinite"):
        for C in (3, 4):
            img = lc.image(B, Hs, Ws, C, kind)
            out[f"sweep_{kind}_c{C}_img_sha"] = np.array(sha(img))
            put(out, f"sweep_{kind}_c{C}_out", ref.plane_sweep_torch(img, depths, poses, K[None].repeat(B, 1, 1)))
        img = lc.image(B, Hs, Ws, 3, kind)
        Ht, Wt = lc.SWEEP_TGT[1]
        for b in (0, 2):
            put(out, f"sweep_{kind}_tgt{b}_out", ref.plane_sweep_torch_one2(img[b], depths, poses[b], K, K, Ht, Wt))
        dmap = lc.degenerate_depth_map(B, Hs, Ws)
        out["warp_depth_sha"] = np.array(sha(dmap))
        put(out, f"warp_{kind}_out", ref.projective_inverse_warp_torch(img, dmap, poses, K[None].repeat(B, 1, 1)))


def sampler_cases(ref, out):
    Hi, Wi, C = 8, 16, 3
    img = torch.cat([lc.image(1, Hi, Wi, C, "finite"), lc.image(1, Hi, Wi, C, "nonfinite")])
    coords = lc.boundary_coords(2, Hi, Wi)
    out["gs_img_sha"] = np.array(sha(img))
    out["gs_coords_sha"] = np.array(sha(coords))
    out["gs_bilinear"] = ref.bilinear_wrapper_torch(img, coords).numpy()
    out["gs_resampler"] = ref.resampler_wrapper_torch(img, coords).numpy()


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    out = {}
    render_cases(ref, out)
    sweep_cases(ref, out)
    sampler_cases(ref, out)
    # (a zip written entry by entry with a fixed date, so the file regenerates byte for byte)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
