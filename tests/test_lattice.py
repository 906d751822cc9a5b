"""CPU: the oracle against the reference on exact-lattice sample positions, huge / w == 0 / non-finite
homographies and non-finite texels (tests/golden/lattice.npz, written by tools/gen_goldens_lattice.py
from the reference's own functions on the crafted matrices of tests/lattice_cases.py), and the
conditions that keep tests/test_lattice_gpu.py from being vacuous -- evaluated on the oracle's output
and on the restated sample position, never on the kernels.

Contract for non-finite values: NaN positions follow the reference, payloads are not compared, every
other value is bit-identical (lattice_cases.match)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, sha256

import lattice_cases as lc
from mpi_vision_amd import _host  # noqa: E402
from oracle import oracle  # noqa: E402

P = 4
SMALL = {"x": lc.X_SMALL, "y": lc.Y_SMALL}
KINDS = ["finite", "nonfinite"]
ALL = lc.FAMILIES + ["nonfinite_h"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "lattice.npz"))


def check(gold, key, got):
    """got against the golden summary of one expected array: shape, NaN count, sampled values, sha."""
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape == tuple(gold[key + "_shape"]), f"{key}: shape {got.shape}"
    lc.match(got.reshape(-1)[lc.sample_idx(got.size)], gold[key + "_val"], f"{key} (sampled values)")
    assert int(np.isnan(got).sum()) == int(gold[key + "_nan"]), f"{key}: NaN count"
    assert lc.canon_sha(got) == str(gold[key + "_sha"]), f"{key}: bits differ outside the samples"


def _homs(fam, shape):
    return lc.nonfinite_views(shape, P) if fam == "nonfinite_h" else lc.family(fam, shape)[None]


def _mpi(kind, shape, B):
    tex = lc.texels(kind, shape[0], shape[1], P).numpy()
    return np.broadcast_to(tex[None], (B,) + tex.shape)


@pytest.mark.parametrize("fam", ALL)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", ["x", "y"])
def test_oracle_render_and_partial(tag, kind, fam, gold):
    shape = SMALL[tag]
    homs = _homs(fam, shape)
    lc.match(homs, gold[f"{tag}_{fam}_H"], "matrices")
    mpi = _mpi(kind, shape, homs.shape[0])
    assert sha256(np.ascontiguousarray(mpi[0])) == str(gold[f"{tag}_{kind}_mpi_sha"])
    check(gold, f"{tag}_{fam}_{kind}_out", oracle.render(mpi, homs))
    # the reference's composite of planes [0, 2) is the colour of the back partial [0, 2)
    check(gold, f"{tag}_{fam}_{kind}_back2", oracle.render_ct(mpi, homs, 0, 2, back=True)[..., :3])


@pytest.mark.parametrize("fam,kind", [(f, "finite") for f in ALL] + [("int_shift", "nonfinite"),
                                                                       ("half_shift", "nonfinite")])
@pytest.mark.parametrize("tag", ["x", "y"])
def test_oracle_render_backward(tag, fam, kind, gold):
    shape = SMALL[tag]
    homs = _homs(fam, shape)
    B = homs.shape[0]
    dout = lc.dout_for((B,) + shape + (3,))
    assert sha256(dout) == str(gold[f"{tag}_{fam}_dout_sha"])
    check(gold, f"{tag}_{fam}_{kind}_grad",
          oracle.render_backward(np.ascontiguousarray(_mpi(kind, shape, B)), homs, dout.numpy()))


def _sweep_mats(B):
    K = torch.tensor(lc.SWEEP_K)[None].repeat(B, 1, 1)
    return _host.psv_matrices(K, K, lc.sweep_poses()[:B])


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_plane_sweep_and_inverse_warp(kind, gold):
    poses = lc.sweep_poses()
    B = poses.shape[0]
    Hs, Ws = lc.SWEEP_SRC
    depths = lc.sweep_depths(9)
    assert np.array_equal(np.array(depths), gold["sweep_depths"]) and np.array_equal(poses.numpy(), gold["sweep_pose"])
    ki, proj = _sweep_mats(B)
    for C in (3, 4):
        img = lc.image(B, Hs, Ws, C, kind)
        assert sha256(img) == str(gold[f"sweep_{kind}_c{C}_img_sha"])
        check(gold, f"sweep_{kind}_c{C}_out", oracle.plane_sweep(img.numpy(), ki.numpy(), proj.numpy(), depths, Hs, Ws))
    img = lc.image(B, Hs, Ws, 3, kind).numpy()
    Ht, Wt = lc.SWEEP_TGT[1]
    for b in (0, 2):
        got = oracle.plane_sweep(img[b:b + 1], ki[b:b + 1].numpy(), proj[b:b + 1].numpy(), depths, Ht, Wt)
        check(gold, f"sweep_{kind}_tgt{b}_out", got)
    dmap = lc.degenerate_depth_map(B, Hs, Ws)
    assert sha256(dmap) == str(gold["warp_depth_sha"])
    check(gold, f"warp_{kind}_out", oracle.inverse_warp(img, ki.numpy(), proj.numpy(), dmap.numpy()))


def test_oracle_grid_sample_boundary_coordinates(gold):
    Hi, Wi, C = 8, 16, 3
    img = torch.cat([lc.image(1, Hi, Wi, C, "finite"), lc.image(1, Hi, Wi, C, "nonfinite")])
    coords = lc.boundary_coords(2, Hi, Wi)
    assert sha256(img) == str(gold["gs_img_sha"]) and sha256(coords) == str(gold["gs_coords_sha"])
    inp = img.numpy().transpose(0, 3, 1, 2)
    lc.match(oracle.grid_sample_nchw(inp, coords.numpy(), False), gold["gs_bilinear"], "bilinear_wrapper")
    lc.match(oracle.grid_sample_nchw(inp, coords.numpy(), True), gold["gs_resampler"], "resampler_wrapper")
    # the set is not vacuous: it holds NaN (Inf * 0 and NaN coordinates) and finite in-image values
    share = lc.nan_share(gold["gs_bilinear"])
    assert 0 < share < 0.5 and np.isfinite(gold["gs_bilinear"]).mean() > 0.3


# ---------------------------------------------------------------------------
# the conditions that keep the GPU tests from being vacuous
# ---------------------------------------------------------------------------

def _frac(a):
    return a - np.floor(a)


@pytest.mark.parametrize("shape", lc.RENDER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", lc.LATTICE + ["edge"])
def test_lattice_positions_are_exact(fam, shape):
    """Every pixel's position on the exact axis has a fraction of exactly 0 or exactly 0.5 (the one
    plane of `scale` with a step of 0.25: a multiple of 0.25), and each family reaches the values at
    which the clamps and the in-image tests switch."""
    n = lc.exact_extent(shape)
    seen = set()
    for i, h in enumerate(lc.family(fam, shape)):
        pos = lc.exact_axis_pos(h, shape)
        assert np.isfinite(pos).all()
        fr = _frac(pos)
        allowed = (0.0, 0.25, 0.5, 0.75) if (fam == "scale" and i == 3) else (0.0, 0.5)
        assert np.isin(fr, allowed).all(), f"{fam} plane {i}: fractions {np.unique(fr)[:8]}"
        seen.update(np.unique(pos).tolist())
    if fam == "int_shift":
        assert {-3.0, -2.0, -1.0, 0.0, n - 1.0, n + 0.0}.issubset(seen)
    if fam == "half_shift":
        assert {-1.5, -0.5, n - 0.5, n + 0.5}.issubset(seen)


@pytest.mark.parametrize("shape", [lc.X_TWO, lc.Y_TWO], ids=["129x128", "128x129"])
def test_edge_thresholds_are_hit_exactly(shape):
    """Plane k of `edge`: the first pixel of the second tile column (row) lies at exactly N-1, N,
    N+0.5, N+1; the last pixel of the first one at exactly -1, -2, -2.5, -3."""
    n = lc.exact_extent(shape)
    want = [n - 1, n, n + 0.5, n + 1, -1, -2, -2.5, -3]
    planes = lc.family("edge", shape)
    assert len(planes) == 8 * len(lc.edge_starts(shape))
    for k, h in enumerate(planes):
        b = lc.edge_starts(shape)[k // 8]
        pos = lc.exact_axis_pos(h, shape)
        line = pos[0, :] if lc.x_exact(shape) else pos[:, 0]
        at = line[b] if k % 8 < 4 else line[b - 1]
        assert at == np.float32(want[k % 8]), (lc.EDGE_THRESHOLDS[k % 8], at)
        assert np.all(np.diff(line) == 1)  # unit steps: [b] is the minimum of its tile, [b-1] the maximum


@pytest.mark.parametrize("tag", ["x", "y"])
def test_nan_shares(tag):
    """0 NaN for the lattice families and `huge` on finite texels; w_zero above 0 and below 10 %; the
    non-finite texel set under the lattice families above 0 and below 20 %; the backward under
    nonfinite_h above 0 and below 50 %.  Printed, then asserted."""
    shape = SMALL[tag]
    fin, bad = _mpi("finite", shape, 1), _mpi("nonfinite", shape, 1)
    for fam in lc.LATTICE + ["huge"]:
        homs = lc.family(fam, shape)[None]
        assert lc.nan_share(oracle.render(fin, homs)) == 0, fam
        assert lc.nan_share(oracle.render_backward(np.ascontiguousarray(fin), homs,
                                                   lc.dout_for((1,) + shape + (3,)).numpy())) == 0, fam
    s = lc.nan_share(oracle.render(fin, lc.family("w_zero", shape)[None]))
    print(f"w_zero: {100 * s:.2f} % NaN")
    assert 0 < s < 0.10
    for fam in lc.LATTICE:
        s = lc.nan_share(oracle.render(bad, lc.family(fam, shape)[None]))
        print(f"non-finite texels, {fam}: {100 * s:.2f} % NaN")
        assert 0 < s < 0.20, fam
    homs = lc.nonfinite_views(shape, P)
    B = homs.shape[0]
    s = lc.nan_share(oracle.render_backward(np.ascontiguousarray(_mpi("finite", shape, B)), homs,
                                            lc.dout_for((B,) + shape + (3,)).numpy()))
    print(f"backward under nonfinite_h: {100 * s:.2f} % NaN")
    assert 0 < s < 0.50
    out = oracle.render(_mpi("finite", shape, B), homs)
    for v in range(B):  # a view with a non-finite plane is NaN in every pixel; its neighbours hold none
        assert np.isnan(out[v]).all() == (v in lc.NONFINITE_BAD_VIEWS) and np.isnan(out[v]).any() == \
            (v in lc.NONFINITE_BAD_VIEWS), v
