"""CPU tests of the geometry fixture (tests/golden/geometry.npz, tools/gen_goldens_geometry.py) and of the
restatement the GPU tests compare with (tests/geometry_cases.py): the regenerated inputs are the
recorder's, the restatement equals every stored reference output with the chain ATen's rule selects, the
other chain does not (a fixture that could not tell the two apart would prove nothing), and the oracle
renders, warps and sweeps the smallest in-contract frame (5x9 = 45 pixels) bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, REPO

import geometry_cases as gc

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_goldens_geometry as gen  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "geometry.npz")))
    g["shas"] = json.loads(str(g["shas"]))
    return g


def ok(got, want, what):
    why = gc.same(got, want)
    assert why is None, f"{what}: {why}"


def host_agrees(mine, recorded) -> bool:
    """torch.inverse (LAPACK) returns host-dependent bits: a drop-in that inverts K on
    this host is held to the reference's golden only where this host's inverse has the recorded bits; the
    kernels fed the recorded bits are held to it everywhere."""
    mine = mine.detach().cpu().numpy() if isinstance(mine, torch.Tensor) else mine
    return gc.same(np.asarray(mine, np.float32).reshape(np.shape(recorded)), recorded) is None


def tp_want(gold, M, n, plain=None):
    """(reference output, restatement with the rule's chain or the given one) of a transform_points case."""
    pts, H = gen.tp_inputs(M, n)
    assert gen.sha(pts, H) == gold["shas"][f"tp_{M}_{n}"], "the regenerated inputs are not the golden's"
    rule = gc.tp_plain(n, M > 0)
    Hn = H.numpy()[..., None, :, :] if M else H.numpy()
    mine = gc.transform_points(pts.numpy(), Hn, rule if plain is None else plain)
    if n in gen.TP_DIGEST_ONLY:  # the reference's output is the restatement, held to the recorded digest
        assert gen.sha(gc.transform_points(pts.numpy(), Hn, rule)) == gold["shas"][f"tp_{M}_{n}_out"]
        return gc.transform_points(pts.numpy(), Hn, rule), mine
    return gold[f"tp_{M}_{n}"], mine


def _rn(q):
    """A Fraction rounded to the nearest float32 (ties to even, subnormals included), exactly."""
    from fractions import Fraction
    if q == 0:
        return np.float32(0)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24
    while q >= Fraction(2) ** (e + 24):
        e += 1
    while q < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)
    m = q / Fraction(2) ** e
    f, r = divmod(m.numerator, m.denominator)
    if 2 * r > m.denominator or (2 * r == m.denominator and f & 1):
        f += 1
    return np.float32(sign * float(f) * 2.0 ** e)  # f <= 2^24: exact in a double


def test_fma_emulation_is_exact():
    """Against exact rational arithmetic: random operands, cancelling ones, and sums that sit 2^-56 below a
    float's rounding midpoint, where a double sum cast to float rounds twice and lands on the wrong side."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(3000).astype(np.float32), rng.standard_normal(3000).astype(np.float32)
    c = rng.standard_normal(3000).astype(np.float32) * 8
    c[::3] = -(a[::3].astype(np.float64) * b[::3]).astype(np.float32)  # cancellation: the product's own error
    ks = np.arange(16, 24)
    a = np.concatenate([a, (2.0 ** -12 * (1 + 2.0 ** -ks)).astype(np.float32)])
    b = np.concatenate([b, (2.0 ** -12 * (1 - 2.0 ** -ks)).astype(np.float32)])
    c = np.concatenate([c, np.full(8, 1 + 2.0 ** -23, np.float32)])
    got = gc.fma32(a, b, c)
    want = np.array([_rn(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float32)
    ok(got, want, "fma32")
    assert (want[-8:] == np.float32(1 + 2.0 ** -23)).all()
    twice = (a.astype(np.float64) * b + c).astype(np.float32)
    assert gc.ndiff(twice[-8:], want[-8:]) == 8, "the operands do not exercise the double rounding"
    assert gc.aten_plain(3, 44, 3) and not gc.aten_plain(3, 45, 3)
    assert gc.aten_plain(4, 4, 24) and not gc.aten_plain(4, 4, 25)


@pytest.mark.parametrize("M,n", gen.TP)
def test_transform_points_restated(M, n, gold):
    want, mine = tp_want(gold, M, n)
    assert want.shape == ((M, 1, n, 3) if M else (1, n, 3))
    ok(mine, want, f"tp M={M} n={n}")
    if n >= 4:  # randn operands: the other chain shows
        assert gc.ndiff(tp_want(gold, M, n, plain=not gc.tp_plain(n, M > 0))[1], want) > 0


@pytest.mark.parametrize("B,n", gen.P2C)
def test_pixel2cam_restated(B, n, gold):
    depth, pix, K = gen.p2c_inputs(B, n)
    assert gen.sha(depth, pix, K) == gold["shas"][f"p2c_{B}_{n}"], "the regenerated inputs are not the golden's"
    assert float(K[:, 0, 1].abs().min()) > 0.5, "K has a skew"
    want = gold[f"p2c_{B}_{n}"]
    assert want.shape == (B, 4) + gen.HW[n] and (want[:, 3] == 1).all()
    assert gen.sha(want[:, :3]) == gold["shas"][f"p2c_{B}_{n}_h0"], "the non-homogeneous call's digest"
    args = depth.reshape(B, n).numpy(), pix.reshape(B, 3, n).numpy(), gold[f"p2c_{B}_{n}_ki"]  # the reference's K^-1
    assert np.abs(args[2] - torch.inverse(K).numpy()).max() < 1e-6  # (this host's may differ in the last bit)
    ok(gc.pixel2cam(*args, True, gc.p2c_plain(n)).reshape(want.shape), want, f"p2c B={B} n={n}")
    if n >= 44:
        assert gc.ndiff(gc.pixel2cam(*args, True, not gc.p2c_plain(n)).reshape(want.shape), want) > 0


@pytest.mark.parametrize("B,n", gen.C2P)
def test_cam2pixel_restated(B, n, gold):
    cam, proj = gen.c2p_inputs(B, n)
    assert gen.sha(cam, proj) == gold["shas"][f"c2p_{B}_{n}"], "the regenerated inputs are not the golden's"
    want = gold[f"c2p_{B}_{n}"]
    assert want.shape == (B,) + gen.HW[n] + (2,)
    args = cam.reshape(B, 4, n).numpy(), proj.numpy()
    ok(gc.cam2pixel(*args, gc.c2p_plain(n)).reshape(want.shape), want, f"c2p B={B} n={n}")
    if n >= 24:
        assert gc.ndiff(gc.cam2pixel(*args, not gc.c2p_plain(n)).reshape(want.shape), want) > 0
        assert np.isinf(want[B - 1, -1, -1]).all(), "z + 1e-10 == 0 at the last point"
        assert np.isfinite(want.reshape(-1, 2)[:-1]).all()
        assert (gc.chain(args[1], args[0], gc.c2p_plain(n))[:, 2] < 0).any(), "a negative z"
    assert (float(cam[:, 3].min()) != 1.0) and bool((proj[:, 3] != torch.tensor([0.0, 0.0, 0.0, 1.0])).any())


@pytest.mark.parametrize("Ht,Wt", gen.PC)
def test_plane_coords_restated(Ht, Wt, gold):
    tag, n = f"pc_{Ht}x{Wt}", Ht * Wt
    hom = gold[tag + "_hom"]
    imgs, pts = gen.pc_inputs(Ht, Wt, hom)
    assert gen.sha(imgs, pts, *gen.pc_cameras(Ht, Wt)) == gold["shas"][tag], "the regenerated inputs are not the golden's"
    want = gold[tag + "_coords"]
    assert want.shape == (2, 2, Ht, Wt, 2) and gold[tag + "_out"].shape == (2, 2, 3, Ht, Wt)
    plain = gc.tp_plain(n, True)
    flat = pts.reshape(2, 2, n, 3).numpy()
    ok(gc.plane_coords(flat, hom, Ht, Wt, plain).reshape(want.shape), want, tag)
    assert gc.ndiff(gc.plane_coords(flat, hom, Ht, Wt, not plain).reshape(want.shape), want) > 0
    w = gc.transform_points(flat, hom, plain)[..., 2]
    assert (w[:, 1, 1] == 0).all() and (w[:, 1, -1] == 0).all(), "w == 0 where the homography is affine"
    assert bool((w[:, 0, 0] == 0).all()) == plain, "(h7, -h6, 0): w == 0 under the plain chain only"
    if Ht == 1 or Wt == 1:
        assert not np.isfinite(want).all() and np.isfinite(want).any()
    else:
        assert np.isfinite(want).all()


def test_plane_coords_straddle(gold):
    """4x11 is the last plain size, 5x9 the first that MKL rounds."""
    assert gc.tp_plain(44, True) and not gc.tp_plain(45, True) and not gc.tp_plain(44, False)
    assert (4, 11) in gen.PC and (5, 9) in gen.PC


@pytest.mark.parametrize("k,n", gen.NH)
def test_normalize_homogeneous_restated(k, n, gold):
    tag = f"nh_{k}_{n}"
    pts = gen.nh_inputs(k, n)
    assert gen.sha(pts) == gold["shas"][tag], "the regenerated inputs are not the golden's"
    out, after = gc.normalize_homogeneous(pts.numpy())
    ok(out, gold[tag + "_out"], tag)
    ok(after[:, k], gold[tag + "_w"], tag + " w after the call")
    assert gen.sha(after) == gold["shas"][tag + "_after"], "the input after the call"
    zero = pts.numpy()[:, k] == 0
    assert gc.same(after[~zero], pts.numpy()[~zero]) is None, "only w == 0 rows are rewritten"
    if n > 1:
        w = pts.numpy()[:, k]
        for rows in (w[:6], w[-6:]):
            assert (rows == 0).sum() == 2 and np.signbit(rows[rows == 0]).sum() == 1
            assert np.isinf(rows).sum() == 2 and np.isnan(rows).sum() == 1
            assert ((rows != 0) & (np.abs(rows) < np.finfo(np.float32).tiny)).sum() == 1  # the subnormal


@pytest.mark.parametrize("n", gen.CODEC_N)
def test_codecs_restated(n, gold):
    pre, dep = gen.codec_inputs(n)
    assert gen.sha(pre, dep) == gold["shas"][f"codec_{n}"], "the regenerated inputs are not the golden's"
    ok(gc.preprocess(pre.numpy()), gold[f"pre_{n}"], f"preprocess n={n}")
    want = gold[f"dep_{n}"]
    assert want.dtype == np.uint8 and want.shape == (n,)
    assert np.array_equal(gc.deprocess_u8(dep.numpy()), want), f"deprocess n={n}"
    if n >= 32:
        d = dep.numpy()
        for rows in (d[:16], d[-16:]):
            assert np.isnan(rows).any() and np.isinf(rows).sum() >= 2 and (np.abs(rows) == np.float32(3e9)).sum() == 2
        v = ((d + np.float32(1)) / np.float32(2)) * np.float32(255)
        ends = np.concatenate([v[:16], v[-16:]])
        for edge in (0.0, 255.0, 256.0, 2.0 ** 31, -2.0 ** 31):
            e = np.float32(edge)
            assert sum(int((ends == x).sum()) for x in (e, np.nextafter(e, np.float32(np.inf)),
                                                        np.nextafter(e, np.float32(-np.inf)))) >= 1, edge
        assert ((ends < 0) & (ends > -1)).any(), "a negative fraction"


# ---------------------------------------------------------------------------
# the fused kernels' smallest in-contract frame through the oracle
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bd(gold):
    b = gen.boundary_inputs()
    assert gen.sha(*[b[k] for k in sorted(b)]) == gold["shas"]["bd"], "the regenerated inputs are not the golden's"
    return b


def test_oracle_renders_the_smallest_in_contract_frame(bd, gold):
    from mpi_vision_amd import _host
    from oracle import oracle
    assert gold["bd_render"].shape == (1, 5, 9, 3)
    homs = np.ascontiguousarray(gold["bd_homs"].transpose(1, 0, 2, 3)).reshape(1, 5, 9)  # the reference's own
    ok(oracle.render(bd["mpi"].numpy(), homs), gold["bd_render"], "render 5x9x5")
    mine = _host.render_homographies(bd["pose"], bd["planes"], bd["K"], 1).numpy()
    if host_agrees(torch.inverse(bd["K"]), gold["bd_ki"][:1]):
        ok(mine, homs, "render_homographies on a host whose LAPACK agrees with the golden's")
    else:  # K^-1 differs in its last bit here: so may the homographies, the frame stays the oracle's
        assert np.abs(mine - homs).max() < 1e-5


def test_oracle_warps_and_sweeps_the_smallest_in_contract_frame(bd, gold):
    from mpi_vision_amd import _host
    from oracle import oracle
    mine, proj = _host.psv_matrices(bd["K2"], bd["K2"], bd["pose2"])
    ki = gold["bd_ki"]  # the reference's K^-1: the goldens on any host
    if host_agrees(mine, ki):
        ok(mine.numpy().reshape(2, 3, 3), ki, "psv_matrices' K^-1 on a host whose LAPACK agrees with the golden's")
    ok(oracle.inverse_warp(bd["img"].numpy(), ki, proj.numpy(), bd["depth"].numpy()), gold["bd_warp"],
       "inverse warp 5x9")
    assert gold["bd_sweep"].shape == (2, 5, 9, 9)
    ok(oracle.plane_sweep(bd["img"].numpy(), ki, proj.numpy(), gen.SWEEP_DEPTHS, 5, 9), gold["bd_sweep"],
       "plane sweep 5x9, D = 3")
