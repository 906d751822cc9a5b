"""The rows kernels' column-separable issue path (render.hip ColSet, option render_colsep).

A view whose planes all have h[1] == h[7] == +-0 (a camera that yaws and translates, no pitch or
roll) computes the u, w chain and everything derived from it once per column and plane instead of
once per row.  The path must be invisible in the output: every comparison here is bit for bit
against the CPU oracle on the same [V,P,9] homographies, for separable views (where automatic
detection may take the path), general views (where it must not), mixtures of both, signed zeros,
near misses, tiles that fail the division proof, plane-range partials and the u8 render.
render_colsep=1 takes the path without the test; on a pitched view it must give other bits, which
shows that the option switches the recipe (so the separable cases are not vacuous).

These tests do not show that automatic detection selects the path on separable input (both paths
give the same bits there); the VALU instruction count of a profile does."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import assert_bits, bits_equal

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

SQ = (100, 100, 16)  # W is no multiple of 64; 100 rows leave a partial 24-row tile
ST = (72, 128, 6)    # stretched: same-row tap reuse (render_same) with render_vshare=4
VMAX = 12


def rot_x(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


def _matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _poses(kind, n=VMAX):
    """n poses of the sway path (yaw + translation), optionally with 1 degree of pitch or roll,
    or a 60 degree yaw."""
    out = []
    for k in range(n):
        a = 2.0 * math.pi * (100 + 37 * k) / 1000
        R = configs.rot_y(60.0 if kind == "yaw60" else 1.0 * math.sin(a))
        if kind == "pitch":
            R = _matmul(R, rot_x(1.0))
        elif kind == "roll":
            R = _matmul(R, rot_z(1.0))
        t = (0.05 * math.sin(a), 0.02 * math.cos(a), 0.03 * math.sin(math.pi * k / n))
        out.append(configs.pose_from(R, t))
    return out


@functools.lru_cache(maxsize=None)
def _homs(kind, shape, focal=None):
    H, W, P = shape
    f = configs.focal_from_fov(W) if focal is None else focal
    K = configs.f32([configs.intrinsics_matrix(f, f, W / 2.0, H / 2.0)] * VMAX)
    return _host.render_homographies(configs.f32(_poses(kind)), configs.f32(configs.inv_depths(1, 100, P)), K, VMAX)


@functools.lru_cache(maxsize=None)
def _mpi(shape):
    H, W, P = shape
    return configs.synthetic_mpi(1, H, W, P, 1000 + H)


@functools.lru_cache(maxsize=None)
def _packed(shape):
    return _lib.pack_planes(_mpi(shape)[0].to("cuda:0"))


def _want(shape, homs):
    V = homs.shape[0]
    return oracle.render(np.broadcast_to(_mpi(shape).numpy(), (V,) + shape + (4,)), homs.numpy())


@functools.lru_cache(maxsize=None)
def _want_kind(kind, shape, V, focal=None):
    return _want(shape, _homs(kind, shape, focal)[:V])


def _render(shape, homs):
    return _lib.render_packed(_packed(shape), homs).cpu().numpy()


def _census(shape, homs):
    H, W, P = shape
    dev = torch.device("cuda:0")
    V = homs.shape[0]
    out = torch.empty((V, H, W, 3), device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib._call("mpiv_render_packed_census", _packed(shape), H, W, P, homs.reshape(V, P, 9).to(dev), V, out, n,
               _lib._stream(dev))
    return out.cpu().numpy(), int(n.item())


# (shape, V, debug options): default routing reaches (R, rows in flight) = (4, 4) at V <= 2, (8, 4) at
# V <= 8 and (6, 3) above; render_vshare=5 is (9, 3); the stretched shape adds SAME and SAME + OOB
FLAVOURS = [(SQ, 1, {}), (SQ, 2, {}), (SQ, 5, {}), (SQ, 12, {}), (SQ, 12, dict(render_vshare=5)),
            (ST, 2, dict(render_vshare=4, render_same=1)), (ST, 12, dict(render_vshare=4, render_same=1)),
            (ST, 2, dict(render_vshare=4, render_same=2)), (ST, 12, dict(render_vshare=4, render_same=2))]
FLAVOUR_IDS = ["44v1", "44v2", "84v5", "63v12", "93v12", "same_v2", "same_v12", "oob_v2", "oob_v12"]


@pytest.mark.parametrize("shape,V,opts", FLAVOURS, ids=FLAVOUR_IDS)
def test_separable_views_every_flavour(shape, V, opts, dev, kopts):
    """Sway-path views: render_colsep 0, -1 and 1 all equal the oracle; the census build gives the same
    frames and the same gather count with and without the path (the offsets are identical)."""
    homs = _homs("sway", shape)[:V]
    assert (homs[..., 1] == 0).all() and (homs[..., 7] == 0).all()
    want = _want_kind("sway", shape, V)
    counts = {}
    for cs in (0, -1, 1):
        kopts(render_colsep=cs, **opts)
        assert_bits(_render(shape, homs), want, f"render_colsep={cs}")
        frames, counts[cs] = _census(shape, homs)
        assert_bits(frames, want, f"census build, render_colsep={cs}")
    print(f"gather instructions: {counts}")
    assert counts[0] == counts[-1] == counts[1] > 0


@pytest.mark.parametrize("kind", ["pitch", "roll"])
@pytest.mark.parametrize("shape,V,opts", FLAVOURS, ids=FLAVOUR_IDS)
def test_general_views_keep_the_row_recipe(shape, V, opts, kind, dev, kopts):
    """1 degree of pitch or roll: automatic detection must not fire (0 and -1 equal the oracle), and
    forcing the path (1) must change the bits."""
    homs = _homs(kind, shape)[:V]
    assert (homs[..., 1] != 0).all()  # (a pure roll keeps h[7] == 0)
    want = _want_kind(kind, shape, V)
    for cs in (0, -1):
        kopts(render_colsep=cs, **opts)
        assert_bits(_render(shape, homs), want, f"render_colsep={cs}")
    kopts(render_colsep=1, **opts)
    assert not bits_equal(_render(shape, homs), want), "render_colsep=1 did not switch the recipe"


SOME = [FLAVOURS[i] for i in (1, 2, 3, 4, 6, 7)]
SOME_IDS = [FLAVOUR_IDS[i] for i in (1, 2, 3, 4, 6, 7)]


@pytest.mark.parametrize("shape,V,opts", SOME, ids=SOME_IDS)
def test_mixed_planes_and_mixed_views(shape, V, opts, dev, kopts):
    """Odd planes from the pitched pose inside every view; separable and pitched views alternating
    in one launch: both equal the oracle with automatic detection."""
    sep, pitch = _homs("sway", shape)[:V], _homs("pitch", shape)[:V]
    planes = sep.clone()
    planes[:, 1::2] = pitch[:, 1::2]
    views = sep.clone()
    views[1::2] = pitch[1::2]
    kopts(render_colsep=0, **opts)
    assert_bits(_render(shape, planes), _want(shape, planes), "mixed planes")
    assert_bits(_render(shape, views), _want(shape, views), "mixed views")


@pytest.mark.parametrize("shape,V,opts", SOME, ids=SOME_IDS)
def test_signed_zeros(shape, V, opts, dev, kopts):
    """h[1], h[7] = -0 everywhere, and +0 / -0 mixed per plane and per entry: still separable,
    still the oracle's bits (0 and the forced path)."""
    base = _homs("sway", shape)[:V]
    neg = base.clone()
    neg[..., 1] = -0.0
    neg[..., 7] = -0.0
    mix = base.clone()
    mix[:, 0::2, 1] = -0.0
    mix[:, 1::3, 7] = -0.0
    for name, homs in (("all -0", neg), ("mixed", mix)):
        assert (homs[..., 1] == 0).all() and (homs[..., 7] == 0).all() and torch.signbit(homs[..., 1]).any()
        want = _want(shape, homs)
        for cs in (0, 1):
            kopts(render_colsep=cs, **opts)
            assert_bits(_render(shape, homs), want, f"{name}, render_colsep={cs}")


@pytest.mark.parametrize("shape,V,opts", SOME, ids=SOME_IDS)
def test_near_misses_are_not_detected(shape, V, opts, dev, kopts):
    """h[1] = 2^-20 with h[7] = 0, and h[1] = 0 with h[7] = 2^-30: not separable, the oracle's bits at 0."""
    base = _homs("sway", shape)[:V]
    a = base.clone()
    a[..., 1] = 2.0 ** -20
    b = base.clone()
    b[..., 7] = 2.0 ** -30
    kopts(render_colsep=0, **opts)
    for name, homs in (("h1 = 2^-20", a), ("h7 = 2^-30", b)):
        want = _want(shape, homs)
        assert_bits(_render(shape, homs), want, name)
    # the forced path ignores the row term, so these inputs do tell the two recipes apart
    kopts(render_colsep=1, **opts)
    assert not bits_equal(_render(shape, a), _want(shape, a))


@pytest.mark.parametrize("V,opts", [(2, {}), (5, {}), (12, {}), (12, dict(render_vshare=5))],
                         ids=["44v2", "84v5", "63v12", "93v12"])
def test_large_yaw_guarded_and_proven_tiles(V, opts, dev, kopts):
    """60 degrees of yaw at a focal of 60 pixels: w changes sign inside the frame, so some tiles fail
    the division proof (the guarded path) and others take the column path; NaN bits included."""
    homs = _homs("yaw60", SQ, 60.0)[:V]
    assert (homs[..., 1] == 0).all() and (homs[..., 7] == 0).all()
    w_left, w_right = homs[..., 8], homs[..., 6] * 99.0 + homs[..., 8]
    assert ((w_left > 0) & (w_right < 0)).any() or ((w_left < 0) & (w_right > 0)).any()
    want = _want_kind("yaw60", SQ, V, 60.0)
    for cs in (0, -1):
        kopts(render_colsep=cs, **opts)
        assert_bits(_render(SQ, homs), want, f"render_colsep={cs}")


@pytest.mark.parametrize("kind", ["sway", "pitch"])
@pytest.mark.parametrize("shape,V,opts", SOME, ids=SOME_IDS)
def test_plane_range_partials_and_row_bands(shape, V, opts, kind, dev, kopts):
    """The (C, T) flavour: plane-range partials (p_begin > 0 among them) equal the oracle's, their
    combine equals the partials' combine without the path, and a row band that starts and ends inside
    a tile equals the same rows of the whole partial."""
    H, W, P = shape
    homs = _homs(kind, shape)[:V]
    full = np.broadcast_to(_mpi(shape).numpy(), (V,) + shape + (4,))
    cuts = [0, P // 3, P]
    got = {}
    for cs in (0, -1):
        kopts(render_colsep=cs, **opts)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ct = _lib.render_packed_ct(_packed(shape), homs, a == 0, a, b)
            assert_bits(ct.cpu().numpy(), oracle.render_ct(full, homs.numpy(), a, b, back=(a == 0)),
                        f"ct [{a},{b}), render_colsep={cs}")
            parts.append(ct)
        band = torch.full_like(parts[1], float("nan"))
        _lib.render_packed_ct_rows(_packed(shape), homs, False, 5, H - 7, band, cuts[1], P)
        assert torch.equal(band[:, 5:H - 7].view(torch.int32), parts[1][:, 5:H - 7].view(torch.int32)), cs
        assert torch.isnan(band[:, :5]).all() and torch.isnan(band[:, H - 7:]).all()
        got[cs] = _lib.combine_ct(torch.stack(parts)).cpu().numpy()
    assert_bits(got[0], got[-1], "combine")
    np.testing.assert_allclose(got[0], _want_kind(kind, shape, V), rtol=0, atol=1e-5)


@pytest.mark.parametrize("kind", ["sway", "pitch"])
@pytest.mark.parametrize("V,flight", [(1, 0), (1, 2), (1, 8), (40, 0), (40, 2)])
def test_u8_render(V, flight, kind, dev, kopts):
    """The u8 rows kernel at 1 and 40 views (2, 4 and 8 rows in flight): with the path (0) it equals
    the run without (-1) and the float render of u8 / 255, on separable and pitched poses."""
    H, W, P = SQ
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (H, W, P, 4), generator=g, dtype=torch.uint8)
    u8[:, :, 0, 3] = 255
    homs = _homs(kind, SQ)
    homs = torch.cat([homs] * 4)[:V] if V > VMAX else homs[:V]
    pk = _lib.pack_planes_u8(u8.to(dev))
    fl = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)
    want = _lib.render_packed(_lib.pack_planes(torch.from_numpy(fl).to(dev)), homs).cpu().numpy()
    got = {}
    for cs in (0, -1):
        kopts(render_colsep=cs, u8_flight=flight)
        got[cs] = _lib.render_packed_u8(pk, homs, route_float=False).cpu().numpy()
    assert_bits(got[0], got[-1], "render_colsep 0 vs -1")
    assert_bits(got[0], want, "u8 vs the float render of u8 / 255")
    if V == 1:
        assert_bits(got[0], oracle.render(fl[None], homs.numpy()), "u8 vs oracle")
