"""The separable row loop of the rows kernels (render.hip render_rows_vs_pixels, render_texel.hip
render_tex_vs_pixels): the 24-bit tap address, its wide-row guard and the first plane's alpha.

On a column-separable view the rows form the tap address as __mul24(cy, row pitch in bytes) + coff,
which is exact only while the pitch fits 24 signed bits; beyond that the kernels must keep the row
recipe, the render_colsep=1 hook included.  The float kernel replaces plane p_begin's alpha by 1 in the
arm of its consume that also holds the per-lane tap selects, so rows that continue carry no select.
Neither may show in a frame: every comparison is bit for bit against the CPU oracle on the same
[V,P,9] homographies, into output buffers prefilled with NaN.

Frames (H x W) 70 x 13 and 64 x 7: a partial tile in x and a partial last strip for every R.  The
stretched shapes reach the float rows kernels through render_vshare; they sample the image in their
top strips only (the lower tiles are dead), so the float flavours also run on 70 x 61.  The u8, f16 and
alpha renders have no such option in the shipped library and route 4 rows with tap reuse only on a
near-square or chip-filling launch: they run on 70 x 61 too (4 rows in flight; 2 at 416 views).

These tests cannot show that the path is taken (both recipes give the same bits on separable views);
the wide-row cases show the guard, because the forced path would compute other offsets without it, and
the VALU counters of a profile show the rest."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import assert_bits
from lattice_cases import match

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

P = 3
V = 3
SHAPES = [(70, 13), (64, 7)]
SHAPE_IDS = ["70x13", "64x7"]
NEAR_SQUARE = (70, 61)
ADDR_SHAPES = SHAPES + [NEAR_SQUARE]
ADDR_IDS = SHAPE_IDS + ["70x61"]
# render_vshare -> (R, rows in flight): the shipped flavours
VSHARE = {3: (8, 4), 4: (6, 3), 5: (9, 3), 11: (4, 4)}
VSHARE_IDS = [f"r{r}d{d}" for _, (r, d) in sorted(VSHARE.items())]
NAN = float("nan")


def _poses(n):
    """yaw plus translation: column-separable views"""
    out = []
    for k in range(n):
        a = 2.0 * math.pi * (100 + 37 * k) / 1000
        t = (0.05 * math.sin(a), 0.02 * math.cos(a), 0.03 * math.sin(math.pi * (k + 1) / (n + 1)))
        out.append(configs.pose_from(configs.rot_y(1.0 * math.sin(a)), t))
    return out


@functools.lru_cache(maxsize=None)
def _homs(hw, nv=V, planes=P):
    H, W = hw
    f = configs.focal_from_fov(W)
    K = configs.f32([configs.intrinsics_matrix(f, f, W / 2.0, H / 2.0)] * nv)
    h = _host.render_homographies(configs.f32(_poses(nv)), configs.f32(configs.inv_depths(1, 100, max(planes, 2))[:planes]), K, nv)
    # at these odd sizes the host chain leaves 1e-9 of rounding residue in h[1] and h[7] (exact zeros at
    # the configs' sizes, tests/test_colsep_premise.py); the views here are separable by construction
    assert (h[..., 1].abs() < 1e-7).all() and (h[..., 7].abs() < 1e-7).all()
    h = h.clone()
    h[..., 1] = 0.0
    h[..., 7] = 0.0
    return h


@functools.lru_cache(maxsize=None)
def _mpi(hw, planes=P):
    return configs.synthetic_mpi(1, hw[0], hw[1], planes, 3000 + hw[0] + planes)


@functools.lru_cache(maxsize=None)
def _packed(hw, planes=P):
    return _lib.pack_planes(_mpi(hw, planes)[0].to("cuda:0"))


def _full(hw, nv, planes=P):
    return np.broadcast_to(_mpi(hw, planes).numpy(), (nv,) + hw + (planes, 4))


@functools.lru_cache(maxsize=None)
def _want(hw, nv=V, planes=P):
    return oracle.render(_full(hw, nv, planes), _homs(hw, nv, planes).numpy())


def _render(hw, homs, packed):
    out = torch.full((homs.shape[0],) + hw + (3,), NAN, device="cuda:0")
    return _lib.render_packed(packed, homs, out=out).cpu().numpy()


def _census(hw, homs, packed):
    dev = torch.device("cuda:0")
    nv, planes = homs.shape[0], homs.shape[1]
    out = torch.full((nv,) + hw + (3,), NAN, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib._call("mpiv_render_packed_census", packed, hw[0], hw[1], planes, homs.reshape(nv, planes, 9).to(dev), nv,
               out, n, _lib._stream(dev))
    return out.cpu().numpy(), int(n.item())


# ---------------------------------------------------------------------------
# the tap address at ordinary widths
# ---------------------------------------------------------------------------

def _float_flavour(hw, opts, kopts):
    homs, want, counts = _homs(hw), _want(hw), {}
    for cs in (0, -1, 1):
        kopts(render_colsep=cs, **opts)
        assert_bits(_render(hw, homs, _packed(hw)), want, f"render_colsep={cs}")
        frames, counts[cs] = _census(hw, homs, _packed(hw))
        assert_bits(frames, want, f"census build, render_colsep={cs}")
    print(f"gather instructions: {counts}")
    assert counts[0] == counts[-1] == counts[1] > 0


@pytest.mark.parametrize("vshare", sorted(VSHARE), ids=VSHARE_IDS)
@pytest.mark.parametrize("hw", ADDR_SHAPES, ids=ADDR_IDS)
def test_address_every_flavour(hw, vshare, dev, kopts):
    """Every shipped (R, D) without same-row reuse: render_colsep 0, -1 and 1 equal the oracle, and the
    counting build counts the same gathers with and without the path."""
    _float_flavour(hw, dict(render_vshare=vshare, render_same=-1), kopts)


@pytest.mark.parametrize("same", [1, 2], ids=["same", "oob"])
@pytest.mark.parametrize("vshare", [4, 11], ids=["r6d3", "r4d4"])
@pytest.mark.parametrize("hw", SHAPES, ids=SHAPE_IDS)
def test_address_same_row_flavours(hw, vshare, same, dev, kopts):
    """The same-row flavours: (6, 3), the automatic one, with and without OOB, and (4, 4)."""
    _float_flavour(hw, dict(render_vshare=vshare, render_same=same), kopts)


@pytest.mark.parametrize("hw", ADDR_SHAPES, ids=ADDR_IDS)
def test_address_partial_and_row_band(hw, dev, kopts):
    """The (C, T) flavour: the partial of planes [1, P) and a row band that starts off a tile boundary
    and ends inside a tile, at render_colsep 0, -1 and 1."""
    H, W = hw
    homs = _homs(hw)
    want = oracle.render_ct(_full(hw, V), homs.numpy(), 1, P, back=False)
    y_lo, y_hi = 5, H - 7
    for cs in (0, -1, 1):
        kopts(render_colsep=cs, render_vshare=4, render_same=-1)
        ct = torch.full((V, H, W, 4), NAN, device=dev)
        _lib.render_packed_ct(_packed(hw), homs, False, 1, P, out=ct)
        assert_bits(ct, want, f"ct [1,{P}), render_colsep={cs}")
        band = torch.full((V, H, W, 4), NAN, device=dev)
        _lib.render_packed_ct_rows(_packed(hw), homs, False, y_lo, y_hi, band, 1, P)
        assert_bits(band[:, y_lo:y_hi], want[:, y_lo:y_hi], f"rows [{y_lo},{y_hi}), render_colsep={cs}")
        assert torch.isnan(band[:, :y_lo]).all() and torch.isnan(band[:, y_hi:]).all(), cs


def _u8_case(hw, nv=V):
    H, W = hw
    g = torch.Generator().manual_seed(5 + H)
    u8 = torch.randint(0, 256, (H, W, P, 4), generator=g, dtype=torch.uint8)
    u8[:, :, 0, 3] = 255
    fl = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)
    homs = _homs(hw, nv)
    return u8, homs, oracle.render(np.broadcast_to(fl[None], (nv,) + fl.shape), homs.numpy())


@pytest.mark.parametrize("flight", [0, 2, 8], ids=["d4", "d2", "d8"])
@pytest.mark.parametrize("hw", ADDR_SHAPES, ids=ADDR_IDS)
def test_address_u8_kernel(hw, flight, dev, kopts):
    """render_u8_kernel: 4 rows with tap reuse and 4 (automatic at this size), 2 and 8 rows in flight on
    the near-square frame; two plain rows on the stretched ones (the shipped library has no option that
    sends them elsewhere)."""
    u8, homs, want = _u8_case(hw)
    pk = _lib.pack_planes_u8(u8.to(dev))
    for cs in (0, -1, 1):
        kopts(render_colsep=cs, u8_flight=flight)
        out = torch.full((V,) + hw + (3,), NAN, device=dev)
        _lib.render_packed_u8(pk, homs, out=out, route_float=False)
        assert_bits(out, want, f"render_colsep={cs}")


def _half_mpi(hw):
    return _mpi(hw)[0].half()


@pytest.mark.parametrize("hw,nv", [(SHAPES[0], V), (SHAPES[1], V), (NEAR_SQUARE, V), (NEAR_SQUARE, 416)],
                         ids=["70x13", "64x7", "70x61", "70x61v416"])
def test_address_f16_and_alpha_kernels(hw, nv, dev, kopts):
    """render_f16_kernel and render_alpha_kernel: two plain rows on the stretched frames, 4 rows with
    tap reuse on the near-square one (4 in flight; 2 at 416 views, a launch of 2080 blocks)."""
    homs = _homs(hw, nv)
    half = _half_mpi(hw)
    pk16 = _lib.pack_planes_f16(half.to(dev))
    want16 = oracle.render(np.broadcast_to(half.float().numpy()[None], (nv,) + hw + (P, 4)), homs.numpy())
    colors = torch.tensor([[0.25, -1.5, 3.0], [1.0, 0.5, -0.125], [2.0, 0.0, 0.75]])
    tinted = _mpi(hw)[0].clone()
    tinted[..., :3] = colors
    pka = _lib.pack_planes_alpha(_mpi(hw)[0].to(dev))
    wanta = oracle.render(np.broadcast_to(tinted.numpy()[None], (nv,) + hw + (P, 4)), homs.numpy())
    for cs in (0, -1, 1):
        kopts(render_colsep=cs)
        out = torch.full((nv,) + hw + (3,), NAN, device=dev)
        _lib.render_packed_f16(pk16, homs, out=out, route_float=False)
        assert_bits(out, want16, f"f16, render_colsep={cs}")
        out = torch.full((nv,) + hw + (3,), NAN, device=dev)
        _lib.render_packed_alpha(pka, colors, homs, out=out)
        assert_bits(out, wanta, f"alpha, render_colsep={cs}")


# ---------------------------------------------------------------------------
# wide rows: the byte pitch does not fit 24 bits
# ---------------------------------------------------------------------------

def _wide_homs(H, W, planes):
    """[1, planes, 9] separable planes that sample the wide frame near the identity (the reference
    normalises x by H - 1 and y by W - 1): px ~ 1.0001 x + 0.3 + p, py = y + 0.25 - p, so the clamped tap
    rows are -1, 0 and 1 -- on the forced path an unguarded 24-bit pitch would move all but row 0."""
    out = []
    for p in range(planes):
        sx, sy = (H - 1) / W, (W - 1) / H
        out.append([1.0001 * sx, 0.0, (0.8 + p) * sx, 0.0, sy, (0.75 - p) * sy, 1e-9, 0.0, 1.0])
    return torch.tensor([out], dtype=torch.float32)


@pytest.mark.parametrize("opts", [{}, dict(render_vshare=4, render_same=-1), dict(render_vshare=11, render_same=-1)],
                         ids=["auto", "r6d3", "r4d4"])
def test_wide_rows_float(opts, dev, kopts):
    """(W + 4) * 16 >= 2^23 (W = 524 300, H = 2, 2 planes, one view): render_colsep 0 and 1 both equal
    the oracle, i.e. the kernel refuses the path whatever the option says."""
    H, W, planes = 2, 524300, 2
    assert (W + 4) * 16 >= 1 << 23
    g = torch.Generator().manual_seed(77)
    mpi = torch.rand((H, W, planes, 4), generator=g)
    homs = _wide_homs(H, W, planes)
    want = oracle.render(mpi.numpy()[None], homs.numpy())
    assert np.count_nonzero(want) > want.size // 2  # the frame samples the image, not the border
    pk = _lib.pack_planes(mpi.to(dev))
    for cs in (0, 1):
        kopts(render_colsep=cs, **opts)
        assert_bits(_render((H, W), homs, pk), want, f"render_colsep={cs}")


def test_wide_rows_u8(dev, kopts):
    """The same for 4-byte texels: (W + 4) * 4 >= 2^23 at W = 2 097 152."""
    H, W, planes = 2, 1 << 21, 2
    assert (W + 4) * 4 >= 1 << 23
    g = torch.Generator().manual_seed(78)
    u8 = torch.randint(0, 256, (H, W, planes, 4), generator=g, dtype=torch.uint8)
    fl = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)
    homs = _wide_homs(H, W, planes)
    want = oracle.render(fl[None], homs.numpy())
    assert np.count_nonzero(want) > want.size // 2
    pk = _lib.pack_planes_u8(u8.to(dev))
    for cs in (0, 1):
        kopts(render_colsep=cs)
        out = torch.full((1, H, W, 3), NAN, device=dev)
        _lib.render_packed_u8(pk, homs, out=out, route_float=False)
        assert_bits(out, want, f"render_colsep={cs}")


# ---------------------------------------------------------------------------
# the first plane
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("vshare,same", [(3, -1), (4, -1), (5, -1), (11, -1), (4, 1), (4, 2), (11, 1)],
                         ids=VSHARE_IDS + ["same", "oob", "r4d4same"])
def test_first_plane_short_ranges(vshare, same, planes, dev, kopts):
    """P = 1 (only the plane that replaces the background) and P = 2."""
    hw = SHAPES[1]
    homs, want = _homs(hw, V, planes), _want(hw, V, planes)
    for cs in (0, -1):
        kopts(render_colsep=cs, render_vshare=vshare, render_same=same)
        assert_bits(_render(hw, homs, _packed(hw, planes)), want, f"P={planes}, render_colsep={cs}")


@pytest.mark.parametrize("back", [False, True], ids=["back0", "back1"])
@pytest.mark.parametrize("rng", [(1, 3), (2, 3), (1, 2)], ids=["p1-3", "p2-3", "p1-2"])
@pytest.mark.parametrize("vshare,same", [(4, -1), (11, -1), (4, 1)], ids=["r6d3", "r4d4", "same"])
def test_first_plane_partials(vshare, same, rng, back, dev, kopts):
    """(C, T) partials that start at p_begin > 0, one plane long among them, with `back` set (the
    range's first plane replaces the background) and clear (its alpha counts)."""
    hw = SHAPES[0]
    a, b = rng
    homs = _homs(hw)
    want = oracle.render_ct(_full(hw, V), homs.numpy(), a, b, back=back)
    for cs in (0, -1):
        kopts(render_colsep=cs, render_vshare=vshare, render_same=same)
        ct = torch.full((V,) + hw + (4,), NAN, device=dev)
        _lib.render_packed_ct(_packed(hw), homs, back, a, b, out=ct)
        assert_bits(ct, want, f"ct [{a},{b}) back={back}, render_colsep={cs}")


def _odd_texels(hw, p_begin):
    """A finite MPI whose plane p_begin holds -0, +-Inf and NaN, in alpha and in colour."""
    H, W = hw
    g = torch.Generator().manual_seed(91 + H)
    m = torch.rand((H, W, P, 4), generator=g)
    m[..., :3] = m[..., :3] * 2 - 1
    q = m[:, :, p_begin]
    q[0::5, :, 3] = -0.0
    q[1::5, :, 3] = float("inf")
    q[2::5, :, 3] = NAN
    q[3::5, 0::2, 3] = float("-inf")
    q[:, 1::4, 0] = -0.0
    q[7::9, :, 1] = float("inf")
    q[4::9, 2::3, 2] = NAN
    return m


@pytest.mark.parametrize("p_begin", [0, 1])
@pytest.mark.parametrize("vshare,same", [(4, -1), (11, -1), (3, -1), (4, 1)], ids=["r6d3", "r4d4", "r8d4", "same"])
def test_first_plane_odd_texels(vshare, same, p_begin, dev, kopts):
    """-0, Inf and NaN texels in plane p_begin: the full composite ignores plane 0's alpha whatever it
    holds; a partial from p_begin = 1 replaces with `back` and blends without.  NaN positions and every
    other bit as the oracle's."""
    hw = SHAPES[0]
    mpi = _odd_texels(hw, p_begin)
    homs = _homs(hw)
    full = np.broadcast_to(mpi.numpy()[None], (V,) + hw + (P, 4))
    pk = _lib.pack_planes(mpi.to(dev))
    for cs in (0, -1):
        kopts(render_colsep=cs, render_vshare=vshare, render_same=same)
        if p_begin == 0:
            want = oracle.render(full, homs.numpy())
            assert np.isfinite(want[..., 2]).any() and np.isnan(want).any()
            match(_render(hw, homs, pk), want, f"render, render_colsep={cs}")
        for back in (False, True):
            want = oracle.render_ct(full, homs.numpy(), p_begin, P, back=back)
            ct = torch.full((V,) + hw + (4,), NAN, device=dev)
            _lib.render_packed_ct(pk, homs, back, p_begin, P, out=ct)
            match(ct, want, f"ct [{p_begin},{P}) back={back}, render_colsep={cs}")


def test_first_plane_odd_texels_f16(dev, kopts):
    """The texel template (4 rows with tap reuse, 4 in flight) on half texels with -0, Inf and NaN in
    plane 0, and the partial from plane 1 with the same in plane 1."""
    hw = NEAR_SQUARE
    homs = _homs(hw)
    for p_begin in (0, 1):
        half = _odd_texels(hw, p_begin).half()
        full = np.broadcast_to(half.float().numpy()[None], (V,) + hw + (P, 4))
        pk = _lib.pack_planes_f16(half.to(dev))
        for cs in (0, -1):
            kopts(render_colsep=cs)
            if p_begin == 0:
                out = torch.full((V,) + hw + (3,), NAN, device=dev)
                _lib.render_packed_f16(pk, homs, out=out, route_float=False)
                match(out, oracle.render(full, homs.numpy()), f"f16 render, render_colsep={cs}")
            for back in (False, True):
                ct = torch.full((V,) + hw + (4,), NAN, device=dev)
                _lib.render_packed_f16_ct(pk, homs, back, p_begin, P, out=ct)
                match(ct, oracle.render_ct(full, homs.numpy(), p_begin, P, back=back),
                      f"f16 ct [{p_begin},{P}) back={back}, render_colsep={cs}")
