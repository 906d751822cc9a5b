"""Exact-lattice sample positions, huge / w == 0 / non-finite homographies and non-finite texels
through every kernel route (tests/lattice_cases.py).

Every comparison is lattice_cases.match -- equal NaN positions, identical bits elsewhere, signed zeros
included -- against the CPU oracle on the same matrices; the oracle itself is pinned to the reference
on these input classes by tests/test_lattice.py, which also asserts (on the oracle, not on the
kernels) that the cases are not vacuous: the positions lie exactly on texel centres and edges, the
`edge` planes hit the dead-tile thresholds exactly, and the NaN shares are neither 0 nor everything.
Output buffers are prefilled with a finite sentinel, so an unwritten pixel fails the comparison."""
import functools

import numpy as np
import pytest
import torch

import lattice_cases as lc
from lattice_cases import match
from test_render_colsep_gpu import FLAVOUR_IDS, FLAVOURS
from test_render_gpu import NATIVE_KERNELS

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib  # noqa: E402
from oracle import oracle  # noqa: E402

DEV = "cuda:0"
SENT = 7.25e11  # no output of these cases equals it
V = 12
KINDS = ["finite", "nonfinite"]
SAME_SHAPE = (72, 128)  # tests/test_render_colsep_gpu.py ST: neither x nor y exact
GPU_FAMILIES = lc.LATTICE + ["edge", "huge", "w_zero", "nonfinite_h"]
TWO = [lc.X_TWO, lc.Y_TWO]


def shapes_of(fam, shapes=None):
    shapes = lc.RENDER_SHAPES if shapes is None else shapes
    return [s for s in shapes if fam != "edge" or s in TWO]


def planes_of(fam, shape):
    return 4 if fam in ("nonfinite_h", "edge") else len(lc.family(fam, shape))


def make_homs(fam, shape, nv, P):
    if fam == "nonfinite_h":
        six = lc.nonfinite_views(shape, P)
        return np.stack([six[v % 6] for v in range(nv)])
    return lc.views(fam, shape, nv, P)


@functools.lru_cache(maxsize=None)
def _homs(fam, shape, nv=V, P=None):
    P = planes_of(fam, shape) if P is None else P
    return torch.from_numpy(np.ascontiguousarray(make_homs(fam, shape, nv, P), np.float32))


@functools.lru_cache(maxsize=None)
def _tex(kind, shape, P):
    return lc.texels(kind, shape[0], shape[1], P)


@functools.lru_cache(maxsize=None)
def _packed(kind, shape, P):
    return _lib.pack_planes(_tex(kind, shape, P).to(DEV))


def _full(kind, shape, P, nv):
    t = _tex(kind, shape, P).numpy()
    return np.broadcast_to(t[None], (nv,) + t.shape)


@functools.lru_cache(maxsize=None)
def _want(fam, shape, kind, nv=V):
    h = _homs(fam, shape)[:nv]
    return oracle.render(_full(kind, shape, h.shape[1], nv), h.numpy())


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV)


def _render(fam, shape, kind, nv=V):
    h = _homs(fam, shape)[:nv]
    out = _sent(nv, shape[0], shape[1], 3)
    return _lib.render_packed(_packed(kind, shape, h.shape[1]), h, out=out)


def _census(fam_or_homs, shape, kind, nv=V):
    h = _homs(fam_or_homs, shape)[:nv] if isinstance(fam_or_homs, str) else fam_or_homs
    nv, P = h.shape[0], h.shape[1]
    dev = torch.device(DEV)
    out = _sent(nv, shape[0], shape[1], 3)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib._call("mpiv_render_packed_census", _packed(kind, shape, P), shape[0], shape[1], P,
               h.reshape(nv, P, 9).to(dev), nv, out, n, _lib._stream(dev))
    return out, int(n.item())


def setopts(kopts, **opts):
    _lib.reset_debug()
    if opts:
        kopts(**opts)


# ---------------------------------------------------------------------------
# packed float render
# ---------------------------------------------------------------------------

# (the same-row flavours keep the 72 x 128 shape, which has no exact axis: no edge planes there)
PACKED_CASES = [(fl, fam) for fl in FLAVOURS for fam in GPU_FAMILIES if not ("render_same" in fl[2] and fam == "edge")]
PACKED_IDS = [f"{FLAVOUR_IDS[FLAVOURS.index(fl)]}-{fam}" for fl, fam in PACKED_CASES]


@pytest.mark.parametrize("flavour,fam", PACKED_CASES, ids=PACKED_IDS)
def test_packed_render_every_flavour(flavour, fam, dev, kopts):
    """The nine (R, rows in flight) flavours, render_colsep 0 and -1, both texel sets, every shape; the
    counting build gives the same frames."""
    _, nv, opts = flavour
    same = "render_same" in opts
    for shape in ([SAME_SHAPE] if same else shapes_of(fam)):
        for kind in KINDS:
            want = _want(fam, shape, kind, nv)
            for cs in (0, -1):
                setopts(kopts, render_colsep=cs, **opts)
                match(_render(fam, shape, kind, nv), want, f"{shape} {kind} render_colsep={cs}")
            frames, n = _census(fam, shape, kind, nv)
            match(frames, want, f"{shape} {kind} census build")


@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_one_row_kernel_and_tile_orders(fam, dev, kopts):
    """The one-row kernel (render_tile=-1) on every shape; both tile orders on the two-column shapes,
    for the one-row kernel and the default rows route."""
    for kind in KINDS:
        for shape in shapes_of(fam):
            for nv in (2, V):
                setopts(kopts, render_tile=-1)
                match(_render(fam, shape, kind, nv), _want(fam, shape, kind, nv), f"{shape} {kind} one row, {nv} views")
        for shape in shapes_of(fam, TWO):
            for order in (-1, 1):
                for tile in (0, -1):
                    setopts(kopts, render_order=order, render_tile=tile)
                    match(_render(fam, shape, kind), _want(fam, shape, kind),
                          f"{shape} {kind} render_order={order} render_tile={tile}")


@pytest.mark.parametrize("shape", TWO, ids=["129x128", "128x129"])
def test_edge_dead_tiles_gather_less(shape, dev, kopts):
    """`edge` under render_vshare=4 (64 x 24 tiles; the planes of the tile start at row 72 for the y-exact
    shape), every plane of the view the same threshold plane: the frames equal the oracle's, and the
    tile column (row) whose first position is N+1 is dead -- fewer gathers than at N+0.5, where it is
    not; on the low side -2.5 is dead and -2 is not (tile_dead: px0 >= W+1 || px1 < -2)."""
    setopts(kopts, render_vshare=4)
    P = 4
    counts = {}
    for k in range(8):
        plane = lc.family("edge", shape)[k]
        homs = torch.from_numpy(np.broadcast_to(plane, (2, P, 9)).copy())
        for kind in KINDS:
            frames, n = _census(homs, shape, kind)
            match(frames, oracle.render(_full(kind, shape, P, 2), homs.numpy()), f"{lc.EDGE_THRESHOLDS[k]} {kind}")
            counts[k, kind] = n
    print({f"{lc.EDGE_THRESHOLDS[k]} {kind}": n for (k, kind), n in counts.items()})
    for kind in KINDS:
        assert 0 < counts[3, kind] < counts[2, kind], "first position N+1 must be a dead tile, N+0.5 not"
        assert 0 < counts[6, kind] < counts[5, kind], "last position -2.5 must be a dead tile, -2 not"


# ---------------------------------------------------------------------------
# (C, T) partials, row bands, combine
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("nv", [2, V])
@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_plane_range_partials_row_bands_and_combine(fam, nv, dev, kopts):
    for shape in shapes_of(fam):
        H, W = shape
        h = _homs(fam, shape)[:nv]
        P = h.shape[1]
        for kind in KINDS:
            full, pk = _full(kind, shape, P, nv), _packed(kind, shape, P)
            got, want = {}, {}
            for a, b in ((0, P // 3), (P // 3, P), (1, P)):
                want[a, b] = oracle.render_ct(full, h.numpy(), a, b, back=(a == 0))
                got[a, b] = _lib.render_packed_ct(pk, h, a == 0, a, b, out=_sent(nv, H, W, 4))
                match(got[a, b], want[a, b], f"{shape} {kind} ct [{a},{b})")
            band = _sent(nv, H, W, 4)
            _lib.render_packed_ct_rows(pk, h, False, 5, H - 7, band, P // 3, P)
            match(band[:, 5:H - 7], want[P // 3, P][:, 5:H - 7], f"{shape} {kind} rows [5,{H - 7})")
            assert bool((band[:, :5] == SENT).all()) and bool((band[:, H - 7:] == SENT).all()), "other rows touched"
            parts = torch.stack([got[0, P // 3], got[P // 3, P]])
            match(_lib.combine_ct(parts), oracle.combine_ct(np.stack([want[0, P // 3], want[P // 3, P]])),
                  f"{shape} {kind} combine_ct")


# ---------------------------------------------------------------------------
# in-place layout [B, H, W, P, 4]
# ---------------------------------------------------------------------------

PN = 11  # a partial 8-plane chunk
BN = 6   # nonfinite_h's six views


@functools.lru_cache(maxsize=None)
def _native_mpi(kind, shape, P=PN):
    H, W = shape
    m = torch.stack([lc.finite_mpi(H, W, P, seed=b) for b in range(BN)])
    if kind != "finite":
        m = torch.stack([lc.poison(x) for x in m])
    return m


@functools.lru_cache(maxsize=None)
def _native_want(fam, shape, kind, P=PN, p_end=None):
    h = _homs(fam, shape, BN, P).numpy()
    m = _native_mpi(kind, shape, P).numpy()
    if p_end is not None:
        h, m = np.ascontiguousarray(h[:, :p_end]), m[:, :, :, :p_end]
    return oracle.render(m, h)


NATIVE = {"default": None}
NATIVE.update(NATIVE_KERNELS)


@pytest.mark.parametrize("fam", GPU_FAMILIES)
@pytest.mark.parametrize("native", list(NATIVE))
def test_native_layout_kernels(native, fam, dev, kopts):
    """mpiv_render on the default route and with every in-place kernel option."""
    if NATIVE[native] is not None:
        kopts(**NATIVE[native])
    for shape in shapes_of(fam):
        H, W = shape
        h = _homs(fam, shape, BN, PN)
        for kind in KINDS:
            m = _native_mpi(kind, shape).to(dev)
            if native == "default":
                got = _lib.render(m, h)
            else:
                got = _sent(BN, H, W, 3)
                _lib._call("mpiv_render", m, _lib._strides(m), BN, H, W, PN, h.to(dev), got, _lib._stream(dev))
            match(got, _native_want(fam, shape, kind), f"{shape} {kind}")


@pytest.mark.parametrize("P", [PN, 19])
@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_render_train_frames_and_checkpoints(fam, P, dev):
    """render_train: the frames, and checkpoint slot c >= 1 = (the colour of planes [0, 8c), +0) -- the
    fourth channel is written as +0 (render_chunk.hip); slot 0 is never written."""
    for shape in shapes_of(fam):
        h = _homs(fam, shape, BN, P)
        for kind in KINDS:
            m = _native_mpi(kind, shape, P).to(dev)
            out, ck = _lib.render_train(m, h)
            assert ck is not None
            match(out, _native_want(fam, shape, kind, P), f"{shape} {kind} frames")
            for c in range(1, (P + 7) // 8):
                match(ck[:, c, :, :, :3], _native_want(fam, shape, kind, P, 8 * c), f"{shape} {kind} checkpoint {c}")
                assert bool((ck[:, c, :, :, 3].view(torch.int32) == 0).all()), "checkpoint channel 3 is +0"


# ---------------------------------------------------------------------------
# u8 render
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("flight", [0, 2, 8])
@pytest.mark.parametrize("fam", lc.LATTICE + ["edge", "huge", "w_zero"])
def test_u8_render(fam, flight, dev, kopts):
    kopts(u8_flight=flight)
    for shape in shapes_of(fam):
        H, W = shape
        P = planes_of(fam, shape)
        g = torch.Generator().manual_seed(31 + H)
        u8 = torch.randint(0, 256, (H, W, P, 4), generator=g, dtype=torch.uint8)
        pk = _lib.pack_planes_u8(u8.to(dev))
        fl = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)
        for nv in (1, V):
            h = _homs(fam, shape)[:nv]
            got = _lib.render_packed_u8(pk, h, out=_sent(nv, H, W, 3), route_float=False)
            match(got, oracle.render(np.broadcast_to(fl[None], (nv,) + fl.shape), h.numpy()), f"{shape} {nv} views")


# ---------------------------------------------------------------------------
# fused net-output render and the assembly
# ---------------------------------------------------------------------------

NB = 3


@functools.lru_cache(maxsize=None)
def _net(kind, shape, P):
    pred, fg = lc.net_output(NB, shape[0], shape[1], P, kind)
    rgba = oracle.assemble_mpi(pred.numpy(), fg.numpy(), P)
    return pred, fg, rgba


@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_fused_net_output_render(fam, dev):
    """render_net_output and its training forward (frames and checkpoints) on pred / fg holding the
    non-finite pattern, against the oracle's render of the oracle's assembly."""
    P = PN
    for shape in shapes_of(fam, [lc.X_SMALL, lc.Y_SMALL, lc.X_TWO]):
        # three of the six views: nonfinite_h's with two non-finite planes, edge's N+1, N-1 and -2.5
        pick = {"nonfinite_h": [1, 2, 3], "edge": [0, 4, 2]}.get(fam, [0, 1, 2])
        h = _homs(fam, shape, BN, P)[pick]
        for kind in KINDS:
            pred, fg, rgba = _net(kind, shape, P)
            want = oracle.render(rgba, h.numpy())
            match(_lib.render_net_output(pred.to(dev), fg.to(dev), P, h), want, f"{shape} {kind} frames")
            out, ck = _lib.render_net_output_train(pred.to(dev), fg.to(dev), P, h)
            match(out, want, f"{shape} {kind} training frames")
            match(ck[:, 1, :, :, :3], oracle.render(rgba[:, :, :, :8], np.ascontiguousarray(h.numpy()[:, :8])),
                  f"{shape} {kind} checkpoint 1")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [lc.X_SMALL, lc.Y_SMALL, (37, 70)], ids=["65x64", "64x65", "37x70"])
def test_assemble_non_finite(shape, kind, dev):
    P = 5
    pred, fg, rgba = _net(kind, shape, P)
    match(_lib.assemble_mpi(pred.to(dev), fg.to(dev), P), rgba, "assemble_mpi")
    for b in range(NB):
        pk = _lib.assemble_mpi_packed(pred.to(dev), fg.to(dev), P, b)
        match(_lib.unpack_planes(pk), rgba[b], f"assemble_mpi_packed, element {b}")
        H, W = shape
        border = pk.clone()
        border[:, 2:2 + H, 2:2 + W] = 0
        assert bool((border.view(torch.int32) == 0).all()), "the packed border is +0"


@pytest.mark.parametrize("fam", ["edge", "w_zero"])
def test_assemble_sampled_then_backward(fam, dev):
    """mpiv_assemble_mpi_sampled into a NaN-filled buffer, then render_backward: equal to the oracle's
    backward of the whole assembly (a skipped row that a sample reads would show as NaN)."""
    P = PN
    for shape in shapes_of(fam, TWO + [lc.X_SMALL, lc.Y_SMALL]):
        H, W = shape
        h = _homs(fam, shape, BN, P)[:NB]
        pred, fg, rgba = _net("finite", shape, P)
        dout = lc.dout_for((NB, H, W, 3))
        part = torch.full((NB, H, W, P, 4), float("nan"), device=dev)
        p, f = pred.to(dev), fg.to(dev)
        _lib._call("mpiv_assemble_mpi_sampled", p, _lib._strides(p), f, _lib._strides(f), NB, H, W, P, h.to(dev), part,
                   _lib._stream(dev))
        written = ~torch.isnan(part).any(dim=-1)
        assert torch.equal(part[written].view(torch.int32), torch.from_numpy(rgba).to(dev)[written].view(torch.int32))
        want = oracle.render_backward(rgba, h.numpy(), dout.numpy())
        match(_lib.render_backward(part, h, dout.to(dev), check=True), want, f"{shape} sampled assembly")
        match(_lib.render_backward(torch.from_numpy(rgba).to(dev), h, dout.to(dev), check=True), want,
              f"{shape} whole assembly")


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------

BWD_MODES = {"tile": {}, "fallback": {"bwd_fallback": 1}, "miss": {"bwd_margin": -96}}


def _backward_checked(mpi, homs, dout, ckpt, dev):
    """The gradient through a caller-owned workspace, with the abort words checked (no abort)."""
    B, H, W, P, _ = mpi.shape
    L = _lib.load()
    ws = torch.zeros(L.mpiv_render_backward_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    got = _lib.render_backward(mpi, homs, dout, workspace=ws, ckpt=ckpt)
    off = _lib.bwd_flag_offset(H, W, P)
    words = ws[off:off + 20].view(torch.int32).tolist()
    assert words[3] == 0 and words[4] == 0, "the fallback aborted"
    assert _lib.render_backward_status(ws, H, W, P) == 0
    return got


BWD_CASES = [(f, "finite") for f in GPU_FAMILIES] + [("int_shift", "nonfinite"), ("half_shift", "nonfinite")]


@pytest.mark.parametrize("mode", list(BWD_MODES))
@pytest.mark.parametrize("fam,kind", BWD_CASES, ids=[f"{f}-{k}" for f, k in BWD_CASES])
def test_render_backward(fam, kind, mode, dev, kopts):
    """d render / d MPI in the three production modes, with and without checkpoints; signed zeros
    count (on a lattice every second weight is exactly 0, so g * 0 terms are +0 or -0)."""
    if BWD_MODES[mode]:
        kopts(**BWD_MODES[mode])
    for shape in shapes_of(fam):
        H, W = shape
        nb = BN if fam in ("nonfinite_h", "edge") else 2  # (edge: one threshold per view, N-1 among the six)
        h = _homs(fam, shape, BN, PN)[:nb]
        m = _native_mpi(kind, shape)[:nb]
        dout = lc.dout_for((nb, H, W, 3))
        want = oracle.render_backward(m.numpy(), h.numpy(), dout.numpy())
        md = m.to(dev)
        match(_backward_checked(md, h, dout.to(dev), None, dev), want, f"{shape} without checkpoints")
        _, ck = _lib.render_train(md, h)
        match(_backward_checked(md, h, dout.to(dev), ck, dev), want, f"{shape} with checkpoints")


# ---------------------------------------------------------------------------
# plane sweep, inverse warp
# ---------------------------------------------------------------------------

def _sweep_mats(B):
    K = torch.tensor(lc.SWEEP_K)[None].repeat(B, 1, 1)
    return _host.psv_matrices(K, K, lc.sweep_poses()[:B])


# (box_shrink, sweep_direct, sweep_band); sweep_band=1 selects an A/B-only kernel (skipped by the gate)
SWEEP_OPTS = {"default": {}, "shrink3": dict(box_shrink=3), "staged": dict(sweep_direct=-1),
              "staged_shrink3": dict(sweep_direct=-1, box_shrink=3),
              "band": dict(sweep_band=1), "band_staged": dict(sweep_band=1, sweep_direct=-1)}


@functools.lru_cache(maxsize=None)
def _sweep_want(kind, C, D, tgt):
    B = 4
    ki, proj = _sweep_mats(B)
    img = lc.image(B, lc.SWEEP_SRC[0], lc.SWEEP_SRC[1], C, kind)
    return oracle.plane_sweep(img.numpy(), ki.numpy(), proj.numpy(), lc.sweep_depths(D), tgt[0], tgt[1])


@pytest.mark.parametrize("opts", list(SWEEP_OPTS))
@pytest.mark.parametrize("D", [1, 2, 3, 8, 10, 64, 65])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
def test_plane_sweep(C, D, opts, dev, kopts):
    """Exact-lattice source positions (K = [[64,0,32],[0,64,32],[0,0,1]], translations k/64 and k/128),
    inexact and degenerate depths (1/3, 0, -1), raw and padded sources, a wider pixel stride, finite
    and non-finite images, a square and a non-square target."""
    if SWEEP_OPTS[opts]:
        kopts(**SWEEP_OPTS[opts])
    B = 4
    Hs, Ws = lc.SWEEP_SRC
    ki, proj = _sweep_mats(B)
    depths = lc.sweep_depths(D)
    for kind in KINDS:
        img = lc.image(B, Hs, Ws, C, kind).to(dev)
        for tgt in lc.SWEEP_TGT:
            Ht, Wt = tgt
            want = _sweep_want(kind, C, D, tgt)
            match(_lib.plane_sweep(img, depths, ki, proj, Ht, Wt), want, f"{kind} {tgt} raw")
            if C <= 4:
                match(_lib.plane_sweep_padded(img, depths, ki, proj, Ht, Wt), want, f"{kind} {tgt} padded")
            if C > 4:
                continue
            pst = D * C + 5  # mpiv_plane_sweep_into with a wider pixel stride: the gaps stay untouched
            wide = _sent(B, Ht, Wt, pst)
            _lib._call("mpiv_plane_sweep_into", img, _lib._strides(img), B, Hs, Ws, C, ki.to(dev), proj.to(dev),
                       _lib._depths_on(depths, torch.device(DEV)), D, Ht, Wt, wide[..., 2:], Ht * Wt * pst, pst,
                       _lib._stream(torch.device(DEV)))
            match(wide[..., 2:2 + D * C], want, f"{kind} {tgt} into a wider stride")
            assert bool((wide[..., :2] == SENT).all()) and bool((wide[..., 2 + D * C:] == SENT).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1, 3, 4, 5])
def test_inverse_warp_degenerate_depth_map(C, kind, dev):
    """A depth map holding 0, a negative value, Inf and NaN."""
    B = 4
    Hs, Ws = lc.SWEEP_SRC
    ki, proj = _sweep_mats(B)
    img = lc.image(B, Hs, Ws, C, kind)
    dmap = lc.degenerate_depth_map(B, Hs, Ws)
    want = oracle.inverse_warp(img.numpy(), ki.numpy(), proj.numpy(), dmap.numpy())
    assert 0 < lc.nan_share(want) < 0.5
    match(_lib.inverse_warp_depthmap(img.to(dev), dmap.to(dev), ki, proj, Hs, Ws), want, "inverse warp")


# ---------------------------------------------------------------------------
# grid_sample primitive, over_composite
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C", [1, 3, 4, 6])
def test_bilinear_sample_boundary_coordinates(C, channels_last, dev):
    Hi, Wi = 8, 16
    img = torch.cat([lc.image(1, Hi, Wi, C, "finite"), lc.image(1, Hi, Wi, C, "nonfinite")])
    coords = lc.boundary_coords(2, Hi, Wi)
    want = oracle.grid_sample_nchw(img.numpy().transpose(0, 3, 1, 2), coords.numpy(), channels_last)
    assert 0 < lc.nan_share(want) < 0.6
    match(_lib.bilinear_sample(img.to(dev), coords.to(dev), channels_last), want, "bilinear_sample")


@pytest.mark.parametrize("P", [1, 2, 5])
def test_over_composite_non_finite_layers(P, dev):
    H, W = 33, 70
    layers = lc.nonfinite_mpi(H, W, max(P, 3))[:, :, :P].permute(2, 0, 1, 3).contiguous()
    layers[:, 3, 3, 3] = 0.0   # alpha exactly 0 and 1 next to the Inf / NaN texels
    layers[:, 4, 4, 3] = 1.0
    layers[:, 3:5, 0, 3] = torch.tensor([0.0, 1.0])[None, :]
    want = oracle.over_composite(layers.numpy())
    if P > 1:
        assert lc.nan_share(want) > 0
    match(_lib.over_composite([layers[i].to(dev) for i in range(P)]), want, "over_composite")
