"""GPU parity of the half-precision RGBA MPI render (render_f16.hip): rendering an fp16 MPI is
defined as rendering mpi.float(), so frames from packed 8-byte texels must equal the CPU oracle and
the fp32 kernels on the float copy BIT FOR BIT -- for every half value through pack / unpack, every
instantiation the dispatcher can choose, the (C, T) partials, the exact-lattice and non-finite view
families and the drop-in wrapper."""
import numpy as np
import pytest
import torch

import lattice_cases as lc
from conftest import assert_bits, load_test_mpi
from test_lattice_gpu import GPU_FAMILIES, SENT, V as LATTICE_V, _homs as lattice_homs, planes_of, shapes_of
from test_render_colsep_gpu import SQ, VMAX, _homs as colsep_homs
from test_render_order_gpu import P as ORDER_P, _homs as order_homs
from test_u8_gpu import _extreme_case

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib  # noqa: E402
from mpi_vision_amd import utils as mvu  # noqa: E402
from oracle import oracle  # noqa: E402

SPECIALS = np.array([0x0001, 0x03FF, 0x8001, 0x83FF, 0x0200, 0x8000, 0x7BFF, 0xFBFF], np.uint16)


def _half_mpi(H, W, P, seed):
    """[H,W,P,4] float16: rgb uniform in [-1, 1), alpha in [0, 1], rounded to half; about 1 % of the
    channels overwritten with subnormal halves, -0 and +-65504; plane 0 alpha 1.  All finite."""
    rng = np.random.default_rng(seed)
    x = rng.random((H, W, P, 4), dtype=np.float32)
    x[..., :3] = x[..., :3] * 2 - 1
    h = x.astype(np.float16)
    flat = h.reshape(-1).view(np.uint16)
    idx = rng.choice(flat.size, size=flat.size // 100, replace=False)
    flat[idx] = SPECIALS[rng.integers(0, len(SPECIALS), size=idx.size)]
    h[:, :, 0, 3] = 1.0
    assert np.isfinite(h.astype(np.float32)).all()
    return h


def _oracle(h, homs):
    V = homs.shape[0]
    want = oracle.render(np.broadcast_to(h.astype(np.float32)[None], (V,) + h.shape).copy(), homs.numpy())
    assert np.isfinite(want).all()  # the texels are finite and sparse enough in +-65504
    return want


def _f16(packed, homs, out=None):
    """The f16 KERNEL at any view count (render_packed_f16 alone sends launches of >= F16_FLOAT_MIN_VIEWS
    views to the float kernel on the float copy: test_float_route_many_views)."""
    return _lib.render_packed_f16(packed, homs, out=out, route_float=False)


def _check_render(h, homs, dev, route=None, float_path=True):
    """The f16 kernel == oracle.render(x.float()) == render_packed(pack_planes(x.float()))."""
    H, W, P, _ = h.shape
    V = homs.shape[0]
    if route is not None:
        assert _lib.route("render_packed_f16", H, W, P, V)[0] == f"render_f16_kernel<false, {route}>"
    want = _oracle(h, homs)
    t = torch.from_numpy(h).to(dev)
    out = torch.full((V, H, W, 3), SENT, device=dev)
    _f16(_lib.pack_planes_f16(t), homs, out=out)
    assert_bits(out, want, "f16 kernel vs oracle")
    if float_path:
        assert_bits(_lib.render_packed(_lib.pack_planes(t.float()), homs), want, "float path")


# ---------------------------------------------------------------------------
# 1, 2: pack / unpack
# ---------------------------------------------------------------------------

def test_every_half_value_packs_and_unpacks_exactly(dev):
    """All 65536 bit patterns (subnormals, +-0, +-inf, 65504, every NaN) through pack + unpack: the
    packed float MPI of x.float(), bit for bit where it is no NaN, NaN where it is; border +0."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    np.random.default_rng(16).shuffle(bits)
    v_np = bits.view(np.float16).reshape(64, 64, 4, 4)
    pk = _lib.pack_planes_f16(torch.from_numpy(v_np).to(dev))
    assert pk.dtype == torch.float16 and tuple(pk.shape) == (4, 68, 68, 4)
    got = _lib.unpack_planes_f16(pk).cpu().numpy()
    want = _lib.pack_planes(torch.from_numpy(v_np.astype(np.float32)).to(dev)).cpu().numpy()
    lc.match(got, want, "unpack(pack(every half))")
    assert np.isnan(want).sum() == 2 * 1023  # the NaN patterns were really there
    border = np.ones((68, 68), bool)
    border[2:66, 2:66] = False
    assert (got[:, border].view(np.uint32) == 0).all(), "border is +0"
    assert (pk.cpu().numpy().view(np.uint16)[:, border] == 0).all(), "packed border is +0"


def test_pack_layout_and_strides(dev):
    """pack_planes_f16 = plane-major RGBA texels inside a zero border, for a strided view (the
    channel-contiguous 8-B read path and, on a channel-strided view, the per-channel one)."""
    rng = np.random.default_rng(2)
    big = rng.integers(0, 0x7C00, size=(9, 21, 6, 5), dtype=np.uint16).view(np.float16)  # finite, distinct bits
    tb = torch.from_numpy(big).to(dev)
    for view, ref in ((tb[1:8, 2:19, 1:5, :4], big[1:8, 2:19, 1:5, :4]),    # channel stride 1, odd strides
                      (tb[1:8, 2:19, 1:5, 1:], big[1:8, 2:19, 1:5, 1:]),    # texels never 8-B aligned as a whole
                      (tb[1:8, 2:19, :4].permute(0, 1, 3, 2),               # channel stride != 1 (5 planes)
                       big[1:8, 2:19, :4].transpose(0, 1, 3, 2))):
        Hh, Ww, Pp, _ = ref.shape
        want = np.zeros((Pp, Hh + 4, Ww + 4, 4), np.uint16)
        want[:, 2:2 + Hh, 2:2 + Ww] = np.ascontiguousarray(ref).view(np.uint16).transpose(2, 0, 1, 3)
        got = _lib.pack_planes_f16(view).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want)
    out = torch.empty((4, 11, 21, 4), dtype=torch.float16, device=dev)
    assert _lib.pack_planes_f16(tb[1:8, 2:19, 1:5, :4], out=out) is out
    with pytest.raises(RuntimeError, match="out must be"):
        _lib.pack_planes_f16(tb[1:8, 2:19, 1:5, :4], out=out.float())


# ---------------------------------------------------------------------------
# 3: render against the oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(70, 150, 9), (37, 203, 7), (64, 66, 16)])
def test_render_vs_oracle(shape, dev):
    """Odd sizes, partial tiles, rotations up to +-17 degrees, planes partly behind the camera."""
    H, W, P = shape
    _, homs = _extreme_case(7, H, W, P, seed=H * W + P)
    _check_render(_half_mpi(H, W, P, H + W + P), homs, dev)


# ---------------------------------------------------------------------------
# 4: every instantiation the dispatcher chooses
# ---------------------------------------------------------------------------

def _tiled_homs(V, H, W, P, seed):
    _, homs = _extreme_case(8, H, W, P, seed=seed)
    return homs[torch.arange(V) % 8].contiguous()


# (shape, views, template arguments after CT): 2 plain rows (stretched, small launch); 4 rows with
# vertical reuse and 4 in flight (near-square, under 2048 blocks); 2 in flight from 2048 blocks up --
# near-square at 1024 views of 1 x 2 tiles, and stretched (landscape) at 1024 views of 1 x 2 tiles of
# 64 x 32 (2048 of them: the launch fills the chip)
ROUTES = [((37, 203, 7), 7, "2, false, 2"), ((64, 66, 16), 7, "4, true, 4"), ((20, 18, 3), 1024, "4, true, 2"),
          ((36, 64, 2), 1024, "4, true, 2")]
ROUTE_IDS = ["plain2", "reuse_flight4", "reuse_flight2", "reuse_flight2_stretched"]


@pytest.mark.parametrize("shape,V,route", ROUTES, ids=ROUTE_IDS)
def test_routes(shape, V, route, dev):
    H, W, P = shape
    _check_render(_half_mpi(H, W, P, 5 + H), _tiled_homs(V, H, W, P, 77 + H), dev, route=route)


@pytest.mark.parametrize("shape,V,route", ROUTES[1:3], ids=ROUTE_IDS[1:3])
def test_routes_ct(shape, V, route, dev):
    """The (C, T) instantiations of the reuse kernels (test_ct_partials runs the plain-rows one)."""
    H, W, P = shape
    assert _lib.route("render_packed_f16_ct", H, W, P, V)[0] == f"render_f16_kernel<true, {route}>"
    h = _half_mpi(H, W, P, 6 + H)
    homs = _tiled_homs(V, H, W, P, 78 + H)
    full = np.broadcast_to(h.astype(np.float32)[None], (V,) + h.shape).copy()
    pk = _lib.pack_planes_f16(torch.from_numpy(h).to(dev))
    for a, b, back in ((0, P, True), (1, P, False)):
        ct = _lib.render_packed_f16_ct(pk, homs, back=back, p_begin=a, p_end=b)
        assert_bits(ct, oracle.render_ct(full, homs.numpy(), a, b, back=back), f"ct [{a},{b})")


def test_float_route_many_views(dev):
    """Launches of >= F16_FLOAT_MIN_VIEWS views (40 here) render the MPI's exact float copy with the
    float kernel: the oracle's frames and the f16 kernel's; the copy is made once per MPI (memo),
    again after an in-place edit or a refill through pack_planes_f16(out=), and released by
    clear_float_copies (one entry per device, shared with the u8 MPIs' copies)."""
    H, W, P, V = 37, 203, 7, 40
    assert V >= _lib.F16_FLOAT_MIN_VIEWS
    h = _half_mpi(H, W, P, 40)
    homs = _tiled_homs(V, H, W, P, 41)
    want = _oracle(h, homs)
    t = torch.from_numpy(h).to(dev)
    pk = _lib.pack_planes_f16(t)
    _lib.clear_float_copies()
    assert_bits(_lib.render_packed_f16(pk, homs), want, "automatic route at 40 views")
    assert dev in _lib._U8_FLOAT, "40 views took the float route"
    f1 = _lib.f16_float_copy(pk)
    assert _lib.f16_float_copy(pk) is f1  # memoised
    assert_bits(f1, _lib.pack_planes(t.float()).cpu().numpy(), "the float copy is the packed float MPI")
    assert_bits(_lib.render_packed_f16(pk, homs, route_float=True), want, "float route")
    _lib.clear_float_copies(dev)
    assert_bits(_lib.render_packed_f16(pk, homs, route_float=False), want, "f16 kernel")
    assert_bits(_lib.render_packed_f16(pk, homs[:7]), want[:7], "7 views: the f16 kernel")
    assert dev not in _lib._U8_FLOAT, "few views and route_float=False make no copy"
    f1 = _lib.f16_float_copy(pk)
    pk[1:, 2:-2, 2:-2, :3] *= 0.5  # in place: a new copy, new frames
    assert _lib.f16_float_copy(pk) is not f1
    c = _lib.render_packed_f16(pk, homs, route_float=True)
    assert_bits(c, _lib.render_packed_f16(pk, homs, route_float=False).cpu().numpy(), "after an in-place edit")
    assert not np.array_equal(c.cpu().numpy(), want)
    f2 = _lib.f16_float_copy(pk)
    _lib.pack_planes_f16(t, out=pk)  # a ctypes write: the memo must see it
    assert _lib.f16_float_copy(pk) is not f2
    assert_bits(_lib.render_packed_f16(pk, homs, route_float=True), want, "after a refill")
    u8 = _lib.synth_mpi_packed_u8(1, 16, 70, 0, 3, dev)  # the u8 copies share the one entry per device
    fu = _lib.u8_float_copy(u8)
    assert _lib._U8_FLOAT[dev][2] is fu and _lib.u8_float_copy(u8) is fu
    with pytest.raises(RuntimeError, match="float16"):
        _lib.f16_float_copy(u8)
    with pytest.raises(RuntimeError):
        _lib.u8_float_copy(pk)
    del f1, f2, fu, u8
    assert dev not in _lib._U8_FLOAT  # dropped with its MPI
    _lib.clear_float_copies()


def test_landscape_stretch(dev):
    """W > H: the reference's swapped normalisation stretches the sample grid."""
    H, W, P = 36, 64, 8
    _, homs = _extreme_case(3, H, W, P, seed=11)
    _check_render(_half_mpi(H, W, P, 9), homs, dev, route="2, false, 2")


@pytest.mark.parametrize("kind", ["sway", "pitch"])
@pytest.mark.parametrize("V,route", [(1, "4, true, 4"), (40, "4, true, 4"), (147, "4, true, 2")])
def test_render_colsep(V, route, kind, dev, kopts):
    """The column-separable issue path (render_colsep 0: automatic, -1: off) of the f16 kernel with 4
    rows in flight (1 and 40 views: 14 and 560 blocks) and with 2 (147 views: 2058 blocks): the same
    frames, equal to the float render of x.float()."""
    H, W, P = SQ
    assert _lib.route("render_packed_f16", H, W, P, V)[0] == f"render_f16_kernel<false, {route}>"
    homs = colsep_homs(kind, SQ)
    homs = torch.cat([homs] * -(-V // VMAX))[:V]
    h = _half_mpi(H, W, P, 3)
    t = torch.from_numpy(h).to(dev)
    pk = _lib.pack_planes_f16(t)
    want = _lib.render_packed(_lib.pack_planes(t.float()), homs).cpu().numpy()
    got = {}
    for cs in (0, -1):
        kopts(render_colsep=cs)
        got[cs] = _f16(pk, homs).cpu().numpy()
    assert_bits(got[0], got[-1], "render_colsep 0 vs -1")
    assert_bits(got[0], want, "f16 vs the float render of x.float()")
    if V == 1:
        assert_bits(got[0], _oracle(h, homs), "f16 vs oracle")


@pytest.mark.parametrize("V", [3, 40])
@pytest.mark.parametrize("hw", [(136, 200), (40, 70), (150, 160)], ids=["136x200", "40x70", "150x160"])
def test_render_order(hw, V, dev, kopts):
    """Both tile orders (render_order -1: bands, 1: interleaved) of the f16 kernel equal the oracle;
    150 x 160 takes the reuse kernel, the others two plain rows."""
    H, W = hw
    vs = "4, true, 4" if hw == (150, 160) else "2, false, 2"
    assert _lib.route("render_packed_f16", H, W, ORDER_P, V)[0] == f"render_f16_kernel<false, {vs}>"
    h = _half_mpi(H, W, ORDER_P, 3 + H)
    homs = order_homs(hw, V)
    want = _oracle(h, homs)
    pk = _lib.pack_planes_f16(torch.from_numpy(h).to(dev))
    for order in (-1, 1):
        kopts(render_order=order)
        out = torch.full((V, H, W, 3), float("nan"), device=dev)
        _f16(pk, homs, out=out)
        assert_bits(out, want, f"render_order={order}")


# ---------------------------------------------------------------------------
# 5: (C, T) partials
# ---------------------------------------------------------------------------

def test_ct_partials(dev):
    """Plane-range (C, T) partials equal the oracle's; their ordered combine equals the sequential
    render within the project's 1e-5."""
    H, W, P, V = 45, 130, 11, 4
    _, homs = _extreme_case(V, H, W, P, seed=5)
    rng = np.random.default_rng(45)
    x = rng.random((H, W, P, 4), dtype=np.float32)
    x[..., :3] = x[..., :3] * 2 - 1
    h = x.astype(np.float16)  # no +-65504 here: the 1e-5 bound is absolute
    h[:, :, 0, 3] = 1.0
    full = np.broadcast_to(h.astype(np.float32)[None], (V,) + h.shape).copy()
    assert _lib.route("render_packed_f16_ct", H, W, P, V)[0] == "render_f16_kernel<true, 2, false, 2>"
    pk = _lib.pack_planes_f16(torch.from_numpy(h).to(dev))
    parts = []
    for a, b in zip([0, 3, 8], [3, 8, P]):
        ct = _lib.render_packed_f16_ct(pk, homs, back=(a == 0), p_begin=a, p_end=b)
        assert_bits(ct, oracle.render_ct(full, homs.numpy(), a, b, back=(a == 0)), f"ct [{a},{b})")
        parts.append(ct)
    got = _lib.combine_ct(torch.stack(parts)).cpu().numpy()
    np.testing.assert_allclose(got, oracle.render(full, homs.numpy()), rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------
# 6: lattice and non-finite geometry
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_lattice_and_nonfinite_views(fam, dev):
    """Exact-lattice positions, dead-tile thresholds, huge / w == 0 / non-finite homographies: the f16
    kernel's frames (at 1 and 12 views) equal the fp32 kernel's frames of x.float() (NaN positions there, bits elsewhere)."""
    for shape in shapes_of(fam):
        H, W = shape
        P = planes_of(fam, shape)
        t = lc.finite_mpi(H, W, P).half().to(dev)
        pk, pf = _lib.pack_planes_f16(t), _lib.pack_planes(t.float())
        for nv in (1, LATTICE_V):
            hm = lattice_homs(fam, shape)[:nv]
            got = _f16(pk, hm, out=torch.full((nv, H, W, 3), SENT, device=dev))
            want = _lib.render_packed(pf, hm, out=torch.full((nv, H, W, 3), SENT, device=dev))
            lc.match(got, want, f"{fam} {shape} {nv} views")


# ---------------------------------------------------------------------------
# 7: drop-in
# ---------------------------------------------------------------------------

def test_drop_in_reference_test_mpi(large, dev):
    """mpi_render_view_f16 on the reference's 10-plane test MPI rounded to half, at the two golden
    config-1 poses: the oracle on x.float(), mpi_render_view_torch(x.float()), and the per-view path."""
    x = load_test_mpi().half()  # [1,400,640,10,4]
    pose, K, depths = (torch.tensor(large[k]) for k in ("c1_pose", "c1_K", "c1_depths"))
    homs = _host.render_homographies(pose, depths, K, 2)
    want = oracle.render(np.broadcast_to(x.float().numpy(), (2,) + tuple(x.shape[1:])).copy(),
                         homs.reshape(2, 10, 9).numpy())
    xd, pd, Kd, dd = x.to(dev), pose.to(dev), K.to(dev), depths.to(dev)
    out = mvu.mpi_render_view_f16(xd.expand(2, *x.shape[1:]), pd, dd, Kd)
    assert out.dtype == torch.float32
    assert_bits(out, want, "stride-0 batch vs oracle")
    ref = mvu.mpi_render_view_torch(xd.float().expand(2, *x.shape[1:]), pd, dd, Kd)
    assert_bits(out, ref.cpu().numpy(), "vs mpi_render_view_torch(x.float())")
    per = mvu.mpi_render_view_f16(xd.repeat(2, 1, 1, 1, 1), pd, dd, Kd)  # non-broadcast: packs per view
    assert_bits(per, want, "per-view path")
    # more views of a stride-0 batch: still the f16 kernel (the packed MPI is a temporary: a float copy
    # would serve this one launch, and pays only from F16_FLOAT_ONCE_MIN_VIEWS views)
    _lib.clear_float_copies()
    V = 2 * _lib.F16_FLOAT_MIN_VIEWS
    assert V < _lib.F16_FLOAT_ONCE_MIN_VIEWS
    many = mvu.mpi_render_view_f16(xd.expand(V, *x.shape[1:]), pd[torch.arange(V) % 2], dd, Kd[torch.arange(V) % 2])
    assert_bits(many, want[np.arange(V) % 2], f"{V} views of the golden poses")
    assert dev not in _lib._U8_FLOAT
    V = _lib.F16_FLOAT_ONCE_MIN_VIEWS  # from here the copy pays even for one launch: the float route
    many = mvu.mpi_render_view_f16(xd.expand(V, *x.shape[1:]), pd[torch.arange(V) % 2], dd, Kd[torch.arange(V) % 2])
    assert_bits(many, want[np.arange(V) % 2], f"{V} views of the golden poses (float route)")
    del many
    _lib.clear_float_copies()
    with pytest.raises(RuntimeError, match="float16"):
        mvu.mpi_render_view_f16(xd.float(), pd[:1], dd, Kd[:1])
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        mvu.mpi_render_view_torch(xd, pd[:1], dd, Kd[:1])  # the fp32 entry keeps refusing half input
