"""GPU parity of the alpha-only plane-colour render (render_texel.hip, the TexA32 format): compositing
one constant colour per plane through an MPI's alpha is defined as rendering the float MPI whose RGB
is that colour all over the plane, so frames from the packed 4-byte alpha planes must equal the CPU
oracle and the fp32 kernel on that constructed MPI BIT FOR BIT -- through the pack, every instantiation
the dispatcher can choose, both tile orders, the column-separable issue, the exact-lattice and
non-finite view families, non-finite colours, the drop-in wrappers (goldens of the reference), their
memory footprint and autograd rule, a side stream and a captured graph."""
import hashlib

import numpy as np
import pytest
import torch

import lattice_cases as lc
import planecolor_cases as pc
from conftest import assert_bits, load_test_mpi
from test_lattice_gpu import GPU_FAMILIES, SENT, V as LATTICE_V, _homs as lattice_homs, planes_of, shapes_of
from test_render_colsep_gpu import SQ, VMAX, _homs as colsep_homs
from test_render_order_gpu import P as ORDER_P, _homs as order_homs
from test_u8_gpu import _extreme_case

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib  # noqa: E402
from mpi_vision_amd import utils as mvu  # noqa: E402
from oracle import oracle  # noqa: E402


def _alpha(H, W, P, seed):
    """[H,W,P] float32 in [0, 1) with exact 0 and 1 sprinkled in (the back plane's alpha is left
    random: it counts as 1 whatever it holds)."""
    rng = np.random.default_rng(seed)
    a = rng.random((H, W, P), dtype=np.float32)
    pick = rng.random((H, W, P))
    a[pick < 0.05] = 0.0
    a[pick > 0.95] = 1.0
    return a


def _colors(P, seed):
    """[P,3] random signed colours; one -0.0 and one 65504 entry."""
    c = (np.random.default_rng(seed).random((P, 3), dtype=np.float32) * 4 - 2).astype(np.float32)
    c[1 % P, 0] = -0.0
    c[(P - 1) // 2, 1] = 65504.0
    return c


def _oracle(alpha, colors, homs):
    V = homs.shape[0]
    mpi = pc.constructed(alpha, colors)
    want = oracle.render(np.broadcast_to(mpi[None], (V,) + mpi.shape).copy(), homs.numpy())
    assert np.isfinite(want).all()
    return want


def _render(alpha, colors, homs, dev, fill=SENT):
    H, W, P = alpha.shape
    pk = _lib.pack_planes_alpha(torch.from_numpy(alpha).to(dev)[..., None])
    out = torch.full((homs.shape[0], H, W, 3), fill, device=dev)
    assert _lib.render_packed_alpha(pk, torch.from_numpy(colors), homs, out=out) is out
    return out


def _float_render(alpha, colors, homs, dev):
    """The parent's way to the same frame: the float kernel on the packed constructed MPI."""
    return _lib.render_packed(_lib.pack_planes(torch.from_numpy(pc.constructed(alpha, colors)).to(dev)), homs)


def _check_render(alpha, colors, homs, dev, route=None, float_path=True):
    H, W, P = alpha.shape
    if route is not None:
        assert _lib.route("render_packed_alpha", H, W, P, homs.shape[0])[0] == pc.kernel_name(route)
    want = _oracle(alpha, colors, homs)
    assert_bits(_render(alpha, colors, homs, dev), want, "alpha kernel vs oracle")
    if float_path:
        assert_bits(_float_render(alpha, colors, homs, dev), want, "float path")


# ---------------------------------------------------------------------------
# 1: pack
# ---------------------------------------------------------------------------

def test_pack_layout_and_strides(dev):
    """pack_planes_alpha = the view's last channel, plane-major inside a +0 border: channel 3 of a
    strided view at odd offsets, a channel-strided permuted view, a [H,W,P,1] tensor; out= reused."""
    rng = np.random.default_rng(2)
    big = rng.integers(1, 0x7F800000, size=(9, 21, 6, 5), dtype=np.uint32).view(np.float32)  # distinct non-zero bits
    tb = torch.from_numpy(big).to(dev)
    for view, ref in ((tb[1:8, 2:19, 1:5, 1:], big[1:8, 2:19, 1:5, 4]),       # [7,17,4,4]: channel 3 at odd offsets
                      (tb[1:8, 2:19, :4].permute(0, 1, 3, 2),                 # channel stride != 1 (5 planes)
                       big[1:8, 2:19, 3]),
                      (tb[1:8, 2:19, 1:5, 2:3], big[1:8, 2:19, 1:5, 2]),      # [H,W,P,1], strided
                      (tb[1:8, 2:19, 1:5, 2:3].contiguous(), big[1:8, 2:19, 1:5, 2])):
        Hh, Ww, Pp = ref.shape
        want = np.zeros((Pp, Hh + 4, Ww + 4), np.uint32)
        want[:, 2:2 + Hh, 2:2 + Ww] = np.ascontiguousarray(ref).view(np.uint32).transpose(2, 0, 1)
        got = _lib.pack_planes_alpha(view)
        assert got.dtype == torch.float32 and tuple(got.shape) == (Pp, Hh + 4, Ww + 4)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)  # layout, and a +0 border
    view = tb[1:8, 2:19, 1:5, 1:]
    out = torch.full((4, 11, 21), SENT, device=dev)
    assert _lib.pack_planes_alpha(view, out=out) is out
    first = out.clone()
    out.fill_(SENT)
    assert _lib.pack_planes_alpha(view, out=out) is out and torch.equal(out, first)  # border rewritten too
    for bad in (out.double(), torch.empty((4, 11, 22), device=dev), torch.empty((4, 11, 42), device=dev)[..., ::2]):
        with pytest.raises(RuntimeError, match="out must be"):
            _lib.pack_planes_alpha(view, out=bad)
    with pytest.raises(RuntimeError, match=r"\[H, W, P, 4\] or \[H, W, P, 1\]"):
        _lib.pack_planes_alpha(tb[1:8, 2:19, 1:5, :3])
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        _lib.pack_planes_alpha(view.half())


# ---------------------------------------------------------------------------
# 2: render against the oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(70, 150, 9), (37, 203, 7), (64, 66, 16)])
def test_render_vs_oracle(shape, dev):
    """Odd sizes, partial tiles, rotations up to +-17 degrees, planes partly behind the camera; random
    signed colours with a -0.0 and a 65504."""
    H, W, P = shape
    _, homs = _extreme_case(7, H, W, P, seed=H * W + P)
    _check_render(_alpha(H, W, P, H + W + P), _colors(P, P), homs, dev)


def test_not_colour_times_coverage(dev):
    """The definition's consequence: where taps leave the plane the frame differs from colour x
    coverage (so the kernel may not factorise), and equals the oracle."""
    H, W, P = 40, 72, 1
    _, homs = _extreme_case(4, H, W, 2, seed=5)
    homs = homs.reshape(4, 2, 9)[:, 1:].contiguous()  # the near plane's homographies, as a one-plane MPI's
    alpha = _alpha(H, W, P, 1)
    colors = np.array([[0.3, -1.7, 1.0]], np.float32)
    got = _render(alpha, colors, homs, dev).cpu().numpy()
    assert_bits(got, _oracle(alpha, colors, homs), "one plane")
    assert (got[..., 0] != np.float32(0.3) * got[..., 2]).any()


# ---------------------------------------------------------------------------
# 3: every instantiation the dispatcher chooses
# ---------------------------------------------------------------------------

def _tiled_homs(V, H, W, P, seed):
    _, homs = _extreme_case(8, H, W, P, seed=seed)
    return homs[torch.arange(V) % 8].contiguous()


@pytest.mark.parametrize("shape,V,route", pc.ROUTES, ids=pc.ROUTE_IDS)
def test_routes(shape, V, route, dev):
    H, W, P = shape
    _check_render(_alpha(H, W, P, 5 + H), _colors(P, 6 + H), _tiled_homs(V, H, W, P, 77 + H), dev, route=route)


def test_landscape_stretch(dev):
    """W > H: the reference's swapped normalisation stretches the sample grid."""
    H, W, P = 36, 64, 8
    _, homs = _extreme_case(3, H, W, P, seed=11)
    _check_render(_alpha(H, W, P, 9), _colors(P, 10), homs, dev, route="2, false, 2")


@pytest.mark.parametrize("V", [3, 40])
@pytest.mark.parametrize("hw", [(136, 200), (150, 160)], ids=["136x200", "150x160"])
def test_render_order(hw, V, dev, kopts):
    """Both tile orders (render_order -1: bands, 1: interleaved) equal the oracle; 150 x 160 takes the
    reuse kernel, 136 x 200 two plain rows."""
    H, W = hw
    route = "4, true, 4" if hw == (150, 160) else "2, false, 2"
    assert _lib.route("render_packed_alpha", H, W, ORDER_P, V)[0] == pc.kernel_name(route)
    alpha, colors = _alpha(H, W, ORDER_P, 3 + H), _colors(ORDER_P, 4 + H)
    homs = order_homs(hw, V)
    want = _oracle(alpha, colors, homs)
    for order in (-1, 1):
        kopts(render_order=order)
        assert_bits(_render(alpha, colors, homs, dev, fill=float("nan")), want, f"render_order={order}")


@pytest.mark.parametrize("kind", ["sway", "pitch"])
@pytest.mark.parametrize("V,route", [(1, "4, true, 4"), (40, "4, true, 4"), (147, "4, true, 2")])
def test_render_colsep(V, route, kind, dev, kopts):
    """The column-separable issue path (render_colsep 0: automatic, -1: off) with 4 rows in flight (1
    and 40 views) and with 2 (147 views: 2058 blocks): the same frames, equal to the float render of
    the constructed MPI (sway views are separable, pitch views are not)."""
    H, W, P = SQ
    assert _lib.route("render_packed_alpha", H, W, P, V)[0] == pc.kernel_name(route)
    homs = colsep_homs(kind, SQ)
    homs = torch.cat([homs] * -(-V // VMAX))[:V]
    alpha, colors = _alpha(H, W, P, 3), _colors(P, 4)
    want = _float_render(alpha, colors, homs, dev).cpu().numpy()
    got = {}
    for cs in (0, -1):
        kopts(render_colsep=cs)
        got[cs] = _render(alpha, colors, homs, dev).cpu().numpy()
    assert_bits(got[0], got[-1], "render_colsep 0 vs -1")
    assert_bits(got[0], want, "alpha kernel vs the float render of the constructed MPI")
    if V == 1:
        assert_bits(got[0], _oracle(alpha, colors, homs), "alpha kernel vs oracle")


# ---------------------------------------------------------------------------
# 4: lattice and non-finite geometry, non-finite colours
# ---------------------------------------------------------------------------

def _lattice_check(fam, colors_of, dev):
    for shape in shapes_of(fam):
        H, W = shape
        P = planes_of(fam, shape)
        alpha = lc.finite_mpi(H, W, P)[..., 3].contiguous().numpy()
        colors = colors_of(P)
        pk = _lib.pack_planes_alpha(torch.from_numpy(alpha).to(dev)[..., None])
        pf = _lib.pack_planes(torch.from_numpy(pc.constructed(alpha, colors)).to(dev))
        for nv in (1, LATTICE_V):
            hm = lattice_homs(fam, shape)[:nv]
            got = _lib.render_packed_alpha(pk, torch.from_numpy(colors), hm,
                                           out=torch.full((nv, H, W, 3), SENT, device=dev))
            want = _lib.render_packed(pf, hm, out=torch.full((nv, H, W, 3), SENT, device=dev))
            lc.match(got, want, f"{fam} {shape} {nv} views")


@pytest.mark.parametrize("fam", GPU_FAMILIES)
def test_lattice_and_nonfinite_views(fam, dev):
    """Exact-lattice positions, dead-tile thresholds, huge / w == 0 / non-finite homographies: the
    alpha kernel's frames (at 1 and 12 views) equal the fp32 kernel's frames of the constructed MPI
    (NaN positions there, bits elsewhere)."""
    _lattice_check(fam, lambda P: _colors(P, 21), dev)


@pytest.mark.parametrize("fam", ["half_shift", "edge"])
def test_nonfinite_colors(fam, dev):
    """An Inf and a NaN colour propagate as they do in the float render: Inf x a zero weight is NaN
    there and here, and a tap outside the plane is 0, not the colour."""
    def colors_of(P):
        c = _colors(P, 22)
        c[0, 2] = np.inf
        c[P - 1, 0] = np.nan
        c[1 % P, 1] = -np.inf
        return c

    _lattice_check(fam, colors_of, dev)


# ---------------------------------------------------------------------------
# 5: drop-ins
# ---------------------------------------------------------------------------

def _golden_inputs(name, dev):
    g = pc.golden()
    return {k: torch.tensor(g[f"{name}_{k}"]).to(dev) for k in ("alpha", "colors", "pose", "K", "depths")}


def test_drop_in_goldens(dev):
    """The reference's frames: `pa` (B = 2, colours (1/d, d, 1)) from a [B,H,W,P,4] MPI whose RGB is
    junk, through both wrappers and with host poses; `pb` (signed colours, a -0.0) from a [B,H,W,P,1]
    tensor."""
    g = pc.golden()
    t = _golden_inputs("pa", dev)
    rgba = torch.cat([torch.full(t["alpha"].shape + (3,), float("nan"), device=dev), t["alpha"][..., None]], -1)
    assert_bits(mvu.mpi_render_plane_colors_torch(rgba, t["colors"], t["pose"], t["depths"], t["K"]), g["pa_out"], "pa")
    assert_bits(mvu.mpi_render_depth_torch(rgba, t["pose"], t["depths"], t["K"]), g["pa_out"], "pa, depth wrapper")
    assert_bits(mvu.mpi_render_depth_torch(rgba, t["pose"].cpu(), t["depths"].cpu(), t["K"].cpu()), g["pa_out"],
                "pa, host cameras")
    t = _golden_inputs("pb", dev)
    out = mvu.mpi_render_plane_colors_torch(t["alpha"][..., None], t["colors"].cpu(), t["pose"], t["depths"], t["K"])
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 37, 53, 3)
    assert_bits(out, g["pb_out"], "pb")


def test_drop_in_reference_test_mpi(large, dev):
    """mpi_render_depth_torch on the reference's 10-plane test MPI at the two golden config-1 poses:
    the reference's frame (sha256 and centre crop); a stride-0 batch (packed once, one launch) equals
    the per-view path; a [...,4] input equals its [...,3:4] slice; and the frame equals
    mpi_render_view_torch on the explicitly constructed MPI."""
    g = pc.golden()
    x = load_test_mpi().to(dev)  # [1,400,640,10,4]
    pose, K, depths = (torch.tensor(large[k]).to(dev) for k in ("c1_pose", "c1_K", "c1_depths"))
    out = mvu.mpi_render_depth_torch(x.expand(2, *x.shape[1:]), pose, depths, K)
    got = out.cpu().numpy()
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(g["tm_sha"])
    assert_bits(got[:, 184:216, 304:336], g["tm_crop"], "centre crop")
    assert float(got[..., 2].max()) == 1.0 and float(got[..., 2].min()) < 1.0  # coverage
    per = mvu.mpi_render_depth_torch(x.repeat(2, 1, 1, 1, 1), pose, depths, K)  # non-broadcast: packs per view
    assert_bits(per, got, "per-view path")
    sl = mvu.mpi_render_depth_torch(x[..., 3:4].expand(2, 400, 640, 10, 1), pose, depths, K)
    assert_bits(sl, got, "[...,3:4] slice")
    colors = torch.stack([1.0 / depths, depths, torch.ones_like(depths)], -1)
    explicit = torch.cat([colors[None, None, None].expand(2, 400, 640, 10, 3),
                          x[..., 3:].expand(2, 400, 640, 10, 1)], -1)
    assert_bits(mvu.mpi_render_view_torch(explicit, pose, depths, K), got, "mpi_render_view_torch(constructed)")


def test_no_float_mpi_is_made(dev):
    """The wrapper's device memory: the packed alpha (1.39 MB) and the frame (0.25 MB), not a
    constructed or packed float MPI (>= 5.2 MB) -- peak growth below H*W*P*8 bytes."""
    H, W, P = 128, 160, 16
    x = torch.from_numpy(_alpha(H, W, P, 1)).to(dev)[None, ..., None].expand(1, H, W, P, 4).contiguous()
    t = _golden_inputs("pb", dev)  # (its camera)
    colors = torch.from_numpy(_colors(P, 2)).to(dev)
    planes = torch.linspace(30.0, 0.3, P, device=dev)
    args = (x, colors, t["pose"], planes, t["K"])
    want = mvu.mpi_render_plane_colors_torch(*args).cpu()  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = mvu.mpi_render_plane_colors_torch(*args)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak growth {growth} bytes (bound {H * W * P * 8})")
    assert growth < H * W * P * 8, growth
    assert growth >= (H + 4) * (W + 4) * P * 4  # the packed alpha was really made
    assert torch.equal(out.cpu(), want)


def test_autograd_rule(dev, monkeypatch):
    """Grad required: the result is the differentiable mpi_render_view_torch of the constructed MPI --
    the gradient equals that of the explicit construction and reaches only channel 3 (and the
    colours).  No grad required: the alpha entries run, nothing else renders."""
    B, H, W, P = 1, 23, 35, 5
    g = torch.Generator().manual_seed(9)
    base = torch.rand((B, H, W, P, 4), generator=g).to(dev)
    colors0 = (torch.rand((P, 3), generator=g) * 2 - 1).to(dev)
    dout = (torch.rand((B, H, W, 3), generator=g) * 2 - 1).to(dev)
    t = _golden_inputs("pb", dev)
    planes = torch.linspace(20.0, 0.5, P, device=dev)

    names = []
    call = _lib._call
    monkeypatch.setattr(_lib, "_call", lambda name, *a: (names.append(name), call(name, *a))[1])

    leaf, cl = base.clone().requires_grad_(True), colors0.clone().requires_grad_(True)
    out = mvu.mpi_render_plane_colors_torch(leaf, cl, t["pose"], planes, t["K"])
    out.backward(dout)
    assert "mpiv_render_packed_alpha" not in names
    ref_leaf, ref_cl = base.clone().requires_grad_(True), colors0.clone().requires_grad_(True)
    explicit = torch.cat([ref_cl[None, None, None].expand(B, H, W, P, 3), ref_leaf[..., 3:]], -1)
    ref = mvu.mpi_render_view_torch(explicit, t["pose"], planes, t["K"])
    ref.backward(dout)
    assert_bits(out, ref.detach().cpu().numpy(), "frame under autograd")
    assert_bits(leaf.grad, ref_leaf.grad.cpu().numpy(), "d rgba_layers")
    assert_bits(cl.grad, ref_cl.grad.cpu().numpy(), "d plane_colors")
    assert float(leaf.grad[..., :3].abs().max()) == 0.0 and float(leaf.grad[..., 3].abs().max()) > 0.0
    assert float(cl.grad.abs().max()) > 0.0

    for enabled, inp in ((True, base), (False, leaf)):  # nothing requires grad / grad disabled
        names.clear()
        with torch.set_grad_enabled(enabled):
            plain = mvu.mpi_render_plane_colors_torch(inp, colors0, t["pose"], planes, t["K"])
        assert not plain.requires_grad
        assert [n for n in names if "render" in n and "homographies" not in n] == ["mpiv_render_packed_alpha"]
        assert "mpiv_pack_planes_alpha" in names and "mpiv_pack_planes" not in names
        assert_bits(plain, out.detach().cpu().numpy(), "alpha kernel vs the autograd path's frame")


# ---------------------------------------------------------------------------
# 6: side stream, captured graph
# ---------------------------------------------------------------------------

def _stream_sets(dev):
    H, W, P, V = 64, 66, 16, 3
    _, homs = _extreme_case(8, H, W, P, seed=31)
    sets = []
    for k in range(2):
        rgba = np.random.default_rng(40 + k).random((H, W, P, 4), dtype=np.float32)
        rgba[..., 3] = _alpha(H, W, P, 50 + k)
        sets.append((torch.from_numpy(rgba).to(dev), torch.from_numpy(_colors(P, 60 + k)).to(dev),
                     homs[k * 3:k * 3 + V].contiguous().to(dev)))
    want = [_oracle(m.cpu().numpy()[..., 3], c.cpu().numpy(), h.cpu()) for m, c, h in sets]
    assert not np.array_equal(want[0], want[1])
    return (H, W, P, V), sets, want


def test_side_stream(dev):
    """Both entries on a side stream (channel 3 of an RGBA view, read in place): the oracle's frames."""
    (H, W, P, V), sets, want = _stream_sets(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = [_lib.render_packed_alpha(_lib.pack_planes_alpha(m), c, h, out=torch.full((V, H, W, 3), SENT, device=dev))
               for m, c, h in sets]
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2):
        assert_bits(got[k], want[k], f"side stream, data set {k}")


def test_captured_graph_replays_with_new_data(dev):
    """mpiv_pack_planes_alpha + mpiv_render_packed_alpha captured on a side stream and replayed with
    other alpha, colours and homographies in the static inputs: the oracle's frames on every replay."""
    (H, W, P, V), sets, want = _stream_sets(dev)
    m, c, h = (t.clone() for t in sets[1])
    pk = torch.full((P, H + 4, W + 4), SENT, device=dev)
    out = torch.full((V, H, W, 3), SENT, device=dev)
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):  # warm-up on the capture stream
        _lib.render_packed_alpha(_lib.pack_planes_alpha(m, out=pk), c, h, out=out)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        _lib.render_packed_alpha(_lib.pack_planes_alpha(m, out=pk), c, h, out=out)
    for k in (0, 1, 0):
        for dst, src in zip((m, c, h), sets[k]):
            dst.copy_(src)
        pk.fill_(SENT)
        out.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(out, want[k], f"replay with data set {k}")
