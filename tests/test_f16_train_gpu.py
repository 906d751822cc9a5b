"""GPU: training through a half MPI (mpi_render_view_f16 under autograd; render_chunk.hip InF16,
mpiv_render_train_f16, mpiv_render_backward[_watched|_cam]_f16).

Bars, all bit-exact.  The frame equals the float route's on x16.float().  x16.grad is float16 and equals
RN_half(G32) per view, G32 the float route's fp32 gradient on x16.float(): against the reference's own
half leaf gradients (tests/golden/f16grad.npz, pinned to the oracle by tests/test_f16_train.py) and
against .half() of _lib.render_backward(x16.float(), ...) on the same GPU.  Half -> float is exact, so
comparisons widen both sides; where the yardstick is NaN a NaN is required and the remaining bits are
compared (lattice_cases.match).  dhoms and the camera gradients are the float route's bits."""
import os

import numpy as np
import pytest
import torch

import stream_cases as sc
from conftest import GOLD, assert_bits
from lattice_cases import match
from test_backward_gpu import BWD_MODES
from test_camgrad_gpu import CASES as CAM_CASES
from test_camgrad_gpu import record_calls, same_bits
from test_f16_train import CASES, case_arrays

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

F16 = torch.float16


@pytest.fixture(scope="module")
def f16grad():
    return np.load(os.path.join(GOLD, "f16grad.npz"))


@pytest.fixture(scope="module")
def cam():
    return np.load(os.path.join(GOLD, "camgrad.npz"))


@pytest.fixture(params=list(BWD_MODES))
def bwd_mode(request, kopts):
    kopts(**BWD_MODES[request.param])  # ("barrier" selects an A/B kernel: skipped under the A/B gate)
    return request.param


def match16(got, want, what):
    """got is float16 and equals want (float16) bit for bit, NaN for NaN."""
    assert got.dtype == F16 and want.dtype == F16 and got.shape == want.shape, (what, got.dtype, got.shape)
    match(got.float(), want.float().cpu().numpy(), what)


def scene(V, H, W, P, seed, dev):
    """(x16 [V,H,W,P,4] half on dev, homs [V,P,9] on the host, dout [V,H,W,3] on dev) of a small sweep."""
    x16 = configs.synthetic_mpi(V, H, W, P, seed).half().to(dev)
    f = 0.9 * max(W, 8)
    K = configs.f32([configs.intrinsics_matrix(f, 1.05 * f, W / 2.0 + 0.5, H / 2.0 - 0.25)] * V)
    poses = configs.f32([configs.pose_from(configs.rot_y(1.5 * (v + 1)), (0.04 * (v + 1), -0.02, 0.03 * v))
                         for v in range(V)])
    depths = configs.f32(configs.inv_depths(1, 100, max(P, 2))[:P])  # (inv_depths returns both ends for P = 1)
    homs = _host.render_homographies(poses, depths, K, V).clone()
    dout = torch.rand((V, H, W, 3), generator=torch.Generator().manual_seed(seed + 100)) * 2 - 1
    return x16, homs, dout.to(dev)


def float_route(x16, homs, dout, **kw):
    """The yardstick: .half() of the float route's gradient on the widened MPI, one per view."""
    return _lib.render_backward(x16.float(), homs, dout, check=True, **kw).half()


# ---------------------------------------------------------------------------
# 1. against the reference's half leaf gradients
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_matches_the_reference_half_leaf(name, f16grad, dev, bwd_mode):
    c = case_arrays(f16grad, name)
    t = {k: torch.tensor(c[k]).to(dev) for k in ("pose", "K", "depths", "dout")}
    leaf = torch.tensor(c["mpi"]).to(dev).requires_grad_(True)
    out = mv.mpi_render_view_f16(leaf, t["pose"], t["depths"], t["K"])
    assert out.grad_fn is not None and out.dtype == torch.float32
    assert_bits(out.detach(), c["out"], f"{name} forward")
    out.backward(t["dout"])
    match16(leaf.grad, torch.tensor(c["grad"]), f"{name} d rgba_layers ({bwd_mode})")


@pytest.mark.parametrize("name", ["ga", "gp17"])
def test_wide_instantiations_forced_at_a_small_shape(name, f16grad, dev, kopts):
    """Views of 2 GiB and more take the wide half instantiations (64-bit tap addresses, 8-byte global
    loads); chunk_wide=1 forces them here: the same frames and half gradients."""
    kopts(chunk_wide=1)
    c = case_arrays(f16grad, name)
    B, H, W, P, _ = c["mpi"].shape
    t = {k: torch.tensor(c[k]).to(dev) for k in ("pose", "K", "depths", "dout")}
    leaf = torch.tensor(c["mpi"]).to(dev).requires_grad_(True)
    out = mv.mpi_render_view_f16(leaf, t["pose"], t["depths"], t["K"])
    assert_bits(out.detach(), c["out"], f"{name} forward, wide")
    out.backward(t["dout"])
    match16(leaf.grad, torch.tensor(c["grad"]), f"{name} d rgba_layers, wide")
    homs = torch.tensor(c["H"].transpose(1, 0, 2, 3).reshape(B, P, 9).copy())
    x16 = leaf.detach()
    g16, dh16 = _lib.render_backward(x16, homs, t["dout"], want_dhoms=True, check=True)  # ckpt=None, wide
    g32, dh32 = _lib.render_backward(x16.float(), homs, t["dout"], want_dhoms=True, check=True)
    match16(g16, g32.half(), "wide, no checkpoints")
    assert same_bits(dh16, dh32)


# ---------------------------------------------------------------------------
# 2. against the float route on the same GPU
# ---------------------------------------------------------------------------

# (P797: more planes than the training forward holds homographies for in LDS -- the frame comes from the
# packed f16 render without checkpoints, and the chain reads its homographies from global memory)
SHAPES = {
    "45x71x7": (2, 45, 71, 7), "33x65x9": (1, 33, 65, 9), "1x40x3": (1, 1, 40, 3), "40x1x3": (1, 40, 1, 3),
    "P1": (2, 19, 37, 1), "P17": (1, 24, 36, 17), "P797": (1, 9, 12, 797),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_equals_the_float_route_rounded_once(shape, dev):
    """Autograd (checkpoints from the training forward where the view is read in place) and the raw
    backward without checkpoints (ckpt=None: the chain recomputes them) against RN_half of the float
    route; frames against the float route's."""
    V, H, W, P = SHAPES[shape]
    x16, homs, dout = scene(V, H, W, P, 60 + P, dev)
    want = float_route(x16, homs, dout)
    match16(_lib.render_backward(x16, homs, dout, check=True), want, f"{shape}: ckpt=None")
    leaf = x16.clone().requires_grad_(True)
    out = _lib.RenderF16Function.apply(leaf, homs)
    match(out.detach(), _lib.render(x16.float(), homs).cpu().numpy(), f"{shape}: frame")
    out.backward(dout)
    match16(leaf.grad, want, f"{shape}: autograd")
    if P > 796:
        assert _lib.render_train(x16, homs)[1] is None
    elif H >= 2 and W >= 2:
        frames, ck = _lib.render_train(x16, homs)
        frames32, ck32 = _lib.render_train(x16.float(), homs)
        # (chunk 0's checkpoint slot is never written: the colour before plane 0 is the constant start)
        assert ck is not None and same_bits(ck[:, 1:], ck32[:, 1:]) and same_bits(frames, frames32)
        match16(_lib.render_backward(x16, homs, dout, ckpt=ck, check=True), want, f"{shape}: with checkpoints")


def test_minimum_workspace_runs_plane_groups(dev, kopts):
    """A caller's workspace of the minimum size: the backward runs in plane groups (forced to 8 planes
    on 19), the sizes being the float entries' own queries."""
    V, H, W, P = 1, 30, 41, 19
    x16, homs, dout = scene(V, H, W, P, 71, dev)
    want = float_route(x16, homs, dout)
    kopts(bwd_group=8)
    L = _lib.load()
    need = L.mpiv_render_backward_workspace_size_min(H, W, P)
    assert 0 < need <= L.mpiv_render_backward_workspace_size(H, W, P)
    for ck in (None, _lib.render_train(x16, homs)[1]):
        ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
        got = _lib.render_backward(x16, homs, dout, workspace=ws, ckpt=ck, check=True)
        match16(got, want, f"plane groups, ckpt {'given' if ck is not None else 'None'}")


def test_broadcast_batch_one_half_gradient_per_view(dev):
    """A stride-0 batch of 3: per-view half gradients, then autograd's expand backward sums them in half,
    exactly as torch sums those per-view gradients."""
    V, H, W, P = 3, 23, 35, 4
    x16, homs, dout = scene(1, H, W, P, 81, dev)
    _, homs, dout = scene(V, H, W, P, 82, dev)
    bc = x16.expand(V, H, W, P, 4)
    assert bc.stride(0) == 0
    per_view = _lib.render_backward(bc, homs, dout, check=True)
    match16(per_view, float_route(bc, homs, dout), "per-view gradients")
    leaf = x16.clone().requires_grad_(True)
    _lib.RenderF16Function.apply(leaf.expand(V, H, W, P, 4), homs).backward(dout)
    match16(leaf.grad, per_view.sum(dim=0, keepdim=True), "torch's own half sum of the per-view gradients")


def test_strided_view_is_read_in_place(dev):
    V, H, W, P = 1, 20, 34, 5
    big, homs, dout = scene(V, H + 2, W + 4, P, 91, dev)
    view = big[:, 1:-1, 2:-2]
    assert not view.is_contiguous() and _lib.bwd_layout_ok(view) and _lib._f16_in_place(view) is view
    homs = scene(V, H, W, P, 91, dev)[1]
    dout = dout[:, 1:-1, 2:-2].contiguous()
    leaf = view.detach().requires_grad_(True)
    assert _lib._f16_in_place(leaf) is leaf
    _lib.RenderF16Function.apply(leaf, homs).backward(dout)
    match16(leaf.grad, float_route(view, homs, dout), "strided in-place view")


def test_misaligned_view_takes_the_contiguous_half_copy(dev):
    """A data pointer that is only 4-byte aligned cannot be read as 8-byte texels: a half copy, never a
    float one; the same gradient."""
    V, H, W, P = 1, 17, 29, 3
    x16, homs, dout = scene(V, H, W, P, 95, dev)
    buf = torch.zeros(x16.numel() + 6, dtype=F16, device=dev)
    view = buf[2:2 + x16.numel()].view(V, H, W, P, 4)
    view.copy_(x16)
    assert view.data_ptr() % 8 == 4 and not _lib.bwd_layout_ok(view)
    leaf = view.detach().requires_grad_(True)
    _lib.RenderF16Function.apply(leaf, homs).backward(dout)
    match16(leaf.grad, float_route(x16, homs, dout), "4-byte aligned data pointer")


def test_special_texels(dev):
    """-0, +-65504, half subnormals, +-inf and NaN texels: no fault, NaN exactly where the float route
    has NaN, the remaining bits equal."""
    V, H, W, P = 1, 26, 38, 9
    x16, homs, dout = scene(V, H, W, P, 97, dev)
    flat = x16.view(-1)
    vals = torch.tensor([-0.0, 65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -15, float("inf"), float("-inf"),
                         float("nan")], dtype=F16, device=dev)
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(5))[:9 * 40].to(dev)
    flat[idx] = vals.repeat(40)
    want = float_route(x16, homs, dout)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())
    leaf = x16.clone().requires_grad_(True)
    out = _lib.RenderF16Function.apply(leaf, homs)
    match(out.detach(), _lib.render(x16.float(), homs).cpu().numpy(), "frame with special texels")
    out.backward(dout)
    match16(leaf.grad, want, "special texels")
    match16(_lib.render_backward(x16, homs, dout, check=True), want, "special texels, ckpt=None")


# ---------------------------------------------------------------------------
# 3. camera gradients
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ca", "cb"])
def test_camera_gradients_are_the_float_routes_bits(name, cam, dev):
    B, H, W, P, seed, _ = CAM_CASES[name]
    x16 = configs.synthetic_mpi(B, H, W, P, seed).half().to(dev)
    pose, depths, K = (torch.tensor(cam[f"{name}_{k}"]) for k in ("pose", "depths", "K"))
    homs = _host.render_homographies(pose, depths, K, B).to(dev)
    dout = torch.tensor(cam[f"{name}_dout"]).to(dev)
    g32, dh32 = _lib.render_backward(x16.float(), homs, dout, want_dhoms=True, check=True)
    g16, dh16 = _lib.render_backward(x16, homs, dout, want_dhoms=True, check=True)
    assert same_bits(dh16, dh32) and float(dh32.abs().max()) > 0
    match16(g16, g32.half(), f"{name}: d rgba_layers beside dhoms")
    none, fixed = _lib.render_backward(x16, homs, dout, want_dhoms=True, want_dmpi=False, check=True)
    assert none is None and same_bits(fixed, dh32)  # the fixed-MPI case

    def run(fn, mpi):
        cams = [t.clone().to(dev).requires_grad_(True) for t in (pose, depths, K)]
        fn(mpi, *cams).backward(dout)
        return [c.grad for c in cams]
    leaf16 = x16.clone().requires_grad_(True)
    got = run(mv.mpi_render_view_f16, leaf16)
    want = run(mv.mpi_render_view_torch, x16.float().requires_grad_(True))
    for g, w, what in zip(got, want, ("tgt_pose", "planes", "intrinsics")):
        assert g is not None and same_bits(g, w), what
    match16(leaf16.grad, g32.half(), f"{name}: x16.grad under a camera gradient")
    fixed_cam = run(mv.mpi_render_view_f16, x16)  # fixed MPI: only the cameras require grad
    for g, w, what in zip(fixed_cam, want, ("tgt_pose", "planes", "intrinsics")):
        assert same_bits(g, w), what + " (fixed MPI)"


# ---------------------------------------------------------------------------
# 4. routes that must not change; the new route's entries
# ---------------------------------------------------------------------------

def test_without_a_gradient_nothing_changes(dev, monkeypatch):
    """Nothing requires grad, or grad is disabled: exactly the entries the inference route calls (pack
    and packed render per view; one pack for a broadcast batch).  With a gradient: the half entries."""
    B, H, W, P = 2, 21, 33, 5
    x16, homs, dout = scene(B, H, W, P, 33, dev)
    pose = configs.f32([configs.pose_from(configs.rot_y(2.0), (0.05, -0.02, 0.04))] * B).to(dev)
    planes = configs.f32(configs.inv_depths(1, 100, P)).to(dev)
    K = configs.f32([configs.intrinsics_matrix(30.0, 31.0, 16.0, 10.0)] * B).to(dev)
    names = record_calls(monkeypatch)
    plain = mv.mpi_render_view_f16(x16, pose, planes, K)
    with torch.no_grad():
        a = mv.mpi_render_view_f16(x16.clone().requires_grad_(True), pose.clone().requires_grad_(True), planes, K)
    per_view = ["mpiv_pack_planes_f16", "mpiv_render_packed_f16"] * B
    assert names == ["mpiv_render_homographies_device"] + per_view + ["mpiv_render_homographies_device"] + per_view, names
    assert plain.grad_fn is None and a.grad_fn is None and same_bits(a, plain)
    del names[:]
    mv.mpi_render_view_f16(x16[:1].expand(B, H, W, P, 4), pose, planes, K)
    assert names == ["mpiv_render_homographies_device", "mpiv_pack_planes_f16", "mpiv_render_packed_f16"], names
    del names[:]
    leaf = x16.clone().requires_grad_(True)
    out = mv.mpi_render_view_f16(leaf, pose, planes, K)
    out.backward(dout)
    assert names == ["mpiv_render_homographies_device", "mpiv_render_train_f16", "mpiv_render_backward_watched_f16"], names
    assert same_bits(out.detach(), plain) and leaf.grad.dtype == F16
    # the float drop-in still refuses half input -- also when the half MPI or a camera input requires grad
    # (RenderFunction's own check: render_train / render_backward behind it serve half tensors) -- and no
    # training entry is reached
    del names[:]
    for mpi, cam_pose in ((x16, pose), (x16.clone().requires_grad_(True), pose),
                          (x16, pose.clone().requires_grad_(True)),
                          (x16.clone().requires_grad_(True), pose.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="expected scalar type Float but found torch.float16"):
            mv.mpi_render_view_torch(mpi, cam_pose, planes, K)
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        _lib.RenderFunction.apply(x16.clone().requires_grad_(True), homs.to(dev))
    with pytest.raises(RuntimeError, match="expected scalar type Half"):
        _lib.RenderF16Function.apply(x16.float().requires_grad_(True), homs.to(dev))
    assert not [n for n in names if "train" in n or "backward" in n], names


# ---------------------------------------------------------------------------
# 5. an aborted fallback is loud in half too
# ---------------------------------------------------------------------------

def test_forced_abort_gives_nan_halves(dev, kopts):
    """The zero-poll-limit debug option makes the (forced) fallback abort, as in
    tests/test_backward_gpu.py: that view's half gradient is all NaN and the status count is 1; the
    production path on the same workspace then gives the float route's gradient.
    Like that test, this one needs the A/B library: bwd_poll_limit is refused by the production build, so
    the default GPU run skips it at the A/B gate and the half NaN fills (dmpi_store in bwd_poison_kernel and
    in the fallback's last block) run only under MPIV_AB_TESTS=1."""
    V, H, W, P = 1, 45, 71, 7
    x16, homs, dout = scene(V, H, W, P, 44, dev)
    want = float_route(x16, homs, dout)
    kopts(bwd_fallback=1, bwd_poll_limit=-1)
    L = _lib.load()
    ws = torch.zeros(L.mpiv_render_backward_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    got = _lib.render_backward(x16, homs, dout, workspace=ws, check=False)
    assert _lib.render_backward_status(ws, H, W, P) == 1
    assert got.dtype == F16 and bool(torch.isnan(got).all())
    with pytest.raises(RuntimeError, match="aborted on 1 of 1 views"):
        _lib.render_backward(x16, homs, dout, workspace=ws, check=True)
    kopts(bwd_fallback=0, bwd_poll_limit=0)
    match16(_lib.render_backward(x16, homs, dout, workspace=ws, check=True), want, "after an abort")


# ---------------------------------------------------------------------------
# 6. side stream, captured graph replayed with new data
# ---------------------------------------------------------------------------

SP = 19  # planes of the stream cases: three chunks, the last partial


def _half_step_case(entry):
    """The training step on static buffers, as tests/stream_cases.py's backward cases: the forward that
    writes the checkpoints, the backward that takes them and the one that recomputes them.  Two data
    sets; expected values from the CPU oracle on the widened MPI, rounded to half once."""
    NB, NH, NW = sc.NB, sc.NH, sc.NW

    def mpi16(k):
        return sc._nat_mpi(k, SP).half()

    def inputs(k):
        return {"mpi": mpi16(k), "homs": sc.cam_homs(k, NB, SP, NH, NW), "dout": sc.lc.dout_for((NB, NH, NW, 3), seed=k)}

    def want(k):
        m, h = mpi16(k).float().numpy(), sc.cam_homs(k, NB, SP, NH, NW).numpy()
        g = oracle.render_backward(m, h, sc.lc.dout_for((NB, NH, NW, 3), seed=k).numpy()).astype(np.float16)
        return {"out": oracle.render(m, h), "grad_ckpt": g, "grad_null": g}

    def call(b, d):
        _lib._call("mpiv_render_train_f16", b["mpi"], sc._st(b["mpi"]), NB, NH, NW, SP, b["homs"], b["out"], b["ckpt"],
                   sc.S(d))
        _lib._call(entry, b["mpi"], sc._st(b["mpi"]), NB, NH, NW, SP, b["homs"], b["dout"], b["ckpt"], b["grad_ckpt"],
                   b["ws"], b["ws"].numel(), sc.S(d))
        _lib._call(entry, b["mpi"], sc._st(b["mpi"]), NB, NH, NW, SP, b["homs"], b["dout"], None, b["grad_null"],
                   b["ws"], b["ws"].numel(), sc.S(d))
    n = len(sc.CASES)
    try:  # (Case registers itself in the shared table, which lists one case per _SIGS entry: taken out again)
        return sc.Case(f"{entry[5:]}-half", [entry, "mpiv_render_train_f16"], inputs,
                       {"out": ((NB, NH, NW, 3), sc.F32), "ckpt": ((NB, (SP + 7) // 8, NH, NW, 4), sc.F32),
                        "grad_ckpt": ((NB, NH, NW, SP, 4), F16), "grad_null": ((NB, NH, NW, SP, 4), F16)},
                       call, want, state={"ws": sc._ws_bytes(NH, NW, SP)}, after=sc._no_abort(NH, NW, SP))
    finally:
        del sc.CASES[n:]


@pytest.mark.parametrize("entry", ["mpiv_render_backward_f16", "mpiv_render_backward_watched_f16"])
def test_side_stream_and_captured_replay_with_new_data(entry, dev):
    """Eager on a side stream, then captured there on a single stream and replayed with data sets 2, 1, 2
    copied into the static inputs: frames, and both half gradients, bit for bit every time."""
    sc.replay_case(_half_step_case(entry), dev)


class _RenderF16Module(torch.nn.Module):
    def __init__(self, pose, planes, K):
        super().__init__()
        self.pose, self.planes, self.K = pose, planes, K

    def forward(self, mpi16):
        return mv.mpi_render_view_f16(mpi16, self.pose, self.planes, self.K)


def test_autograd_step_captured_and_replayed_with_new_data(f16grad, dev):
    """The drop-in's own training step -- mpi_render_view_f16 under autograd, forward with checkpoints and
    the backward -- captured in HIP graphs (torch.cuda.make_graphed_callables, as
    tests/test_backward_gpu.py does for the float route) and replayed with the golden MPI, another one and
    the golden one again: frame and half gradient equal the eager step's bits on every replay, and the
    reference's on the golden data."""
    c = case_arrays(f16grad, "gp17")
    t = {k: torch.tensor(c[k]).to(dev) for k in ("pose", "K", "depths", "dout")}
    gold = torch.tensor(c["mpi"]).to(dev)
    other = configs.synthetic_mpi(*c["mpi"].shape[:4], 77).half().to(dev)
    module = _RenderF16Module(t["pose"], t["depths"], t["K"])
    eager = []
    for data in (gold, other):
        leaf = data.clone().requires_grad_(True)
        out = module(leaf)
        out.backward(t["dout"])
        eager.append((out.detach().clone(), leaf.grad.clone()))
    torch.cuda.synchronize()
    assert_bits(eager[0][0], c["out"], "eager forward")
    match16(eager[0][1], torch.tensor(c["grad"]), "eager half gradient")
    leaf = gold.clone().requires_grad_(True)
    graphed = torch.cuda.make_graphed_callables(module, (leaf,))
    for k in (0, 1, 0):
        with torch.no_grad():
            leaf.copy_((gold, other)[k])
        leaf.grad = None
        out = graphed(leaf)
        out.backward(t["dout"])
        torch.cuda.synchronize()
        assert same_bits(out.detach(), eager[k][0]), f"graphed forward, data set {k + 1}"
        match16(leaf.grad, eager[k][1], f"graphed half gradient, data set {k + 1}")


def test_autograd_step_on_a_side_stream(dev):
    """mpi_render_view_f16 forward and backward issued on a side stream equal the default stream's."""
    V, H, W, P = 2, 37, 70, 11
    x16, homs, dout = scene(V, H, W, P, 55, dev)
    leaf = x16.clone().requires_grad_(True)
    out = _lib.RenderF16Function.apply(leaf, homs.to(dev))
    out.backward(dout)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    leaf2 = x16.clone().requires_grad_(True)
    hd = homs.to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out2 = _lib.RenderF16Function.apply(leaf2, hd)
        out2.backward(dout)
    torch.cuda.synchronize()
    assert same_bits(out2.detach(), out.detach())
    match16(leaf2.grad, leaf.grad, "side stream")
