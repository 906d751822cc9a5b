"""GPU tests of the render's CAMERA gradient: d frame / d homographies (render_bwd_cam.hip,
mpiv_render_backward_cam) against the reference's autograd (tests/golden/camgrad.npz,
tools/gen_goldens_camgrad.py), and the public route from there to tgt_pose, planes and intrinsics.

Bars.  The per-sample terms are the reference's to the bit: golden `c1` has one non-zero term per sum,
so every summation order returns that rounded product and dhoms must EQUAL the reference's.  A full
frame's sum has no order the reference fixes, so it is held to the standard bound of an fp32 sum of
N = H*W rounded products in any order, fused or not: |dhoms - S64| <= gamma_N * A per entry, with
gamma_N = N u / (1 - N u), u = 2^-24, S64 the float64 sum of the reference's own fp32 per-pixel terms
and A the sum of their magnitudes.  One dropped pixel is about A / N (1.3e-3 A at N = 768) against a
bound of 4.6e-5 A.  Whatever the schedule, the result is the same bits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, assert_bits

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402

# name -> (B, H, W, P, MPI seed, broadcast), as tools/gen_goldens_camgrad.py CASES
CASES = {
    "ca": (2, 23, 35, 5, 41, False),
    "cb": (1, 24, 32, 17, 42, False),
    "cl": (1, 32, 96, 9, 43, False),
    "cf": (1, 36, 48, 5, 44, False),
    "cbc": (3, 23, 35, 4, 45, True),
    "c1": (8, 24, 32, 5, 46, False),
}
FULL = ["ca", "cb", "cl", "cf", "cbc"]


@pytest.fixture(scope="module")
def cam():
    return np.load(os.path.join(GOLD, "camgrad.npz"))


_MEMO: dict = {}


def inputs(cam, name, dev):
    """(MPI [B,H,W,P,4] on dev -- a stride-0 expand for the broadcast case --, homs [B,P,9] on dev, dout)."""
    if name not in _MEMO:
        B, H, W, P, seed, broadcast = CASES[name]
        mpi = configs.synthetic_mpi(1 if broadcast else B, H, W, P, seed).to(dev)
        if broadcast:
            mpi = mpi.expand(B, H, W, P, 4)
        pose, depths, K = (torch.tensor(cam[f"{name}_{k}"]) for k in ("pose", "depths", "K"))
        homs = _host.render_homographies(pose, depths, K, B).to(dev)
        _MEMO[name] = (mpi, homs, torch.tensor(cam[f"{name}_dout"]).to(dev))
    return _MEMO[name]


def cam_backward(mpi, homs, dout, **kw):
    grad, dhoms = _lib.render_backward(mpi, homs, dout, want_dhoms=True, check=True, **kw)
    assert dhoms.shape == homs.shape and dhoms.is_cuda
    return grad, dhoms


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------
# 1. single-term exactness
# ---------------------------------------------------------------------------

def test_single_term_sums_equal_the_reference(cam, dev):
    """c1: eight views of one pose, view i's dout non-zero at one pixel (corners, an edge, interior
    pixels, samples with one, two and no tap inside the image): dhoms == the reference's dH as floats
    (-0 == +0), and a pixel with no tap inside gives zeros."""
    mpi, homs, dout = inputs(cam, "c1", dev)
    _, dhoms = cam_backward(mpi, homs, dout)
    got, want = dhoms.cpu().numpy(), cam["c1_dH"]
    bad = got != want
    assert not bad.any(), (f"{int(bad.sum())}/{bad.size} entries differ, first at {np.argwhere(bad)[0]}: "
                           f"got {got[bad][0]!r}, want {want[bad][0]!r}; pixels {cam['c1_pixels'].tolist()}")
    assert not got[7].any() and np.abs(got[0]).max() > 0 and np.abs(got[3]).max() > 0


# ---------------------------------------------------------------------------
# 2. full frames
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", FULL)
def test_full_frame_sums_within_the_summation_bound(name, cam, dev):
    B, H, W, P = CASES[name][:4]
    mpi, homs, dout = inputs(cam, name, dev)
    _, dhoms = cam_backward(mpi, homs, dout)
    got = dhoms.cpu().numpy().astype(np.float64)
    S64, A = cam[f"{name}_S64"], cam[f"{name}_A"]
    N = H * W
    gamma = N * 2.0 ** -24 / (1 - N * 2.0 ** -24)
    err = np.abs(got - S64)
    ratio = (err / np.maximum(A * 2.0 ** -24, 1e-300)).max()
    ref = (np.abs(cam[f"{name}_dH"].astype(np.float64) - S64) / np.maximum(A * 2.0 ** -24, 1e-300)).max()
    print(f"{name}: worst |dhoms - S64| = {ratio:.3f} x 2^-24 A (the reference's own: {ref:.3f}; bound "
          f"{gamma * 2 ** 24:.0f})")
    assert np.isfinite(got).all()
    assert (err <= gamma * A).all(), f"{name}: worst error {ratio:.1f} x 2^-24 A, bound {gamma * 2 ** 24:.1f}"
    assert not got[A == 0].any()
    assert A.max() > 0


# ---------------------------------------------------------------------------
# 3. one result, every schedule;  4. the MPI gradient is untouched
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cb", "cl", "ca", "cbc"])
def test_every_schedule_gives_the_same_bits(name, cam, dev, kopts):
    B, H, W, P = CASES[name][:4]
    mpi, homs, dout = inputs(cam, name, dev)
    L = _lib.load()
    _, base = cam_backward(mpi, homs, dout)
    runs = {"a second call": cam_backward(mpi, homs, dout)[1]}
    _, ck = _lib.render_train(mpi, homs, broadcast_in_place=True)
    assert ck is not None
    runs["with checkpoints"] = cam_backward(mpi, homs, dout, ckpt=ck)[1]
    g0, runs["fixed MPI"] = cam_backward(mpi, homs, dout, want_dmpi=False)
    assert g0 is None
    runs["fixed MPI, with checkpoints"] = cam_backward(mpi, homs, dout, want_dmpi=False, ckpt=ck)[1]
    n_min, n_full = (L.mpiv_render_backward_cam_workspace_size_min(H, W, P),
                     L.mpiv_render_backward_cam_workspace_size(H, W, P))
    assert L.mpiv_render_backward_workspace_size_min(H, W, P) < n_min <= n_full
    for what, n in (("minimum", n_min), ("fastest", n_full)):
        # 0xFF bytes: every stale float is a NaN -- the d samples of dead tiles (cl) stay unwritten
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
        runs[f"{what} workspace, 0xFF"] = cam_backward(mpi, homs, dout, workspace=ws)[1]
        ws.fill_(0xFF)
        runs[f"{what} workspace, 0xFF, fixed MPI"] = cam_backward(mpi, homs, dout, workspace=ws, want_dmpi=False)[1]
        # the head is left as the next call expects it: a plain backward in the same workspace
        assert same_bits(_lib.render_backward(mpi, homs, dout, workspace=ws, check=True),
                         _lib.render_backward(mpi, homs, dout, check=True))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        runs["side stream"] = cam_backward(mpi, homs, dout)[1]
        runs["side stream, fixed MPI"] = cam_backward(mpi, homs, dout, want_dmpi=False)[1]
    torch.cuda.current_stream(dev).wait_stream(side)
    if P > 8:
        kopts(bwd_group=8)
        assert L.mpiv_render_backward_cam_workspace_size(H, W, P) < n_full
        runs["groups of 8"] = cam_backward(mpi, homs, dout)[1]
        runs["groups of 8, checkpoints"] = cam_backward(mpi, homs, dout, ckpt=ck)[1]
        runs["groups of 8, fixed MPI"] = cam_backward(mpi, homs, dout, want_dmpi=False)[1]
    torch.cuda.synchronize()
    assert float(base.abs().max()) > 0
    for what, got in runs.items():
        assert same_bits(got, base), f"{name}, {what}: dhoms differs from the first call's"


@pytest.mark.parametrize("name", list(CASES))
def test_mpi_gradient_is_the_plain_backwards(name, cam, dev):
    mpi, homs, dout = inputs(cam, name, dev)
    want = _lib.render_backward(mpi, homs, dout, check=True)
    got, _ = cam_backward(mpi, homs, dout)
    assert same_bits(got, want)
    if not CASES[name][5]:  # (and the reference's own, per view)
        assert_bits(got, cam[f"{name}_dmpi"], f"{name} d rgba_layers")


def test_arguments_are_validated(cam, dev):
    mpi, homs, dout = inputs(cam, "ca", dev)
    B, H, W, P = CASES["ca"][:4]
    L = _lib.load()
    small = torch.empty(L.mpiv_render_backward_cam_workspace_size_min(H, W, P) - 256, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.render_backward(mpi, homs, dout, workspace=small, want_dhoms=True)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        _lib.render_backward(mpi, homs, dout, want_dmpi=False)
    ws = torch.empty(L.mpiv_render_backward_cam_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib._call("mpiv_render_backward_cam", mpi, _lib._strides(mpi), B, H, W, P, homs, dout, None, None, None, ws,
                   ws.numel(), 0, _lib._stream(dev))


# ---------------------------------------------------------------------------
# 5. public API
# ---------------------------------------------------------------------------

def chain_grads(cam, name, dhoms):
    """The CPU chain's backpropagation of dhoms [B,P,9]: (d tgt_pose, d planes, d intrinsics)."""
    pose, depths, K = (torch.tensor(cam[f"{name}_{k}"]).requires_grad_() for k in ("pose", "depths", "K"))
    _host.render_homographies_autograd(pose, depths, K, pose.shape[0]).backward(dhoms.detach().cpu())
    return pose.grad, depths.grad, K.grad


def record_calls(monkeypatch):
    names = []
    real = _lib._call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", call)
    return names


@pytest.mark.parametrize("name", ["ca", "cb", "cl"])
@pytest.mark.parametrize("train_mpi", [True, False])
@pytest.mark.parametrize("cams_on", ["device", "host"])
def test_render_is_differentiable_in_pose_planes_and_intrinsics(name, train_mpi, cams_on, cam, dev, monkeypatch):
    mpi, homs, dout = inputs(cam, name, dev)
    where = dev if cams_on == "device" else "cpu"
    pose, planes, K = (torch.tensor(cam[f"{name}_{k}"]).to(where) for k in ("pose", "depths", "K"))
    plain = mv.mpi_render_view_torch(mpi, pose, planes, K)
    leaf = mpi.clone().requires_grad_(train_mpi)
    names = record_calls(monkeypatch)
    out = mv.mpi_render_view_torch(leaf, pose.requires_grad_(), planes.requires_grad_(), K.requires_grad_())
    assert same_bits(out.detach(), plain), "the frame differs from the no-grad call's"
    out.backward(dout)
    assert "mpiv_render_backward_cam" in names and "mpiv_render_backward" not in names
    want_mpi, dhoms = cam_backward(mpi, homs, dout)
    for got, want, what in zip((pose.grad, planes.grad, K.grad), chain_grads(cam, name, dhoms),
                               ("tgt_pose", "planes", "intrinsics")):
        assert got is not None and got.device == torch.device(where), f"no gradient for {what}"
        assert_bits(got, want.numpy(), f"{name} d {what}")
        assert float(got.abs().max()) > 0
    if train_mpi:
        assert same_bits(leaf.grad, want_mpi)
    else:
        assert leaf.grad is None
    # one camera input alone
    pose.grad = None
    p2 = torch.tensor(cam[f"{name}_depths"]).to(where)
    mv.mpi_render_view_torch(mpi, pose, p2, K.detach()).backward(dout)
    assert_bits(pose.grad, chain_grads(cam, name, dhoms)[0].numpy(), f"{name} d tgt_pose alone")
    assert p2.grad is None


def test_broadcast_mpi_sums_its_views_and_is_read_in_place(cam, dev, monkeypatch):
    B, H, W, P, seed, _ = CASES["cbc"]
    mpi, homs, dout = inputs(cam, "cbc", dev)
    pose, planes, K = (torch.tensor(cam[f"cbc_{k}"]).to(dev).requires_grad_() for k in ("pose", "depths", "K"))
    leaf = mpi[:1].clone().requires_grad_(True)
    names = record_calls(monkeypatch)
    out = mv.mpi_render_view_torch(leaf.expand(B, H, W, P, 4), pose, planes, K)
    assert "mpiv_render_train" in names and not any("pack" in n for n in names), names
    assert same_bits(out.detach(), mv.mpi_render_view_torch(mpi, pose.detach(), planes.detach(), K.detach()))
    out.backward(dout)
    per_view, dhoms = cam_backward(mpi, homs, dout)
    assert tuple(leaf.grad.shape) == (1, H, W, P, 4)
    # (the sum over the views is torch's own, as in tests/test_backward_gpu.py: 1e-6 absolute)
    assert float((leaf.grad - per_view.sum(0, keepdim=True)).abs().max()) <= 1e-6
    assert float((leaf.grad.cpu() - torch.tensor(cam["cbc_dmpi"])).abs().max()) <= 1e-5
    for got, want, what in zip((pose.grad, planes.grad, K.grad), chain_grads(cam, "cbc", dhoms),
                               ("tgt_pose", "planes", "intrinsics")):
        assert_bits(got, want.numpy(), f"cbc d {what}")


@pytest.mark.parametrize("train_net", [True, False])
def test_net_output_render_is_differentiable_in_the_cameras(train_net, cam, dev):
    B, H, W, P = 2, 24, 32, 5
    g = torch.Generator().manual_seed(5)
    pred = (torch.rand((B, 2 * P + 3, H, W), generator=g) * 2 - 1).to(dev)
    fg = (torch.rand((B, H, W, 3), generator=g) * 2 - 1).to(dev)
    dout = (torch.rand((B, H, W, 3), generator=g) * 2 - 1).to(dev)
    pose, planes, K = (torch.tensor(cam[f"ca_{k}"]).to(dev) for k in ("pose", "depths", "K"))
    plain = mv.mpi_render_net_output_torch(pred, fg, pose, planes, K)
    want_pred = None
    if train_net:
        ref_leaf = pred.clone().requires_grad_(True)
        mv.mpi_render_net_output_torch(ref_leaf, fg, pose, planes, K).backward(dout)
        want_pred = ref_leaf.grad
    leaf = pred.clone().requires_grad_(train_net)
    out = mv.mpi_render_net_output_torch(leaf, fg, pose.requires_grad_(), planes.requires_grad_(), K.requires_grad_())
    assert same_bits(out.detach(), plain)
    out.backward(dout)
    homs = _host.render_homographies(pose.detach().cpu(), planes.detach().cpu(), K.detach().cpu(), B).to(dev)
    _, dhoms = cam_backward(_lib.assemble_mpi(pred, fg, P), homs, dout)
    for got, want, what in zip((pose.grad, planes.grad, K.grad), chain_grads(cam, "ca", dhoms),
                               ("tgt_pose", "planes", "intrinsics")):
        assert got is not None, f"no gradient for {what}"
        assert_bits(got, want.numpy(), f"net output d {what}")
        assert float(got.abs().max()) > 0
    if train_net:
        assert same_bits(leaf.grad, want_pred)


def test_without_a_camera_gradient_nothing_changes(cam, dev, monkeypatch):
    """No camera input requires grad: the entries called and the kernels routed are the MPI-only ones."""
    B, H, W, P = CASES["ca"][:4]
    mpi, homs, dout = inputs(cam, "ca", dev)
    pose, planes, K = (torch.tensor(cam[f"ca_{k}"]).to(dev) for k in ("pose", "depths", "K"))
    assert _lib.route("render_backward", B, H, W, P) == ("bwd_chain_strip_kernel<8>", (W + 31) // 32 * ((H + 7) // 8) * 256)
    names = record_calls(monkeypatch)
    leaf = mpi.clone().requires_grad_(True)
    mv.mpi_render_view_torch(leaf, pose, planes, K).backward(dout)
    with torch.no_grad():  # grad disabled: the inference route, whatever the cameras ask for
        mv.mpi_render_view_torch(mpi, pose.clone().requires_grad_(), planes, K)
    mv.mpi_render_view_torch(mpi, pose, planes, K)
    assert names == ["mpiv_render_homographies_device", "mpiv_render_train", "mpiv_render_backward_watched",
                     "mpiv_render_homographies_device", "mpiv_render", "mpiv_render_homographies_device",
                     "mpiv_render"], names
    assert_bits(leaf.grad, cam["ca_dmpi"], "d rgba_layers")


# ---------------------------------------------------------------------------
# 6. a view beyond 2 GiB
# ---------------------------------------------------------------------------

def test_wide_view_gives_the_dense_tensors_bits(dev):
    """One strided view whose span passes 2 GiB (row stride 15 000 000 floats, as
    tests/test_wide_views_gpu.py builds it): the wide tap helpers, same dhoms as the dense copy."""
    ROW, H, W, P = 15_000_000, 48, 24, 11
    mpi = configs.synthetic_mpi(1, H, W, P, 71).to(dev)
    K = configs.f32([configs.intrinsics_matrix(32.0, 32.0, W / 2.0, H / 2.0)])
    pose = configs.f32([configs.pose_from(configs.rot_y(3.0), (0.05, -0.02, 0.04))])
    homs = _host.render_homographies(pose, configs.f32(configs.inv_depths(1, 60, P)), K, 1).to(dev)
    dout = (torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(72)) * 2 - 1).to(dev)
    flat = torch.empty(H * ROW, dtype=torch.float32, device=dev)
    try:
        view = flat.as_strided((1, H, W, P, 4), (0, ROW, P * 4, 4, 1))
        view.copy_(mpi)
        assert (H - 1) * ROW * 4 > 1 << 31 and _lib.bwd_layout_ok(view) and not _lib.chunk_layout_ok(view)
        want_g, want = cam_backward(mpi, homs, dout)
        got_g, got = cam_backward(view, homs, dout)
        fixed = cam_backward(view, homs, dout, want_dmpi=False)[1]
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0
        assert same_bits(got, want) and same_bits(fixed, want) and same_bits(got_g, want_g)
    finally:
        del flat, view
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 7. capture
# ---------------------------------------------------------------------------

def test_captured_backward_replays_with_new_data(cam, dev):
    """mpiv_render_backward_cam (device homographies, the caller's workspace) captured on a side stream --
    with the MPI gradient and for a fixed MPI -- and replayed with other inputs: the eager results'
    bits on every replay."""
    B, H, W, P = CASES["cb"][:4]
    mpi, homs, dout = inputs(cam, "cb", dev)
    sets = [(mpi, homs, dout), (mpi.flip(2).contiguous(), homs, (dout * -0.5).flip(1).contiguous())]
    want = [cam_backward(*s) for s in sets]
    m, h, d = (t.clone() for t in sets[1])
    ws = torch.empty(_lib.load().mpiv_render_backward_cam_workspace_size(H, W, P), dtype=torch.uint8, device=dev)
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):  # warm-up on the capture stream
        _lib.render_backward(m, h, d, workspace=ws, want_dhoms=True, check=False)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        grad, dh = _lib.render_backward(m, h, d, workspace=ws, want_dhoms=True, check=False)
        _, dh_fixed = _lib.render_backward(m, h, d, workspace=ws, want_dhoms=True, want_dmpi=False, check=False)
    for k in (0, 1, 0):
        for dst, src in zip((m, h, d), sets[k]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(grad, want[k][0]) and same_bits(dh, want[k][1]) and same_bits(dh_fixed, want[k][1]), k
    assert not same_bits(want[0][1], want[1][1])


def test_camera_gradient_raises_under_capture(cam, dev, monkeypatch):
    """The chain's device-to-host copy of the cameras cannot be part of a captured graph: the
    host_under_capture error, before anything is launched."""
    mpi, homs, dout = inputs(cam, "ca", dev)
    pose, planes, K = (torch.tensor(cam[f"ca_{k}"]).to(dev) for k in ("pose", "depths", "K"))
    pose.requires_grad_()
    pred = torch.zeros((2, 13, 23, 35), device=dev)
    torch.cuda.synchronize()

    def refuse(name, *a):
        raise AssertionError(f"{name} was called: the error must be raised before any launch")
    monkeypatch.setattr(_lib, "_call", refuse)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        mv.mpi_render_view_torch(mpi, pose, planes, K)
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        mv.mpi_render_net_output_torch(pred, mpi[..., 0, :3], pose, planes, K)
