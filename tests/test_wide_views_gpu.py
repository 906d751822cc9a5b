"""Training through MPI views of 2 GiB and more, read in place: the wide instantiations of the in-place
tap readers (render_chunk.hip issue_taps_*_wide: 64-bit tap addresses, predicated 16-byte global
loads) behind mpiv_render_train and mpiv_render_backward.

1. forced at small shapes (chunk_wide=1) against the reference's goldens, the oracle and the lattice
   matrices, in tile mode and through the bucket fallback, frames and checkpoints also against the
   narrow kernels' bits;
2. taps really read beyond 2^31 bytes from a view's base (a strided view of one 2.9 GB allocation);
3. a dense 1024 x 1024 x 136 view (2.28 GB) through the drop-in's autograd;
4. the fused net-output path at that size;
5. a captured training step under chunk_wide=1.

Every comparison is bit-exact; expected values come from the goldens and the CPU oracle, at full
size from the packed render (pinned to the oracle by the small cases) and from the agreement of the
tile gather, the bucket fallback and the plane-group schedule."""
import functools
import os

import numpy as np
import pytest
import torch

import lattice_cases as lc
import test_lattice_gpu as tl
from conftest import GOLD, assert_bits
from lattice_cases import match

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

MODES = {"tile": {}, "fallback": {"bwd_fallback": 1}}


@pytest.fixture(params=list(MODES))
def wide_mode(request, kopts):
    """chunk_wide=1 (the wide instantiations at any size) in tile mode / through the bucket fallback."""
    kopts(chunk_wide=1, **MODES[request.param])
    return request.param


def _backward_flag(mpi, homs, dout, dev, ckpt=None, ws_bytes=None):
    """(gradient, fallback flag of the last view) through a caller-owned workspace; nothing aborted."""
    B, H, W, P, _ = mpi.shape
    L = _lib.load()
    n = L.mpiv_render_backward_workspace_size(H, W, P) if ws_bytes is None else ws_bytes
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    got = _lib.render_backward(mpi, homs, dout, workspace=ws, ckpt=ckpt)
    off = _lib.bwd_flag_offset(H, W, P)
    words = ws[off:off + 20].view(torch.int32).tolist()
    assert words[3] == 0 and words[4] == 0, "the fallback aborted"
    assert _lib.render_backward_status(ws, H, W, P) == 0
    return got, words[0]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------
# 1. forced wide at small shapes
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grad():
    return np.load(os.path.join(GOLD, "grad.npz"))


@pytest.mark.parametrize("name", ["ga", "gbig", "gbin"])
def test_wide_matches_reference_autograd(name, dev, wide_mode):
    grad = _grad()
    t = {k: torch.tensor(grad[f"{name}_{k}"]).to(dev) for k in ("pose", "K", "depths", "dout")}
    leaf = torch.tensor(grad[f"{name}_mpi"]).to(dev).requires_grad_(True)
    out = mv.mpi_render_view_torch(leaf, t["pose"], t["depths"], t["K"])
    assert_bits(out.detach(), grad[f"{name}_out"], f"{name} forward")
    out.backward(t["dout"])
    assert_bits(leaf.grad, grad[f"{name}_grad"], f"{name} d rgba_layers")


def _collapsing():
    g = torch.Generator().manual_seed(17)
    H, W, P = 48, 80, 3
    mpi = configs.synthetic_mpi(1, H, W, P, 21)
    s = (H - 1) / (W - 1)
    homs = torch.tensor([[[0.0, 0.0, 12.3, 0.0, 0.0, 7.6, 0.0, 0.0, 1.0],
                          [16.0 * s, 0.0, 0.5, 0.0, 16.0 / s, 0.25, 0.0, 0.0, 1.0],
                          [1.01, 0.02, -0.7, -0.01, 0.99, 0.4, 1e-4, 0.0, 1.0]]], dtype=torch.float32)
    return mpi, homs, torch.rand((1, H, W, 3), generator=g) * 2 - 1


def _extreme():
    g = torch.Generator().manual_seed(5)
    H, W, P, V = 45, 71, 7, 5
    mpi = configs.synthetic_mpi(V, H, W, P, 8)
    poses = []
    for k in range(V):
        t = ((torch.rand(3, generator=g) - 0.5) * (0.4 + 1.2 * k)).tolist()
        poses.append(configs.pose_from(configs.rot_y((k - 2) * 15.0), t))
    K = configs.f32([configs.intrinsics_matrix(60.0 + 30 * k, 64.0, 35.0, 22.0) for k in range(V)])
    homs = _host.render_homographies(configs.f32(poses), configs.f32(configs.inv_depths(0.4, 20, P)), K, V)
    return mpi, homs, torch.rand((V, H, W, 3), generator=g) * 2 - 1


def _medium():
    H, W, P = 192, 320, 24
    mpi = configs.synthetic_mpi(1, H, W, P, 9)
    K = configs.f32([configs.intrinsics_matrix(277.0, 277.0, 160.0, 96.0)])
    homs = _host.render_homographies(configs.f32([configs.config4()["poses"][123]]),
                                     configs.f32(configs.inv_depths(1, 100, P)), K, 1)
    return mpi, homs, torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)) * 2 - 1


def _odd(H, W, P):
    """Odd sizes: W % 8 != 0, a partial plane chunk and gather group, partial strips."""
    mpi = configs.synthetic_mpi(1, H, W, P, 4 + P)
    K = configs.f32([configs.intrinsics_matrix(40.0, 40.0, W / 2.0, H / 2.0)])
    homs = _host.render_homographies(configs.f32([configs.config4()["poses"][300]]),
                                     configs.f32(configs.inv_depths(1, 50, P)), K, 1)
    return mpi, homs, torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(8)) * 2 - 1


ORACLE_CASES = {"collapsing": _collapsing, "extreme": _extreme, "medium": _medium,
                "37x53x11": lambda: _odd(37, 53, 11), "12x40x20": lambda: _odd(12, 40, 20)}


@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    """(mpi, homs, dout, the oracle's frames, the oracle's gradient), computed once for both modes."""
    mpi, homs, dout = ORACLE_CASES[name]()
    return (mpi, homs, dout, oracle.render(mpi.numpy(), homs.numpy()),
            oracle.render_backward(mpi.numpy(), homs.numpy(), dout.numpy()))


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_wide_vs_oracle(name, dev, wide_mode, kopts):
    """Frames and gradient against the oracle, with the forward's checkpoints and with the checkpoints the
    backward recomputes (the wide strip forward into the workspace); the frames and checkpoints equal the
    narrow kernel's bits."""
    mpi, homs, dout, want_out, want_grad = _oracle_case(name)
    m, h, d = mpi.to(dev), homs.to(dev), dout.to(dev)
    out, ck = _lib.render_train(m, h)
    assert ck is not None
    assert_bits(out, want_out, f"{name} frames")
    got, flag = _backward_flag(m, h, d, dev, ckpt=ck)
    assert_bits(got, want_grad, f"{name} with checkpoints")
    if name == "medium":
        assert flag == (0 if wide_mode == "tile" else 1)
    got, _ = _backward_flag(m, h, d, dev)
    assert_bits(got, want_grad, f"{name} without checkpoints")
    kopts(chunk_wide=0)
    out_n, ck_n = _lib.render_train(m, h)
    assert _same_bits(out, out_n), "frames: wide != narrow"
    assert _same_bits(ck[:, 1:], ck_n[:, 1:]), "checkpoints: wide != narrow"  # (slot 0 is never written)


def test_wide_plane_groups_vs_oracle(dev, wide_mode, kopts):
    """The wide chain over plane groups (bwd_group=8 on 24 planes: the running adjoint handed down between
    groups), with the forward's checkpoints and with the wide forward pass into the workspace."""
    mpi, homs, dout, _, want_grad = _oracle_case("medium")
    kopts(bwd_group=8)
    m, h, d = mpi.to(dev), homs.to(dev), dout.to(dev)
    got, _ = _backward_flag(m, h, d, dev)
    assert_bits(got, want_grad, "groups of 8, no checkpoints")
    got, _ = _backward_flag(m, h, d, dev, ckpt=_lib.render_train(m, h)[1])
    assert_bits(got, want_grad, "groups of 8, checkpoints")


def test_wide_degenerate_frame_vs_oracle(dev, wide_mode):
    """H == 1: the generic recipe's chain (bwd_chain_kernel<0, false, 1, true>, taps through
    issue_taps_chunk_wide) and the forced fallback."""
    H, W, P = 1, 70, 11
    mpi = configs.synthetic_mpi(2, H, W, P, 12)
    homs = torch.from_numpy(np.ascontiguousarray(lc.views("int_shift", lc.X_SMALL, 2, P), np.float32))
    dout = lc.dout_for((2, H, W, 3))
    want = oracle.render_backward(mpi.numpy(), homs.numpy(), dout.numpy())
    got, _ = _backward_flag(mpi.to(dev), homs, dout.to(dev), dev)
    match(got, want, "H == 1")


@functools.lru_cache(maxsize=None)
def _lattice_backward_want(fam, kind, shape, nb):
    h = tl._homs(fam, shape, tl.BN, tl.PN)[:nb]
    m = tl._native_mpi(kind, shape)[:nb]
    dout = lc.dout_for((nb, shape[0], shape[1], 3))
    return oracle.render_backward(m.numpy(), h.numpy(), dout.numpy())


@pytest.mark.parametrize("fam,kind", tl.BWD_CASES, ids=[f"{f}-{k}" for f, k in tl.BWD_CASES])
def test_wide_lattice_backward(fam, kind, dev, wide_mode):
    """tests/test_lattice_gpu.py's backward matrix (exact-lattice positions, dead-tile thresholds, huge /
    w == 0 / non-finite homographies, non-finite texels) through the wide kernels; signed zeros count."""
    for shape in tl.shapes_of(fam):
        H, W = shape
        nb = tl.BN if fam in ("nonfinite_h", "edge") else 2
        h = tl._homs(fam, shape, tl.BN, tl.PN)[:nb]
        md = tl._native_mpi(kind, shape)[:nb].to(dev)
        dout = lc.dout_for((nb, H, W, 3)).to(dev)
        want = _lattice_backward_want(fam, kind, shape, nb)
        match(tl._backward_checked(md, h, dout, None, dev), want, f"{shape} without checkpoints")
        _, ck = _lib.render_train(md, h)
        match(tl._backward_checked(md, h, dout, ck, dev), want, f"{shape} with checkpoints")


@pytest.mark.parametrize("P", [tl.PN, 19])
@pytest.mark.parametrize("fam", tl.GPU_FAMILIES)
def test_wide_lattice_training_forward(fam, P, dev, kopts):
    """tests/test_lattice_gpu.py's training-forward matrix through the wide strip kernel: frames and
    checkpoints against the oracle (finite and non-finite texels), and against the narrow kernel."""
    for shape in tl.shapes_of(fam):
        h = tl._homs(fam, shape, tl.BN, P)
        for kind in tl.KINDS:
            m = tl._native_mpi(kind, shape, P).to(dev)
            kopts(chunk_wide=1)
            out, ck = _lib.render_train(m, h)
            assert ck is not None
            match(out, tl._native_want(fam, shape, kind, P), f"{shape} {kind} frames")
            for c in range(1, (P + 7) // 8):
                match(ck[:, c, :, :, :3], tl._native_want(fam, shape, kind, P, 8 * c),
                      f"{shape} {kind} checkpoint {c}")
                assert bool((ck[:, c, :, :, 3].view(torch.int32) == 0).all()), "checkpoint channel 3 is +0"
            kopts(chunk_wide=0)
            out_n, ck_n = _lib.render_train(m, h)
            match(out, out_n, f"{shape} {kind} frames: wide vs narrow")
            match(ck[:, 1:], ck_n[:, 1:], f"{shape} {kind} checkpoints: wide vs narrow")


# ---------------------------------------------------------------------------
# 2. offsets past 2^31 really read (no forcing)
# ---------------------------------------------------------------------------

ROW = 15_000_000  # floats between image rows of the strided views
SH, SW, SP = 48, 24, 11


@pytest.fixture(scope="module")
def flat(dev):
    """One uninitialised 2.9 GB allocation; rows 36..47 of a view with row stride ROW lie beyond 2^31 bytes."""
    buf = torch.empty(SH * ROW, dtype=torch.float32, device=dev)
    yield buf
    del buf
    torch.cuda.empty_cache()


def _strided_case(V, seed):
    mpi = configs.synthetic_mpi(V, SH, SW, SP, seed)
    c = configs.config4()
    K = configs.f32([configs.intrinsics_matrix(30.0, 30.0, SW / 2.0, SH / 2.0)] * V)
    homs = _host.render_homographies(configs.f32(c["poses"][250:250 + V]), configs.f32(configs.inv_depths(1, 60, SP)),
                                     K, V)
    dout = torch.rand((V, SH, SW, 3), generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    return mpi, homs, dout


@pytest.mark.parametrize("V", [1, 2])
def test_strided_view_beyond_2_gib_is_read_in_place(V, flat, dev):
    """[V,48,24,11,4] with row stride 15 000 000 floats (V = 2: batch stride one image row, both views
    interleaved in the one allocation): render_train returns checkpoints, its frames and both backwards
    (with the checkpoints and recomputing them) equal the oracle on the dense copy."""
    mpi, homs, dout = _strided_case(V, 61 + V)
    bstride = 0 if V == 1 else SW * SP * 4
    view = flat.as_strided((V, SH, SW, SP, 4), (bstride, ROW, SP * 4, 4, 1))
    view.copy_(mpi.to(dev))
    assert (SH - 1) * ROW * 4 > 1 << 31
    assert _lib.bwd_layout_ok(view) and not _lib.chunk_layout_ok(view)
    h, d = homs.to(dev), dout.to(dev)
    out, ck = _lib.render_train(view, h)
    assert ck is not None and ck.shape == (V, (SP + 7) // 8, SH, SW, 4)
    assert_bits(out, oracle.render(mpi.numpy(), homs.numpy()), "frames")
    want = oracle.render_backward(mpi.numpy(), homs.numpy(), dout.numpy())
    # lower rows of the gradient come from texels beyond 2^31 bytes only if those were read
    assert np.abs(want[:, 40:]).max() > 0
    got, _ = _backward_flag(view, h, d, dev, ckpt=ck)
    assert_bits(got, want, "with checkpoints")
    got, _ = _backward_flag(view, h, d, dev)
    assert_bits(got, want, "without checkpoints")
    leaf = view.detach().requires_grad_(True)  # the drop-in's autograd on the strided leaf
    pose = configs.f32(configs.config4()["poses"][250:250 + V]).to(dev)
    K = configs.f32([configs.intrinsics_matrix(30.0, 30.0, SW / 2.0, SH / 2.0)] * V).to(dev)
    frames = mv.mpi_render_view_torch(leaf, pose, configs.f32(configs.inv_depths(1, 60, SP)).to(dev), K)
    frames.backward(d)
    assert_bits(leaf.grad, want, "autograd on the strided view")


# ---------------------------------------------------------------------------
# 3. / 4. a dense view above 2 GiB
# ---------------------------------------------------------------------------

BH = BW = 1024
BP = 136


def _big_cameras(dev):
    c = configs.config4()
    pose = configs.f32(c["poses"][7:8])
    planes = configs.f32(configs.inv_depths(1, 100, BP))
    K = configs.f32([c["K"]])
    return pose.to(dev), planes.to(dev), K.to(dev), _host.render_homographies(pose, planes, K, 1).to(dev)


def test_dense_view_above_2_gib_trains(dev, kopts):
    """1024 x 1024 x 136 (2.28 GB, one plane group more than config 4) through mpi_render_view_torch's
    autograd: the frames equal the packed render's; the gradient of the tile path (flag 0), of the bucket
    fallback (flag 1) and of the plane-group schedule in the smallest workspace are bit-identical, with
    the forward's checkpoints and recomputing them."""
    assert BH * BW * BP * 16 >= 0x7FFFFF00
    pose, planes, K, homs = _big_cameras(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    leaf = torch.rand((1, BH, BW, BP, 4), generator=g, device=dev).requires_grad_(True)
    dout = torch.rand((1, BH, BW, 3), generator=g, device=dev) * 2 - 1
    out = mv.mpi_render_view_torch(leaf, pose, planes, K)
    packed = _lib.pack_planes(leaf.detach()[0])
    assert _same_bits(out.detach(), _lib.render_packed(packed, homs)), "frames != the packed render's"
    del packed
    out.backward(dout)
    ref, leaf.grad = leaf.grad, None
    mpi = leaf.detach()
    del out, leaf
    frames, ck = _lib.render_train(mpi, homs)
    assert ck is not None
    del frames
    got, flag = _backward_flag(mpi, homs, dout, dev, ckpt=ck)
    assert flag == 0
    assert _same_bits(got, ref), "tile path: caller workspace != autograd"
    del got
    L = _lib.load()
    n_min = L.mpiv_render_backward_workspace_size_min(BH, BW, BP)
    assert n_min < L.mpiv_render_backward_workspace_size(BH, BW, BP)
    got, flag = _backward_flag(mpi, homs, dout, dev, ckpt=ck, ws_bytes=n_min)
    assert flag == 0
    assert _same_bits(got, ref), "plane groups (smallest workspace) != one group"
    del got, ck
    got, flag = _backward_flag(mpi, homs, dout, dev)
    assert flag == 0
    assert _same_bits(got, ref), "recomputed checkpoints != the forward's"
    del got
    kopts(bwd_fallback=1)
    got, flag = _backward_flag(mpi, homs, dout, dev)
    assert flag == 1
    assert _same_bits(got, ref), "bucket fallback != tile gather"
    del got, ref, mpi
    torch.cuda.empty_cache()


def test_fused_net_output_above_2_gib_equals_two_steps(dev):
    """mpi_render_net_output_torch under autograd at 1024 x 1024 x 136 (its backward re-assembles the
    2.28 GB MPI and reads it in place): frames, d pred and d ref_img equal the two-step form's bits."""
    pose, planes, K, _ = _big_cameras(dev)
    g = torch.Generator(device=dev).manual_seed(19)
    pred = torch.rand((1, 2 * BP + 3, BH, BW), generator=g, device=dev) * 2 - 1
    ref_img = torch.rand((1, BH, BW, 3), generator=g, device=dev) * 2 - 1
    dout = torch.rand((1, BH, BW, 3), generator=g, device=dev) * 2 - 1
    res = []
    for fused in (True, False):
        p, r = pred.clone().requires_grad_(True), ref_img.clone().requires_grad_(True)
        if fused:
            out = mv.mpi_render_net_output_torch(p, r, pose, planes, K)
        else:
            rgba = mv.mpi_from_net_output(p, {"mpi_planes": torch.zeros((1, BP), device=dev), "ref_img": r})
            out = mv.mpi_render_view_torch(rgba, pose, planes, K)
            del rgba
        out.backward(dout)
        res.append((out.detach(), p.grad, r.grad))
        del out, p, r
        torch.cuda.empty_cache()
    for what, a, b in zip(("frames", "d pred", "d ref_img"), *res):
        assert _same_bits(a, b), f"{what}: fused != two-step"
    assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][1].abs().max()) > 0
    del res
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------

def test_wide_training_step_captured_and_replayed_with_new_data(dev, kopts):
    """chunk_wide=1: a 24 x 40 x 9 training step (forward with checkpoints + backward, static inputs)
    captured with torch.cuda.graph on a side stream after a warm-up there, replayed with a second data
    set: frames and gradient equal the oracle (and so the eager run) bit for bit."""
    kopts(chunk_wide=1)
    H, W, P = 24, 40, 9
    planes = configs.f32(configs.inv_depths(1, 100, P))
    K = configs.f32([configs.intrinsics_matrix(38.0, 41.0, W / 2.0, H / 2.0)])
    sets = []
    for k in range(2):
        pose = configs.f32([configs.pose_from(configs.rot_y(2.0 - 5.0 * k), (0.03, -0.02 * k, 0.01))])
        mpi = configs.synthetic_mpi(1, H, W, P, 70 + k)
        dout = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(80 + k)) * 2 - 1
        homs = _host.render_homographies_torch(pose, planes, K, 1)
        sets.append((mpi, pose, dout, oracle.render(mpi.numpy(), homs.numpy()),
                     oracle.render_backward(mpi.numpy(), homs.numpy(), dout.numpy())))
    planes_d, K_d = planes.to(dev), K.to(dev)
    mpi_s = sets[0][0].to(dev).requires_grad_(True)
    pose_s, dout_s = sets[0][1].to(dev), sets[0][2].to(dev)

    def step():
        out = mv.mpi_render_view_torch(mpi_s, pose_s, planes_d, K_d)
        (grad,) = torch.autograd.grad(out, mpi_s, dout_s)
        return out.detach(), grad
    S = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        out, grad = step()  # the warm-up, eager
    torch.cuda.synchronize()
    assert_bits(out, sets[0][3], "eager frames")
    assert_bits(grad, sets[0][4], "eager gradient")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        out, grad = step()
    for k in (1, 0, 1):
        with torch.no_grad():
            mpi_s.copy_(sets[k][0])
        pose_s.copy_(sets[k][1])
        dout_s.copy_(sets[k][2])
        out.fill_(tl.SENT)
        grad.fill_(tl.SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_bits(out, sets[k][3], f"replay with data set {k}: frames")
        assert_bits(grad, sets[k][4], f"replay with data set {k}: gradient")
    del g
