"""GPU tests of the inverse warp's adjoint (warp_bwd.hip, mpiv_inverse_warp_backward) against the
reference's autograd (tests/golden/warpgrad.npz, tools/gen_goldens_warpgrad.py) and against ATen's own
CPU grid_sample backward, and of the public route from there to pose and intrinsics.

Bars.  d img and d depth are the reference's to the bit, zeros' signs and non-finite values included.
dki and dproj are frame sums: golden `w1` has one non-zero term per sum, so they must EQUAL the
reference's; a full frame is held to |got - S64| <= gamma_N * A per entry (N = Ht*Wt, u = 2^-24,
gamma_n = n u / (1 - n u); S64 and A from the reference's own fp32 per-pixel factors), and is the same
bits whatever else runs.  d pose and d K: bit-exact end to end on `w1`; on full frames compared with
the same torch chain in float64 at S64, allowance = the chain's absolute-value Jacobian applied to
gamma_N * A plus gamma_8 times the same products at |S64| (the chain's own fp32 dot products: at most
four terms, two deep)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, assert_bits

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _lib  # noqa: E402

FULL = ["piw", "piw4", "piw2"]
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "warp.npz")))
    g.update(np.load(os.path.join(GOLD, "warpgrad.npz")))
    for k in ("img", "depth"):  # w1: four views of one image and depth map
        g["w1_" + k] = np.repeat(g["w1_" + k], 4, axis=0)
    return g


_MEMO: dict = {}


def inputs(gold, name, dev):
    """(img, depth, ki, proj, dout) on dev; ki and proj are the reference's own inverse(K) and K4 @ pose."""
    if name not in _MEMO:
        _MEMO[name] = tuple(torch.tensor(gold[f"{name}_{k}"]).to(dev) for k in ("img", "depth", "ki", "proj", "dout"))
    return _MEMO[name]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def backward(img, depth, ki, proj, dout, want=(True, True, True, True), **kw):
    return _lib.inverse_warp_backward(img, depth, ki, proj, dout, want, **kw)


def record_calls(monkeypatch):
    names = []
    real = _lib._call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", call)
    return names


# ---------------------------------------------------------------------------
# 1. the goldens
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", FULL + ["w1"])
def test_image_and_depth_gradients_are_the_references_bits(name, gold, dev):
    img, depth, ki, proj, dout = inputs(gold, name, dev)
    leaf_i, leaf_d = img.clone().requires_grad_(), depth.clone().requires_grad_()
    out = _lib.InverseWarpFunction.apply(leaf_i, leaf_d, ki, proj, *depth.shape[1:])
    assert same_bits(out.detach(), _lib.inverse_warp_depthmap(img, depth, ki, proj, *depth.shape[1:]))
    out.backward(dout)
    assert_bits(leaf_d.grad, gold[f"{name}_ddepth"], f"{name} d depth")
    assert_bits(leaf_i.grad, gold[f"{name}_dimg"], f"{name} d img")


def test_single_term_camera_sums_equal_the_reference(gold, dev):
    _, _, dki, dproj = backward(*inputs(gold, "w1", dev))
    for got, what in ((dki, "dki"), (dproj, "dproj")):
        got, want = got.cpu().numpy(), gold[f"w1_{what}"]
        bad = got != want
        assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.size} entries differ, first at {np.argwhere(bad)[0]}: "
                               f"got {got[bad][0]!r}, want {want[bad][0]!r}; pixels {gold['w1_pixels'].tolist()}")
    assert np.abs(dproj[0].cpu().numpy()).max() > 0 and not dproj[3].cpu().numpy().any()
    assert_bits(dproj[:, 12:], np.zeros((4, 4), np.float32), "dproj row 3")


@pytest.mark.parametrize("name", FULL)
def test_full_frame_camera_sums_within_the_summation_bound(name, gold, dev):
    img, depth, ki, proj, dout = inputs(gold, name, dev)
    _, _, dki, dproj = backward(img, depth, ki, proj, dout)
    N = depth.shape[1] * depth.shape[2]
    for got, what in ((dki, "dki"), (dproj, "dproj")):
        got = got.cpu().numpy().astype(np.float64)
        S64, A = gold[f"{name}_{what}_S64"], gold[f"{name}_{what}_A"]
        err = np.abs(got - S64)
        ratio = (err / np.maximum(A * U, 1e-300)).max()
        ref = (np.abs(gold[f"{name}_{what}"].astype(np.float64) - S64) / np.maximum(A * U, 1e-300)).max()
        print(f"{name} {what}: worst |got - S64| = {ratio:.3f} x 2^-24 A (the reference's own: {ref:.3f}; bound "
              f"{gamma(N) / U:.0f})")
        assert np.isfinite(got).all() and A.max() > 0
        assert (err <= gamma(N) * A).all(), f"{name} {what}: worst error {ratio:.1f} x 2^-24 A"
        assert not got[A == 0].any()


@pytest.mark.parametrize("name", ["piw", "piw2"])
def test_camera_sums_are_the_same_bits_whatever_else_runs(name, gold, dev):
    args = inputs(gold, name, dev)
    base = backward(*args)
    runs = {"a second call": backward(*args)[2:], "cameras alone": backward(*args, want=(False, False, True, True))[2:],
            "with d depth": backward(*args, want=(False, True, True, True))[2:],
            "with d img": backward(*args, want=(True, False, True, True))[2:]}
    n = _lib.load().mpiv_inverse_warp_backward_workspace_size(*args[0].shape, *args[1].shape[1:])
    ws = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=dev)  # every stale float a NaN
    full = backward(*args, workspace=ws)
    runs["a 0xFF workspace"] = full[2:]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = backward(*args)
        runs["side stream"] = on_side[2:]
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    alone = backward(*args, want=(False, False, True, False))
    assert alone[0] is None and alone[1] is None and alone[3] is None and same_bits(alone[2], base[2])
    for what, (dki, dproj) in runs.items():
        assert same_bits(dki, base[2]) and same_bits(dproj, base[3]), f"{name}, {what}"
    for got in (full, on_side):
        assert same_bits(got[0], base[0]) and same_bits(got[1], base[1])
    assert_bits(base[0], gold[f"{name}_dimg"], "d img")


# ---------------------------------------------------------------------------
# 2. the public functions
# ---------------------------------------------------------------------------

def public(gold, name, dev, where, grads=(True, True, True, True)):
    """Call the public function of golden case `name` with leaves on `where`; returns (out, leaves)."""
    two = name == "piw2"
    keys = ("img", "depth", "pose", "Ks", "Kt") if two else ("img", "depth", "pose", "K")
    on = list(grads) + [grads[3]]
    ts = []
    for k, g in zip(keys, on):
        t = torch.tensor(gold[f"{name}_{k}"]).to(dev if k in ("img", "depth") else where)
        ts.append(t.requires_grad_(g))
    if two:
        return mv.projective_inverse_warp_torch2(*ts, *(int(v) for v in gold["piw2_tgt"])), ts
    return mv.projective_inverse_warp_torch(*ts), ts


@pytest.mark.parametrize("where", ["device", "host"])
def test_single_pixel_case_is_exact_end_to_end(where, gold, dev):
    out, (img, depth, pose, K) = public(gold, "w1", dev, dev if where == "device" else "cpu")
    out.backward(torch.tensor(gold["w1_dout"]).to(dev))
    assert_bits(img.grad, gold["w1_dimg"], "d img")
    assert_bits(depth.grad, gold["w1_ddepth"], "d depth")
    for got, k in ((pose.grad, "dpose"), (K.grad, "dK")):
        assert got is not None and got.device == pose.device
        bad = got.cpu().numpy() != gold[f"w1_{k}"]
        assert not bad.any(), f"{k}: {int(bad.sum())} entries differ"
    assert float(pose.grad.abs().max()) > 0 and float(K.grad.abs().max()) > 0


def chain64(Ks, Kt, pose):
    """The camera chain of _host.psv_matrices_autograd in float64: (ki [B,9], proj [B,16]) flattened."""
    B = pose.shape[0]
    k4 = torch.cat([torch.cat([Ks, torch.zeros(B, 3, 1, dtype=torch.float64)], 2),
                    torch.tensor([[[0.0, 0.0, 0.0, 1.0]]], dtype=torch.float64).repeat(B, 1, 1)], 1)
    return torch.cat([torch.inverse(Kt).reshape(-1), torch.matmul(k4, pose).reshape(-1)])


@pytest.mark.parametrize("name", FULL)
def test_pose_and_intrinsics_gradients_within_the_chain_bound(name, gold, dev):
    two = name == "piw2"
    out, ts = public(gold, name, dev, dev)
    plain, _ = public(gold, name, dev, dev, grads=(False,) * 4)
    assert same_bits(out.detach(), plain), "the frame differs from the no-grad call's"
    out.backward(torch.tensor(gold[f"{name}_dout"]).to(dev))
    assert_bits(ts[0].grad, gold[f"{name}_dimg"], "d img")
    assert_bits(ts[1].grad, gold[f"{name}_ddepth"], "d depth")
    pose = torch.tensor(gold[f"{name}_pose"]).double()
    Ks = torch.tensor(gold[f"{name}_Ks" if two else f"{name}_K"]).double()
    Kt = torch.tensor(gold[f"{name}_Kt"]).double() if two else Ks
    B = pose.shape[0]
    N = ts[1].shape[1] * ts[1].shape[2]
    if two:
        J = torch.autograd.functional.jacobian(chain64, (Ks, Kt, pose))
        got = {"dKs": ts[3].grad, "dKt": ts[4].grad, "dpose": ts[2].grad}
        Js = {"dKs": J[0], "dKt": J[1], "dpose": J[2]}
    else:
        J = torch.autograd.functional.jacobian(lambda K, p: chain64(K, K, p), (Ks, pose))
        got = {"dK": ts[3].grad, "dpose": ts[2].grad}
        Js = {"dK": J[0], "dpose": J[1]}
    cot = torch.cat([torch.tensor(gold[f"{name}_dki_S64"]).reshape(-1), torch.tensor(gold[f"{name}_dproj_S64"]).reshape(-1)])
    A = torch.cat([torch.tensor(gold[f"{name}_dki_A"]).reshape(-1), torch.tensor(gold[f"{name}_dproj_A"]).reshape(-1)])
    for k, g in got.items():
        Jk = Js[k].reshape(cot.numel(), -1)
        want = (cot @ Jk).reshape(g.shape)
        allow = ((gamma(N) * A + gamma(8) * cot.abs()) @ Jk.abs()).reshape(g.shape)
        err = (g.cpu().double() - want).abs()
        print(f"{name} {k}: worst |got - chain64| / allowance = {float((err / allow.clamp_min(1e-300)).max()):.4f}; "
              f"the reference's own: {float(((torch.tensor(gold[f'{name}_{k}']).double() - want).abs() / allow.clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= allow).all()), f"{name} {k}"
        assert float(g.abs().max()) > 0 and g.device == ts[2].device


def test_each_input_alone_and_nothing_changes_without_a_gradient(gold, dev, monkeypatch):
    """One input requiring grad launches the backward once with only its gradient; with nothing
    requiring grad, or under no_grad, the entries called are today's."""
    dout = torch.tensor(gold["piw_dout"]).to(dev)
    seen = []
    real = _lib._call

    def spy(name, *a):
        if name == "mpiv_inverse_warp_backward":
            seen.append(tuple(p is not None for p in a[14:18]))  # ddepth, dimg, dki, dproj
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", spy)
    for i, (want, what) in enumerate((((False, True, False, False), "img"), ((True, False, False, False), "depth"),
                                      ((False, False, False, True), "pose"), ((False, False, True, True), "K"))):
        grads = tuple(j == i for j in range(4))
        out, ts = public(gold, "piw", dev, dev, grads=grads)
        out.backward(dout)
        assert seen[-1] == want and len(seen) == i + 1, (what, seen)
        for j, t in enumerate(ts):
            assert (t.grad is not None) == (j == i), (what, j)
    monkeypatch.undo()
    names = record_calls(monkeypatch)
    public(gold, "piw", dev, dev, grads=(False,) * 4)
    with torch.no_grad():
        public(gold, "piw", dev, dev)
    public(gold, "piw", dev, "cpu", grads=(False,) * 4)
    assert names == ["mpiv_psv_proj_device", "mpiv_inverse_warp", "mpiv_psv_proj_device", "mpiv_inverse_warp",
                     "mpiv_inverse_warp"], names
    out, _ = public(gold, "piw", dev, dev, grads=(True, True, False, False))
    out.backward(dout)
    assert names[5:] == ["mpiv_psv_proj_device", "mpiv_inverse_warp", "mpiv_inverse_warp_backward"], names


def test_ret_flows_still_raises(gold, dev):
    img, depth = (torch.tensor(gold[f"piw4_{k}"]).to(dev) for k in ("img", "depth"))
    pose, K = (torch.tensor(gold[f"piw4_{k}"]) for k in ("pose", "K"))
    with pytest.raises(RuntimeError, match="ret_flows"):
        mv.projective_inverse_warp_torch(img.requires_grad_(), depth, pose, K, ret_flows=True)


# ---------------------------------------------------------------------------
# 3. ATen itself: d img, and the position gradient through d depth
# ---------------------------------------------------------------------------

def aten(img, depth, ki, proj, dout):
    """ATen's CPU grid_sample backward at the coordinates the project's bit-exact pixel2cam / cam2pixel
    kernels produce: (d img [B,Hs,Ws,C], d grid [B,Ht,Wt,2]) as CPU tensors."""
    dev = img.device
    B, Hs, Ws, C = img.shape
    _, Ht, Wt = depth.shape
    n = Ht * Wt
    ys, xs = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(n)], 0).expand(B, 3, n).contiguous().to(dev)
    cam = torch.empty((B, 4, Ht, Wt), device=dev)
    _lib._call("mpiv_pixel2cam", depth.contiguous(), pc, ki.contiguous(), B, n, 1, cam, _lib._stream(dev))
    pix = _lib.cam2pixel(cam, proj).cpu()
    coords = (pix + torch.tensor([0.5, 0.5])) / torch.tensor([float(Hs), float(Ws)])
    grid = (torch.tensor([-1.0, -1.0]) + 2.0 * coords).requires_grad_()
    leaf = img.detach().cpu().contiguous().requires_grad_()
    out = F.grid_sample(leaf.permute(0, 3, 1, 2), grid, align_corners=False).permute(0, 2, 3, 1)
    out.backward(dout.detach().cpu())
    return leaf.grad, grid.grad


def rand_case(seed, B, Hs, Ws, C, Ht, Wt, dev, spread=1.0):
    """A general camera whose samples cover the source and its surroundings."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, Hs, Ws, C), generator=g)
    depth = torch.rand((B, Ht, Wt), generator=g) * 4 + 1
    dout = torch.rand((B, Ht, Wt, C), generator=g) * 2 - 1
    # the reference's swapped normalisation: x spans Hs, y spans Ws
    ki = torch.tensor([[1.2 * spread * Hs / Wt, 0.01, -0.1 * Hs, 0.02, 1.2 * spread * Ws / Ht, -0.1 * Ws, 0.0, 0.0, 1.0]])
    ki = ki.repeat(B, 1) * (1 + 0.1 * torch.arange(B).reshape(B, 1))
    proj = torch.tensor([[1.0, 0.03, 0.2, 0.5, -0.02, 1.0, 0.1, -0.4, 0.001, 0.002, 1.0, 0.05, 0.0, 0.0, 0.0, 1.0]])
    proj = proj.repeat(B, 1) * (1 + 0.05 * torch.arange(B).reshape(B, 1))
    return [t.to(dev) for t in (img, depth, ki, proj, dout)]


def check_dimg(args, what):
    dimg = backward(*args, want=(True, False, False, False))[0]
    want, _ = aten(*args)
    got = dimg.cpu().numpy()
    nz = float((want != 0).double().mean())
    fin = np.isfinite(want.numpy())
    assert (np.isfinite(got) == fin).all(), f"{what}: non-finite pattern"
    assert_bits(np.where(fin, got, 0), np.where(fin, want.numpy(), 0), f"{what} d img vs ATen")
    return nz


@pytest.mark.parametrize("C", [1, 3, 4, 5])
def test_dimg_is_atens_13x21(C, dev):
    """273 pixels: chunks of 8 wrap rows and the count is no multiple of 64; B = 2 with two cameras."""
    assert check_dimg(rand_case(10 + C, 2, 9, 11, C, 13, 21, dev), f"C={C}") > 0.3


@pytest.mark.parametrize("shape", [(5, 7, 3, 64, 64), (36, 48, 3, 70, 60), (260, 260, 1, 40, 50), (1, 9, 3, 13, 21),
                                   (9, 1, 3, 13, 21)])
def test_dimg_is_atens_shapes(shape, dev):
    """Strong minification (every bucket of a texel interleaves within chunks), a sort over several
    blocks and two digit passes (36x48 source, 70x60 targets), three digit passes (260x260), Hs or Ws = 1."""
    Hs, Ws, C, Ht, Wt = shape
    assert check_dimg(rand_case(sum(shape), 1, Hs, Ws, C, Ht, Wt, dev, spread=0.6 if Hs == 5 else 1.0), str(shape)) > 0


def test_every_pixel_into_one_texel(dev):
    """A depth map of zeros: one bucket of N entries."""
    args = rand_case(3, 1, 9, 11, 3, 13, 21, dev)
    args[1] = torch.zeros_like(args[1])
    args[3] = args[3].clone()
    args[3][:, 3], args[3][:, 7], args[3][:, 11] = 3.3, 4.6, 1.0  # proj's last column: the one sample position
    assert check_dimg(args, "depth 0") > 0
    dimg = backward(*args, want=(True, False, False, False))[0]
    assert int((dimg.abs().sum(-1) != 0).sum()) == 4


def test_nonfinite_and_negative_depths(dev):
    args = rand_case(4, 2, 9, 11, 3, 13, 21, dev)
    d = args[1]
    d[0, 2, 3], d[0, 5, 5], d[1, 0, 0], d[1, 7, 8] = float("nan"), float("inf"), -float("inf"), 0.0
    d[1, 9:12, 4:9] = -1.5
    check_dimg(args, "non-finite depths")


def test_strided_inputs_and_gradients(dev):
    """Strided img and depth, a stride-0 and a permuted dout: the dense tensors' bits, no hidden copy."""
    img, depth, ki, proj, dout = rand_case(5, 2, 9, 11, 3, 13, 21, dev)
    base = backward(img, depth, ki, proj, dout)
    wide_i = torch.zeros((2, 9, 11, 5), device=dev)
    wide_i[..., 1:4] = img
    wide_d = torch.zeros((2, 13, 21 * 2), device=dev)
    wide_d[..., ::2] = depth
    perm = dout.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    assert not perm.is_contiguous()
    got = backward(wide_i[..., 1:4], wide_d[..., ::2], ki, proj, perm)
    for a, b in zip(got, base):
        assert same_bits(a, b)
    ones = torch.ones((), device=dev).expand(2, 13, 21, 3)
    assert ones.stride() == (0, 0, 0, 0)
    for a, b in zip(backward(img, depth, ki, proj, ones), backward(img, depth, ki, proj, ones.contiguous())):
        assert same_bits(a, b)
    leaf = img.clone().requires_grad_()
    _lib.InverseWarpFunction.apply(leaf, depth, ki, proj, 13, 21).sum().backward()
    assert same_bits(leaf.grad, backward(img, depth, ki, proj, ones)[0])


@pytest.mark.parametrize("shape", [(9, 11, 3, 13, 21), (5, 7, 4, 64, 64)])
def test_position_gradient_is_atens_through_ddepth(shape, dev):
    """A camera whose chain after the sampler is exact: proj rows (1,0,0,0), (0,1,0,0), (0,0,0,1), so
    pz = 1, den = 1, du = ax, dv = ay, d cam = (du, dv, +0) and d depth = (ax * rx + ay * ry) + 0 * rz
    with ax = (d grid_x * 2) / Hs, ay = (d grid_y * 2) / Ws: ATen's d grid, four IEEE operations on."""
    Hs, Ws, C, Ht, Wt = shape
    img, depth, ki, _, dout = rand_case(7 + Hs, 2, Hs, Ws, C, Ht, Wt, dev)
    depth = (depth - 1) * 0.2 + 0.2  # in [0.2, 1): most samples inside the source
    ki = ki.clone()
    ki[:, 1], ki[:, 3] = 0.0, 0.0
    proj = torch.tensor([[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1]], device=dev).repeat(2, 1)
    ddepth = backward(img, depth, ki, proj, dout, want=(False, True, False, False))[1]
    _, dgrid = aten(img, depth, ki, proj, dout)
    k = ki.cpu()
    ys, xs = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
    rx = k[:, 0].reshape(2, 1, 1) * xs + k[:, 2].reshape(2, 1, 1)
    ry = k[:, 4].reshape(2, 1, 1) * ys + k[:, 5].reshape(2, 1, 1)
    ax, ay = (dgrid[..., 0] * 2) / float(Hs), (dgrid[..., 1] * 2) / float(Ws)
    want = (ax * rx + ay * ry) + torch.zeros(())
    assert float((want != 0).double().mean()) > 0.3
    assert_bits(ddepth, want.numpy(), "d depth vs ATen's d grid")


# ---------------------------------------------------------------------------
# 4. streams and capture
# ---------------------------------------------------------------------------

def test_arguments_are_validated(dev):
    img, depth, ki, proj, dout = rand_case(8, 1, 9, 11, 3, 13, 21, dev)
    with pytest.raises(RuntimeError, match="workspace"):
        backward(img, depth, ki, proj, dout, workspace=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="nothing to compute"):
        backward(img, depth, ki, proj, dout, want=(False,) * 4)
    L = _lib.load()
    assert L.mpiv_inverse_warp_backward_workspace_size(1, 4, 4, 3, 1 << 16, 1 << 15) == 0
    assert L.mpiv_inverse_warp_backward_workspace_size(1, 1 << 16, 1 << 15, 1, 4, 4) == 0
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="limited to"):  # refused before anything is launched
        _lib._call("mpiv_inverse_warp_backward", img, _lib._strides(img), 1, 9, 11, 3, ki, proj, depth,
                   _lib._strides(depth), 1 << 16, 1 << 15, dout, _lib._strides(dout), depth, None, None, None, ws,
                   ws.numel(), _lib._stream(dev))


def test_captured_forward_and_backward_replay_with_new_data(dev):
    """The img + depth route (device matrices) captured whole on a side stream and replayed with other
    inputs: the eager results' bits on every replay."""
    sets = [rand_case(20, 2, 9, 11, 3, 13, 21, dev), rand_case(21, 2, 9, 11, 3, 13, 21, dev)]

    def step(img, depth, ki, proj, dout):
        li, ld = img.detach().requires_grad_(), depth.detach().requires_grad_()
        out = _lib.InverseWarpFunction.apply(li, ld, ki, proj, 13, 21)
        gi, gd = torch.autograd.grad(out, (li, ld), dout)
        return out.detach(), gi, gd

    want = [step(*s) for s in sets]
    static = [t.clone() for t in sets[1]]
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):  # warm-up on the capture stream
        step(*static)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        res = step(*static)
    for k in (0, 1, 0):
        for dst, src in zip(static, sets[k]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(res, want[k]):
            assert same_bits(a, b), k
    assert not same_bits(want[0][1], want[1][1])


def test_public_call_with_device_cameras_is_capturable(gold, dev):
    """projective_inverse_warp_torch with img and depth requiring grad and pose / K in HBM (the no-grad device
    route of the matrices): forward + backward captured and replayed with new images, depths and poses."""
    img, depth, dout = (torch.tensor(gold[f"piw_{k}"]).to(dev) for k in ("img", "depth", "dout"))
    pose, K = (torch.tensor(gold[f"piw_{k}"]).to(dev) for k in ("pose", "K"))
    pose2 = pose.clone()
    pose2[:, :3, 3] += 0.05
    sets = [(img, depth, pose, dout), (img.flip(2).contiguous(), depth * 1.25, pose2, dout * -0.5)]

    def step(img, depth, pose, dout):
        li, ld = img.detach().requires_grad_(), depth.detach().requires_grad_()
        out = mv.projective_inverse_warp_torch(li, ld, pose, K)
        return (out.detach(),) + torch.autograd.grad(out, (li, ld), dout)

    want = [step(*s) for s in sets]
    assert_bits(want[0][1], gold["piw_dimg"], "d img")
    static = [t.clone() for t in sets[1]]
    S = torch.cuda.Stream(dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(S):  # warm-up on the capture stream (memoises inverse(K))
        step(*static)
    torch.cuda.current_stream(dev).wait_stream(S)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        res = step(*static)
    for k in (0, 1, 0):
        for dst, src in zip(static, sets[k]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(res, want[k]):
            assert same_bits(a, b), k


def test_camera_route_raises_under_capture(gold, dev, monkeypatch):
    img, depth = (torch.tensor(gold[f"piw4_{k}"]).to(dev) for k in ("img", "depth"))
    pose, K = (torch.tensor(gold[f"piw4_{k}"]).to(dev) for k in ("pose", "K"))
    pose.requires_grad_()
    torch.cuda.synchronize()

    def refuse(name, *a):
        raise AssertionError(f"{name} was called: the error must be raised before any launch")
    monkeypatch.setattr(_lib, "_call", refuse)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        mv.projective_inverse_warp_torch(img, depth, pose, K)
