"""GPU tests of the sampler's and the compositor's adjoints (helper_bwd.hip: mpiv_grid_sample_backward,
mpiv_over_composite_backward) against the reference's autograd (tests/golden/helpergrad.npz,
tools/gen_goldens_helpergrad.py), against ATen's own CPU grid_sample backward and against torch's CPU
autograd of the reference's over_composite formula.

Bars.  Every gradient is the CPU's to the bit, zeros' signs included; where the CPU's value is not finite
the pattern (NaN, +inf, -inf) must be equal and the rest equal to the bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, REPO, assert_bits

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _lib, configs  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_goldens_helpergrad as gen  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "helpergrad.npz")))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_pattern_and_bits(got, want, what):
    """Equal non-finite pattern, and the finite values equal to the bit."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN pattern"
    inf = np.isinf(want)
    assert (np.isinf(got) == inf).all() and (got[inf] == want[inf]).all(), f"{what}: inf pattern"
    fin = np.isfinite(want)
    assert_bits(np.where(fin, got, 0), np.where(fin, want, 0), what)


def record_calls(monkeypatch):
    names = []
    real = _lib._call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", call)
    return names


# ---------------------------------------------------------------------------
# 1. the sampler: goldens
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bw", "rs"])
def test_sampler_goldens_through_the_public_helpers(name, gold, dev):
    imgs, coords, dout = (t.to(dev) for t in gen.helper_inputs(name))
    fn = mv.bilinear_wrapper_torch if name == "bw" else mv.resampler_wrapper_torch
    li, lc = imgs.clone().requires_grad_(), coords.clone().requires_grad_()
    out = fn(li, lc)
    assert out.grad_fn is not None and same_bits(out.detach(), fn(imgs, coords))
    assert_bits(out, gold[f"{name}_out"], f"{name} out")
    out.backward(dout)
    for got, k in ((li.grad, "dimgs"), (lc.grad, "dcoords")):
        assert (gold[f"{name}_{k}"] != 0).mean() > 0.3, k
        assert_bits(got, gold[f"{name}_{k}"], f"{name} {k}")


# ---------------------------------------------------------------------------
# 2. the sampler: ATen itself
# ---------------------------------------------------------------------------

def aten(imgs, coords, dout):
    """ATen's CPU grid_sample autograd of the reference's wrapper at the same coordinates, everything
    channels-last: (d imgs [N,Hi,Wi,C], d coords [N,Ho,Wo,2]) as CPU tensors."""
    li = imgs.detach().cpu().contiguous().requires_grad_()
    lc = coords.detach().cpu().contiguous().requires_grad_()
    out = F.grid_sample(li.permute(0, 3, 1, 2), torch.tensor([-1.0, -1.0]) + 2.0 * lc, align_corners=False)
    out.permute(0, 2, 3, 1).backward(dout.detach().cpu())
    return li.grad, lc.grad


def backward(imgs, coords, dout, want=(True, True), **kw):
    return _lib.grid_sample_backward(imgs, coords, dout, True, want, **kw)


def rand_case(seed, N, Hi, Wi, C, Ho, Wo, dev):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand((N, Hi, Wi, C), generator=g)
    coords = torch.rand((N, Ho, Wo, 2), generator=g) * 1.5 - 0.25
    dout = torch.rand((N, Ho, Wo, C), generator=g) * 2 - 1
    return [t.to(dev) for t in (imgs, coords, dout)]


def check(args, what):
    """Both gradients against ATen; returns the non-zero shares of ATen's (d imgs, d coords)."""
    dimgs, dcoords = backward(*args)
    want_i, want_c = aten(*args)
    assert_pattern_and_bits(dimgs, want_i, f"{what} d imgs vs ATen")
    assert_pattern_and_bits(dcoords, want_c, f"{what} d coords vs ATen")
    return float((want_i != 0).double().mean()), float((want_c != 0).double().mean())


@pytest.mark.parametrize("C", [1, 3, 4, 5])
def test_sampler_is_atens_13x21(C, dev):
    """273 pixels: chunks of 8 wrap rows and the count is no multiple of 64."""
    nz = check(rand_case(10 + C, 2, 9, 11, C, 13, 21, dev), f"C={C}")
    assert min(nz) > 0.3, nz


@pytest.mark.parametrize("shape", [(36, 48, 3, 70, 60), (260, 260, 1, 40, 50), (1, 9, 3, 13, 21), (9, 1, 3, 13, 21)])
def test_sampler_is_atens_shapes(shape, dev):
    """A sort over several blocks and two digit passes (36x48 source, 70x60 targets), three digit passes
    (260x260), Hs or Ws = 1."""
    Hi, Wi, C, Ho, Wo = shape
    nz = check(rand_case(sum(shape), 1, Hi, Wi, C, Ho, Wo, dev), str(shape))
    assert min(nz) > 0, nz


def test_every_coordinate_into_one_texel(dev):
    args = rand_case(3, 1, 9, 11, 3, 13, 21, dev)
    args[1] = torch.tensor([0.4, 0.55], device=dev).expand(1, 13, 21, 2).contiguous()
    assert min(check(args, "one texel")) > 0
    dimgs = backward(*args, want=(True, False))[0]
    assert int((dimgs.abs().sum(-1) != 0).sum()) == 4


def test_nonfinite_and_far_outside_coordinates(dev):
    args = rand_case(4, 2, 9, 11, 3, 13, 21, dev)
    c = args[1]
    c[0, 2, 3, 0], c[0, 5, 5, 1], c[1, 0, 0, 0], c[1, 7, 8, 1] = float("nan"), float("inf"), -float("inf"), float("nan")
    c[0, 6, 6], c[0, 6, 7] = float("inf"), float("nan")
    c[1, 9, 4], c[1, 9, 5, 0], c[1, 9, 6, 1], c[1, 9, 7] = 1e30, -1e30, 3e9, -7.0
    c[1, 10, 4:9] = torch.tensor([-1.0 / 11, 12.0 / 11], device=dev)  # the corner just outside
    check(args, "non-finite coordinates")


def test_strided_inputs_and_cotangents(dev):
    """Strided imgs and coords, a permuted and a stride-0 dout: the dense tensors' bits."""
    imgs, coords, dout = rand_case(5, 2, 9, 11, 3, 13, 21, dev)
    base = backward(imgs, coords, dout)
    wide_i = torch.zeros((2, 9, 11, 5), device=dev)
    wide_i[..., 1:4] = imgs
    wide_c = torch.zeros((2, 13, 21 * 2, 3), device=dev)
    wide_c[:, :, ::2, 1:] = coords
    perm = dout.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    assert not perm.is_contiguous()
    for a, b in zip(backward(wide_i[..., 1:4], wide_c[:, :, ::2, 1:], perm), base):
        assert same_bits(a, b)
    ones = torch.ones((), device=dev).expand(2, 13, 21, 3)
    assert ones.stride() == (0, 0, 0, 0)
    for a, b in zip(backward(imgs, coords, ones), backward(imgs, coords, ones.contiguous())):
        assert same_bits(a, b)
    li, lc = imgs.clone().requires_grad_(), coords.clone().requires_grad_()
    mv.resampler_wrapper_torch(li, lc).sum().backward()
    want = backward(imgs, coords, ones)
    assert same_bits(li.grad, want[0]) and same_bits(lc.grad, want[1])
    # bilinear_wrapper_torch's [..., C, Ht, Wt] output: a permuted cotangent of a strided leaf
    li = wide_i[..., 1:4].reshape(2, 1, 9, 11, 3).detach().requires_grad_()
    out = mv.bilinear_wrapper_torch(li, coords.reshape(2, 1, 13, 21, 2))
    assert out.shape == (2, 1, 3, 13, 21)
    out.backward(dout.permute(0, 3, 1, 2).reshape(2, 1, 3, 13, 21))
    assert li.grad.shape == li.shape and same_bits(li.grad.reshape(2, 9, 11, 3), base[0])


def test_each_gradient_alone_launches_only_its_own_kernels(dev, monkeypatch):
    imgs, coords, dout = rand_case(6, 2, 9, 11, 3, 13, 21, dev)
    base = backward(imgs, coords, dout)
    alone_i, none = backward(imgs, coords, dout, want=(True, False))
    assert none is None and same_bits(alone_i, base[0])
    none, alone_c = backward(imgs, coords, dout, want=(False, True))
    assert none is None and same_bits(alone_c, base[1])
    # d coords alone writes no positions or keys and sorts nothing: the workspace is untouched (and optional)
    n = _lib.load().mpiv_grid_sample_backward_workspace_size(2, 3, 9, 11, 13, 21)
    ws = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    dco = torch.empty((2, 13, 21, 2), device=dev)
    _lib._call("mpiv_grid_sample_backward", imgs, _lib._strides(imgs, (0, 3, 1, 2)), 2, 3, 9, 11, coords,
               _lib._strides(coords), 13, 21, dout, _lib._strides(dout, (0, 3, 1, 2)), None, dco, ws, n, _lib._stream(dev))
    assert same_bits(dco, base[1]) and bool((ws == 0xA5).all())
    with pytest.raises(RuntimeError, match="nothing to compute"):
        backward(imgs, coords, dout, want=(False, False))
    with pytest.raises(RuntimeError, match="workspace"):
        backward(imgs, coords, dout, workspace=torch.empty(64, dtype=torch.uint8, device=dev))
    # autograd asks for what needs_input_grad says
    seen = []
    real = _lib._call

    def spy(name, *a):
        if name == "mpiv_grid_sample_backward":
            seen.append((a[12] is not None, a[13] is not None))  # din, dcoords
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", spy)
    for gi, gc in ((True, False), (False, True), (True, True)):
        li, lc = imgs.clone().requires_grad_(gi), coords.clone().requires_grad_(gc)
        mv.resampler_wrapper_torch(li, lc).backward(dout)
        assert seen[-1] == (gi, gc) and (li.grad is not None) == gi and (lc.grad is not None) == gc
    assert len(seen) == 3


def test_side_stream_and_poisoned_workspace(dev):
    imgs, coords, dout = rand_case(7, 2, 36, 48, 3, 70, 60, dev)
    base = backward(imgs, coords, dout)
    n = _lib.load().mpiv_grid_sample_backward_workspace_size(2, 3, 36, 48, 70, 60)
    ws = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=dev)  # every stale float a NaN
    for a, b in zip(backward(imgs, coords, dout, workspace=ws), base):
        assert same_bits(a, b)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = backward(imgs, coords, dout)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(on_side, base):
        assert same_bits(a, b)


def test_captured_forward_and_backward_replay_with_new_data(dev):
    sets = [rand_case(20, 2, 9, 11, 3, 13, 21, dev), rand_case(21, 2, 9, 11, 3, 13, 21, dev)]

    def step(imgs, coords, dout):
        li, lc = imgs.detach().requires_grad_(), coords.detach().requires_grad_()
        out = mv.resampler_wrapper_torch(li, lc)
        return (out.detach(),) + torch.autograd.grad(out, (li, lc), dout)

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


def test_plane_warp_helpers_are_differentiable_in_imgs(dev, monkeypatch):
    """projective_forward_homography_torch -> planar_transform_torch -> transform_plane_imgs_torch: d imgs
    is the sampler route's at the coordinates the warp computed."""
    g = torch.Generator().manual_seed(31)
    P, B, H, W = 3, 2, 12, 16
    layers = torch.rand((P, B, H, W, 4), generator=g).to(dev)
    dout = (torch.rand((P, B, 4, H, W), generator=g) * 2 - 1).to(dev)
    K = configs.f32([configs.intrinsics_matrix(14.0, 13.0, W / 2.0, H / 2.0)] * B).to(dev)
    pose = configs.f32([configs.pose_from(configs.rot_y(3.0), (0.05, -0.02, 0.03)),
                        configs.pose_from(configs.rot_y(-2.0), (-0.04, 0.01, 0.02))]).to(dev)
    depths = torch.tensor([4.0, 2.0, 1.0]).reshape(-1, 1).repeat(1, B).to(dev)
    plain = mv.projective_forward_homography_torch(layers, K, pose, depths)
    seen = []
    real = _lib.bilinear_sample

    def spy(imgs, coords, channels_last_out):
        seen.append(coords)
        return real(imgs, coords, channels_last_out)
    monkeypatch.setattr(_lib, "bilinear_sample", spy)
    leaf = layers.clone().requires_grad_()
    out = mv.projective_forward_homography_torch(leaf, K, pose, depths)
    assert out.grad_fn is not None and same_bits(out.detach(), plain)
    out.backward(dout)
    monkeypatch.undo()
    coords = seen[-1]
    assert not coords.requires_grad and coords.shape == (P, B, H, W, 2)
    direct = layers.clone().requires_grad_()
    mv.bilinear_wrapper_torch(direct, coords).backward(dout)
    assert same_bits(leaf.grad, direct.grad) and float((leaf.grad != 0).float().mean()) > 0.3
    want, _ = aten(layers.reshape(P * B, H, W, 4), coords.reshape(P * B, H, W, 2),
                   dout.reshape(P * B, 4, H, W).permute(0, 2, 3, 1))
    assert_bits(leaf.grad.reshape(P * B, H, W, 4), want.numpy(), "d imgs vs ATen")


# ---------------------------------------------------------------------------
# 3. the compositor
# ---------------------------------------------------------------------------

def cpu_over(layers, dout):
    """torch's CPU autograd of the reference's over_composite formula (utils.py:147-157) over `layers`
    (CPU tensors; the same tensor may appear twice): (out, leaves' gradients are left on the leaves)."""
    for i, t in enumerate(layers):
        rgb, alpha = t[..., 0:3], t[..., 3:]
        if i == 0:
            output = rgb
        else:
            rgb_by_alpha = rgb * alpha
            output = rgb_by_alpha + output * (1.0 - alpha)
    output.backward(dout)
    return output.detach()


def over_case(seed, P, dev, shape=(2, 13, 21)):
    g = torch.Generator().manual_seed(seed)
    stack = torch.rand((P,) + shape + (4,), generator=g) * 1.5 - 0.25
    pick = torch.rand((P,) + shape, generator=g)
    stack[..., 3] = torch.where(pick < 0.02, torch.zeros(()), torch.where(pick > 0.98, torch.ones(()), stack[..., 3]))
    dout = torch.rand(shape + (3,), generator=g) * 2 - 1
    dout[0, 0], dout[0, 1] = 0.0, -0.0
    return stack, dout


@pytest.mark.parametrize("P", gen.OVER_P)
def test_compositor_goldens(P, gold, dev):
    layers, dout = gen.over_inputs(P)
    leaves = [t.to(dev).requires_grad_() for t in layers]
    out = mv.over_composite(leaves)
    assert out.grad_fn is not None
    assert_bits(out, gold[f"oc{P}_out"], f"P={P} out")
    out.backward(dout.to(dev))
    block = torch.stack([t.grad for t in leaves]).cpu()
    assert float((block != 0).double().mean()) > 0.3
    if P <= 2:
        assert_bits(block, gold[f"oc{P}_dlayers"], f"P={P} d layers")
    else:
        assert_bits(block[0], gold[f"oc{P}_d0"], f"P={P} d layer 0")
        assert_bits(block[-1], gold[f"oc{P}_dlast"], f"P={P} d layer {P - 1}")
        # the layers between: this host's CPU autograd, held to the reference's recorded digest
        cpu = [t.clone().requires_grad_() for t in layers]
        cpu_over(cpu, dout)
        want = torch.stack([t.grad for t in cpu])
        assert gen.sha(want) == str(gold[f"oc{P}_dsha"]), "this host's CPU autograd is not the recorded one"
        assert_bits(block, want.numpy(), f"P={P} d layers")
    assert gen.sha(block) == str(gold[f"oc{P}_dsha"])


@pytest.mark.parametrize("P", [1, 2, 8, 9, 10, 17, 33])
def test_compositor_is_cpu_autograd(P, dev):
    stack, dout = over_case(40 + P, P, dev)
    cpu = [stack[p].clone().requires_grad_() for p in range(P)]
    want_out = cpu_over(cpu, dout)
    leaves = [stack[p].to(dev).requires_grad_() for p in range(P)]
    out = mv.over_composite(leaves)
    assert_bits(out, want_out.numpy(), f"P={P} out")
    out.backward(dout.to(dev))
    for p in range(P):
        assert_bits(leaves[p].grad, cpu[p].grad.numpy(), f"P={P} d layer {p}")
    # the entry itself: a poisoned workspace, a stride-0 cotangent
    n = _lib.load().mpiv_over_composite_backward_workspace_size(P, 2 * 13 * 21)
    ws = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=dev)
    block = _lib.over_composite_backward([t.detach() for t in leaves], dout.to(dev), workspace=ws)
    assert same_bits(block, torch.stack([t.grad for t in leaves]))
    ones = torch.ones((), device=dev).expand(2, 13, 21, 3)
    assert same_bits(_lib.over_composite_backward([t.detach() for t in leaves], ones),
                     _lib.over_composite_backward([t.detach() for t in leaves], ones.contiguous()))


def test_compositor_layouts(dev):
    """Channel slices of a wider tensor (scalar route), views of one [B,H,W,P,4] tensor (16-B route, one
    leaf), one tensor listed twice, layers of differing strides (contiguous copies)."""
    P = 10
    stack, dout = over_case(60, P, dev)
    d = dout.to(dev)
    cpu = [stack[p].clone().requires_grad_() for p in range(P)]
    cpu_over(cpu, dout)
    want = torch.stack([t.grad for t in cpu]).numpy()
    # channel slices of a wider tensor, views of one [B,H,W,P,4] tensor: one leaf, whose gradient autograd
    # sums from the layers' zero-padded ones (on the CPU alike: a -0 of layer 0 becomes +0 there)
    wide = torch.zeros((P, 2, 13, 21, 6))
    wide[..., 1:5] = stack
    for what, base, views in (("channel slices", wide, lambda t: [t[p][..., 1:5] for p in range(P)]),
                              ("views of one MPI", stack.permute(1, 2, 3, 0, 4).contiguous(),
                               lambda t: [t[:, :, :, p] for p in range(P)])):
        ref = base.clone().requires_grad_()
        cpu_over(views(ref), dout)
        leaf = base.to(dev).requires_grad_()
        mv.over_composite(views(leaf)).backward(d)
        assert_bits(leaf.grad, ref.grad.numpy(), what)
        assert float((ref.grad != 0).float().mean()) > 0.3
    assert_bits(ref.grad.permute(3, 0, 1, 2, 4) + 0, want + np.float32(0), "the one-leaf sum but for zeros' signs")
    # layers of differing strides
    leaves = [stack[p].to(dev).requires_grad_() for p in range(P)]
    odd = torch.zeros((2, 13, 21, 8), device=dev)
    odd[..., ::2] = stack[3].to(dev)
    odd.requires_grad_()
    mixed = list(leaves)
    mixed[3] = odd[..., ::2]
    mv.over_composite(mixed).backward(d)
    for p in range(P):
        got = odd.grad[..., ::2] if p == 3 else leaves[p].grad
        assert_bits(got, want[p], f"differing strides, layer {p}")
    # dense layers of which one starts 4 bytes off a 16-B boundary: its loads go scalar inside the 16-B kernel
    leaves = [stack[p].to(dev).requires_grad_() for p in range(P)]
    buf = torch.zeros(2 * 13 * 21 * 4 + 1, device=dev)
    buf[1:] = stack[4].to(dev).reshape(-1)
    buf.requires_grad_()
    off = list(leaves)
    off[4] = buf[1:].view(2, 13, 21, 4)
    assert off[4].data_ptr() % 16 == 4 and off[4].stride() == leaves[0].stride()
    mv.over_composite(off).backward(d)
    for p in range(P):
        got = buf.grad[1:].view(2, 13, 21, 4) if p == 4 else leaves[p].grad
        assert_bits(got, want[p], f"unaligned layer, layer {p}")
    # one tensor listed twice (as layers 2 and 7)
    twice_cpu = [stack[p].clone().requires_grad_() for p in range(P)]
    order = list(range(P))
    order[7] = 2
    cpu_over([twice_cpu[p] for p in order], dout)
    leaves = [stack[p].to(dev).requires_grad_() for p in range(P)]
    mv.over_composite([leaves[p] for p in order]).backward(d)
    assert leaves[7].grad is None and twice_cpu[7].grad is None
    for p in range(P):
        if p != 7:
            assert_bits(leaves[p].grad, twice_cpu[p].grad.numpy(), f"listed twice, layer {p}")


def test_compositor_nonfinite_layers(dev):
    P = 12
    stack, dout = over_case(61, P, dev)
    stack[2, 0, 3, 4, 0], stack[5, 0, 3, 5, 3], stack[9, 1, 2, 2, 1] = float("inf"), float("nan"), -float("inf")
    stack[11, 1, 6, 6, 3], stack[0, 1, 7, 7, 2] = float("inf"), float("nan")
    cpu = [stack[p].clone().requires_grad_() for p in range(P)]
    want_out = cpu_over(cpu, dout)
    leaves = [stack[p].to(dev).requires_grad_() for p in range(P)]
    out = mv.over_composite(leaves)
    assert_pattern_and_bits(out, want_out, "out")
    out.backward(dout.to(dev))
    assert not bool(torch.isfinite(torch.stack([t.grad for t in cpu])).all())
    for p in range(P):
        assert_pattern_and_bits(leaves[p].grad, cpu[p].grad, f"d layer {p}")


def test_compositor_raises_under_capture_before_any_launch(dev, monkeypatch):
    layers = [torch.rand((1, 4, 4, 4), device=dev).requires_grad_() for _ in range(3)]
    torch.cuda.synchronize()

    def refuse(name, *a):
        raise AssertionError(f"{name} was called: the error must be raised before any launch")
    monkeypatch.setattr(_lib, "_call", refuse)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="HIP-graph capture"):
        mv.over_composite(layers)


# ---------------------------------------------------------------------------
# 4. nothing changes without a gradient
# ---------------------------------------------------------------------------

def test_nothing_changes_without_a_gradient(dev, monkeypatch):
    imgs, coords, dout = rand_case(8, 2, 9, 11, 3, 13, 21, dev)
    stack, _ = over_case(62, 10, dev)
    layers = [stack[p].to(dev) for p in range(10)]
    want_s, want_o = mv.resampler_wrapper_torch(imgs, coords), mv.over_composite(layers)
    names = record_calls(monkeypatch)
    a = mv.resampler_wrapper_torch(imgs, coords)
    b = mv.bilinear_wrapper_torch(imgs[:, None], coords[:, None])
    c = mv.over_composite(layers)
    with torch.no_grad():
        d = mv.resampler_wrapper_torch(imgs.clone().requires_grad_(), coords.clone().requires_grad_())
        e = mv.over_composite([t.clone().requires_grad_() for t in layers])
    assert names == ["mpiv_grid_sample", "mpiv_grid_sample", "mpiv_over_composite", "mpiv_grid_sample",
                     "mpiv_over_composite"], names
    for t in (a, b, c, d, e):
        assert t.grad_fn is None and not t.requires_grad
    assert same_bits(a, want_s) and same_bits(d, want_s) and same_bits(b[:, 0].permute(0, 2, 3, 1), want_s)
    assert same_bits(c, want_o) and same_bits(e, want_o)
    del names[:]
    li = imgs.clone().requires_grad_()
    out = mv.resampler_wrapper_torch(li, coords)
    assert same_bits(out.detach(), want_s)
    out.backward(dout)
    leaves = [t.clone().requires_grad_() for t in layers[:1]] + layers[1:]
    out = mv.over_composite(leaves)
    assert same_bits(out.detach(), want_o)
    out.sum().backward()
    assert names == ["mpiv_grid_sample", "mpiv_grid_sample_backward", "mpiv_over_composite",
                     "mpiv_over_composite_backward"], names
    assert leaves[0].grad is not None and all(t.grad is None for t in leaves[1:])
