"""GPU tests of the plane sweep's adjoint (psv_bwd.hip, mpiv_plane_sweep_backward) against the reference's
autograd (tests/golden/psvgrad.npz, tools/gen_goldens_psvgrad.py), against the inverse warp's adjoint it is
composed of, and against ATen's own CPU grid_sample backward.

Bars.  d img is the reference's to the bit: per depth ATen's accumulation order, the depths added in
descending d (the goldens' ascending fold differs in >= 1 % of the elements, so the order is checked).
ddepths, dki and dproj are sums: |got - S64| <= gamma_N * A per entry (u = 2^-24, gamma_n = n u / (1 - n u);
S64 and A from the reference's own fp32 per-pixel terms), N the number of terms: B*Ht*Wt per depth for
ddepths, D*Ht*Wt per view for the camera sums; and they are the same bits whatever else runs and however
the planes are grouped.  d pose and d K: compared with the same torch chain in float64 at S64, allowance =
the chain's absolute-value Jacobian applied to gamma_N * A plus gamma_8 times the same products at |S64|
(tests/test_warpgrad_gpu.py's bound; the network input's chain has the relative pose's inverse and matmul
in front of it, four dot products of at most four terms deep: gamma_16)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, assert_bits

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _lib  # noqa: E402

CASES = ["psv", "psv1", "psv33", "one2"]
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "psvgrad.npz")))
    for k in ("img", "pose", "K"):  # psv1: psv's inputs, its first depth and the first C channels of its dout
        g["psv1_" + k] = g["psv_" + k]
    g["psv1_depths"] = g["psv_depths"][:1]
    g["psv1_dout"] = np.ascontiguousarray(g["psv_dout"][..., :3])
    return g


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def T(gold, key, dev):
    return torch.tensor(gold[key]).to(dev)


def inputs(gold, name, dev):
    """(img [B,Hs,Ws,C], depths [D], ki, proj, dout) on dev; ki and proj are the reference's own."""
    img = T(gold, f"{name}_img", dev)
    return (img if img.dim() == 4 else img[None],) + tuple(T(gold, f"{name}_{k}", dev) for k in ("depths", "ki", "proj", "dout"))


def backward(img, depths, ki, proj, dout, want=(True, True, True, True), **kw):
    return _lib.plane_sweep_backward(img, depths, ki, proj, dout, want, **kw)


def public(gold, name, dev, where, grads=(True, True, True, True), depths_as_list=False):
    """Call the public function of golden case `name`; leaves: img, depths, pose, K (one2: Ks, Kt)."""
    two = name == "one2"
    keys = ("img", "depths", "pose", "Ks", "Kt") if two else ("img", "depths", "pose", "K")
    on = list(grads) + [grads[3]]
    ts = []
    for k, g in zip(keys, on):
        t = T(gold, f"{name}_{k}", dev if k in ("img", "depths") else where)
        ts.append(t.requires_grad_(g))
    args = list(ts)
    if depths_as_list:
        args[1] = [float(v) for v in gold[f"{name}_depths"]]
    if two:
        return mv.plane_sweep_torch_one2(*args, *(int(v) for v in gold["one2_tgt"])), ts
    return mv.plane_sweep_torch(*args), ts


def check_sum(got, S64, A, n, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(S64.shape)
    err = np.abs(got - S64)
    print(f"{what}: worst |got - S64| = {(err / np.maximum(A * U, 1e-300)).max():.3f} x 2^-24 A (bound {gamma(n) / U:.0f})")
    assert np.isfinite(got).all() and A.max() > 0
    assert (err <= gamma(n) * A).all(), what
    assert not got[A == 0].any(), what


def check_chain(chain, leaves64, got, cot, A, n, g_chain, what):
    """got: the gradients (in the order of leaves64) vs the float64 chain at cot, within the allowance."""
    J = torch.autograd.functional.jacobian(chain, tuple(leaves64))
    for k, (g, Jk) in enumerate(zip(got, J)):
        Jk = Jk.reshape(cot.numel(), -1)
        want = (cot @ Jk).reshape(g.shape)
        allow = ((gamma(n) * A + gamma(g_chain) * cot.abs()) @ Jk.abs()).reshape(g.shape)
        err = (g.detach().cpu().double() - want).abs()
        print(f"{what}[{k}]: worst |got - chain64| / allowance = {float((err / allow.clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= allow).all()) and float(g.abs().max()) > 0, f"{what}[{k}]"


def chain64(Ks, Kt, pose):
    """The camera chain of _host.psv_matrices_autograd in float64: (ki [B,9], proj [B,16]) flattened."""
    B = pose.shape[0]
    k4 = torch.cat([torch.cat([Ks, torch.zeros(B, 3, 1, dtype=torch.float64)], 2),
                    torch.tensor([[[0.0, 0.0, 0.0, 1.0]]], dtype=torch.float64).repeat(B, 1, 1)], 1)
    return torch.cat([torch.inverse(Kt).reshape(-1), torch.matmul(k4, pose).reshape(-1)])


# ---------------------------------------------------------------------------
# 1. the goldens through the public functions
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_public_call_matches_the_goldens(name, gold, dev):
    two = name == "one2"
    out, ts = public(gold, name, dev, dev)
    assert out.grad_fn is not None, "the volume has no grad_fn"
    plain, _ = public(gold, name, dev, dev, grads=(False,) * 4)
    assert same_bits(out.detach(), plain), "the volume differs from the no-grad call's"
    dout = T(gold, f"{name}_dout", dev)
    out.backward(dout)
    assert_bits(ts[0].grad, gold[f"{name}_dimg"], f"{name} d img")
    D = len(gold[f"{name}_depths"])
    B, Ht, Wt = dout.shape[:3]
    N = Ht * Wt
    check_sum(ts[1].grad, gold[f"{name}_ddepths_S64"], gold[f"{name}_ddepths_A"], B * N, f"{name} ddepths")
    _, _, dki, dproj = backward(*inputs(gold, name, dev), want=(False, False, True, True))
    for g, what in ((dki, "dki"), (dproj, "dproj")):
        check_sum(g, gold[f"{name}_{what}_S64"], gold[f"{name}_{what}_A"], D * N, f"{name} {what}")
    assert_bits(dproj[:, 12:], np.zeros((B, 4), np.float32), "dproj row 3")
    b3 = lambda k: torch.tensor(gold[f"{name}_{k}"]).double().reshape(B, *gold[f"{name}_{k}"].shape[-2:])  # noqa: E731
    cot = torch.cat([torch.tensor(gold[f"{name}_dki_S64"]).reshape(-1), torch.tensor(gold[f"{name}_dproj_S64"]).reshape(-1)])
    A = torch.cat([torch.tensor(gold[f"{name}_dki_A"]).reshape(-1), torch.tensor(gold[f"{name}_dproj_A"]).reshape(-1)])
    if two:
        got = [t.grad.reshape(1, *t.shape) for t in (ts[3], ts[4], ts[2])]
        check_chain(chain64, (b3("Ks"), b3("Kt"), b3("pose")), got, cot, A, D * N, 8, f"{name} dKs/dKt/dpose")
    else:
        check_chain(lambda K, p: chain64(K, K, p), (b3("K"), b3("pose")), [ts[3].grad, ts[2].grad], cot, A, D * N, 8,
                    f"{name} dK/dpose")
    for t in ts:
        assert t.grad is not None and t.grad.device == t.device and t.grad.shape == t.shape


def test_batched_one_is_the_sweep_of_a_batch_of_one(gold, dev):
    """plane_sweep_torch_one: the unbatched form, host cameras requiring grad, a list of depths."""
    img, pose, K = (T(gold, f"psv33_{k}", dev if k == "img" else "cpu")[0] for k in ("img", "pose", "K"))
    depths = [float(v) for v in gold["psv33_depths"]]
    leaves = [img.requires_grad_(), pose.requires_grad_(), K.requires_grad_()]
    out = mv.plane_sweep_torch_one(leaves[0], depths, leaves[1], leaves[2])
    out.backward(T(gold, "psv33_dout", dev))
    assert_bits(leaves[0].grad, gold["psv33_dimg"][0], "d img")
    assert leaves[1].grad.shape == (4, 4) and leaves[2].grad.shape == (3, 3) and float(leaves[1].grad.abs().max()) > 0


def fni_leaves(gold, dev, grads=True, cams_on=None):
    keys = ("ref", "src", "ref_pose", "src_poses", "depths", "K")
    ts = {k: T(gold, f"fni_{k}", dev if k in ("ref", "src") or cams_on is None else cams_on) for k in keys}
    for t in ts.values():
        t.requires_grad_(grads)
    return ts


def fni_call(ts):
    return mv.format_network_input_torch(None, ts["ref"], ts["src"], ts["ref_pose"], ts["src_poses"], ts["depths"], ts["K"])


def test_network_input_matches_the_goldens(gold, dev):
    ts = fni_leaves(gold, dev)
    out = fni_call(ts)
    assert out.grad_fn is not None
    assert same_bits(out.detach(), fni_call(fni_leaves(gold, dev, grads=False)))
    dout = T(gold, "fni_dout", dev)
    out.backward(dout)
    assert_bits(ts["ref"].grad, gold["fni_dref"], "d ref_image")
    assert_bits(ts["src"].grad, gold["fni_dsrc"], "d psv_src_images")
    B, H, W, _ = dout.shape
    S, D = 2, 4
    N = H * W
    check_sum(ts["depths"].grad, gold["fni_ddepths_S64"].sum(0), gold["fni_ddepths_A"].sum(0), S * B * N, "fni ddepths")
    # per source, on the strided slices themselves (a channel slice of the sources, a slice of the wider dout)
    for i in range(S):
        src = ts["src"].detach()[..., 3 * i:3 * i + 3]
        dsl = dout[..., 3 + i * D * 3:3 + (i + 1) * D * 3]
        assert not src.is_contiguous() and not dsl.is_contiguous()
        ki, proj = T(gold, "fni_ki", dev)[i], T(gold, "fni_proj", dev)[i]
        got = backward(src, ts["depths"].detach(), ki, proj, dsl)
        dense = backward(src.contiguous(), ts["depths"].detach(), ki, proj, dsl.contiguous())
        for a, b in zip(got, dense):
            assert same_bits(a, b), "strided inputs change the bits"
        assert_bits(got[0], gold["fni_dsrc"][..., 3 * i:3 * i + 3], f"source {i} d img")
        for g, what in ((got[2], "dki"), (got[3], "dproj")):
            check_sum(g, gold[f"fni_{what}_S64"][i], gold[f"fni_{what}_A"][i], D * N, f"fni[{i}] {what}")
        check_sum(got[1], gold["fni_ddepths_S64"][i], gold["fni_ddepths_A"][i], B * N, f"fni[{i}] ddepths")

    def chain(K, ref_pose, src_poses):
        inv = torch.inverse(ref_pose)
        return torch.cat([chain64(K, K, torch.matmul(src_poses[:, i], inv)) for i in range(S)])

    cot = torch.cat([torch.cat([torch.tensor(gold[f"fni_{w}_S64"][i]).reshape(-1) for w in ("dki", "dproj")]) for i in range(S)])
    A = torch.cat([torch.cat([torch.tensor(gold[f"fni_{w}_A"][i]).reshape(-1) for w in ("dki", "dproj")]) for i in range(S)])
    leaves64 = tuple(torch.tensor(gold[f"fni_{k}"]).double() for k in ("K", "ref_pose", "src_poses"))
    check_chain(chain, leaves64, [ts["K"].grad, ts["ref_pose"].grad, ts["src_poses"].grad], cot, A, D * N, 16,
                "fni dK/dref_pose/dsrc_poses")


# ---------------------------------------------------------------------------
# 2. composition: D inverse-warp adjoints on constant depth maps
# ---------------------------------------------------------------------------

def per_depth(img, depths, ki, proj, dout):
    """_lib.inverse_warp_backward per depth on a constant depth map and dout's slice: lists over d."""
    B, Ht, Wt, _ = dout.shape
    C = img.shape[3]
    res = []
    for d in range(depths.numel()):
        dmap = torch.zeros((B, Ht, Wt), device=img.device) + depths[d]
        res.append(_lib.inverse_warp_backward(img, dmap, ki, proj, dout[..., d * C:(d + 1) * C]))
    return res


def fold_desc(parts):
    acc = parts[-1]
    for p in parts[-2::-1]:
        acc = acc + p
    return acc


@pytest.mark.parametrize("name", ["psv", "psv1", "one2"])
def test_composition_of_inverse_warp_adjoints(name, gold, dev):
    args = inputs(gold, name, dev)
    dimg, ddepths, dki, dproj = backward(*args)
    parts = per_depth(*args)
    D = len(parts)
    B, Ht, Wt, _ = args[4].shape
    N = Ht * Wt
    assert same_bits(dimg, fold_desc([p[0] for p in parts])), "d img is not the descending fold of the per-depth d img"
    if D > 1:
        asc = parts[0][0]
        for p in parts[1:]:
            asc = asc + p[0]
        assert not same_bits(dimg, asc), "the ascending fold has the same bits: the case cannot tell the orders apart"
    else:
        assert same_bits(dimg, parts[0][0])  # the per-pixel path itself
    for d, p in enumerate(parts):
        assert_bits(p[1], gold[f"{name}_ddepth_d"][d], f"{name} per-pixel d depth, plane {d}")
    for k, what in ((2, "dki"), (3, "dproj")):
        tot = sum(p[k].double() for p in parts).cpu().numpy()
        A = gold[f"{name}_{what}_A"]
        got = (dki if k == 2 else dproj).double().cpu().numpy()
        # both sides are sums of the same D*N terms: gamma_{D*N} A for the entry, gamma_N A_d per depth for the parts
        assert (np.abs(got - tot) <= (gamma(D * N) + gamma(N)) * A).all(), what
    maps = np.array([p[1].double().sum().item() for p in parts])  # (float64 sums of B*N terms: S64 to ~N 2^-53)
    A = gold[f"{name}_ddepths_A"]
    assert (np.abs(ddepths.double().cpu().numpy() - maps) <= (gamma(B * N) + B * N * 2.0 ** -53) * A).all()


# ---------------------------------------------------------------------------
# 3. ATen itself
# ---------------------------------------------------------------------------

def aten_dimg(img, depths, ki, proj, dout):
    """ATen's CPU grid_sample backward per depth at the coordinates the project's bit-exact pixel2cam /
    cam2pixel kernels produce, the D image gradients added in descending d: d img [B,Hs,Ws,C] on the CPU."""
    dev = img.device
    B, Hs, Ws, C = img.shape
    _, Ht, Wt, _ = dout.shape
    n = Ht * Wt
    ys, xs = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(n)], 0).expand(B, 3, n).contiguous().to(dev)
    parts = []
    for d in range(depths.numel()):
        dmap = (torch.zeros((B, Ht, Wt), device=dev) + depths[d]).contiguous()
        cam = torch.empty((B, 4, Ht, Wt), device=dev)
        _lib._call("mpiv_pixel2cam", dmap, pc, ki.contiguous(), B, n, 1, cam, _lib._stream(dev))
        pix = _lib.cam2pixel(cam, proj).cpu()
        coords = (pix + torch.tensor([0.5, 0.5])) / torch.tensor([float(Hs), float(Ws)])
        grid = torch.tensor([-1.0, -1.0]) + 2.0 * coords
        leaf = img.detach().cpu().contiguous().requires_grad_()
        out = F.grid_sample(leaf.permute(0, 3, 1, 2), grid, align_corners=False).permute(0, 2, 3, 1)
        out.backward(dout[..., d * C:(d + 1) * C].detach().cpu())
        parts.append(leaf.grad)
    return fold_desc(parts)


def rand_case(seed, B, Hs, Ws, C, Ht, Wt, depths, dev):
    """A general camera whose samples cover the source and its surroundings (tests/test_warpgrad_gpu.py's)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, Hs, Ws, C), generator=g)
    depths = torch.tensor(depths, dtype=torch.float32)
    dout = torch.rand((B, Ht, Wt, len(depths) * C), generator=g) * 2 - 1
    ki = torch.tensor([[1.2 * Hs / Wt, 0.01, -0.1 * Hs, 0.02, 1.2 * Ws / Ht, -0.1 * Ws, 0.0, 0.0, 1.0]])
    ki = ki.repeat(B, 1) * (1 + 0.1 * torch.arange(B).reshape(B, 1))
    proj = torch.tensor([[1.0, 0.03, 0.2, 0.5, -0.02, 1.0, 0.1, -0.4, 0.001, 0.002, 1.0, 0.05, 0.0, 0.0, 0.0, 1.0]])
    proj = proj.repeat(B, 1) * (1 + 0.05 * torch.arange(B).reshape(B, 1))
    return [t.to(dev) for t in (img, depths, ki, proj, dout)]


def check_dimg(args, what):
    dimg = backward(*args, want=(True, False, False, False))[0]
    want = aten_dimg(*args)
    got = dimg.cpu().numpy()
    fin = np.isfinite(want.numpy())
    assert (np.isfinite(got) == fin).all(), f"{what}: non-finite pattern"
    assert_bits(np.where(fin, got, 0), np.where(fin, want.numpy(), 0), f"{what} d img vs ATen")
    return float((want != 0).double().mean())


D5 = [5.0, 3.2, 2.1, 1.4, 1.0]


@pytest.mark.parametrize("C", [1, 3, 4, 5])
def test_dimg_is_atens_13x21(C, dev):
    """273 pixels: chunks of 8 wrap rows and the count is no multiple of 64; B = 2 with two cameras; D = 5."""
    assert check_dimg(rand_case(30 + C, 2, 9, 11, C, 13, 21, D5, dev), f"C={C}") > 0.3


def test_a_zero_depth_puts_every_pixel_into_one_bucket(dev):
    args = rand_case(3, 1, 9, 11, 3, 13, 21, [4.0, 0.0, 1.5], dev)
    args[3] = args[3].clone()
    args[3][:, 3], args[3][:, 7], args[3][:, 11] = 3.3, 4.6, 1.0  # proj's last column: depth 0's one sample position
    assert check_dimg(args, "depth 0") > 0


def test_negative_and_nonfinite_depths(dev):
    args = rand_case(4, 2, 9, 11, 3, 13, 21, [3.0, -1.5, float("inf"), 2.0, float("nan"), 1.2], dev)
    check_dimg(args, "negative / inf / nan depths")


@pytest.mark.parametrize("hw", [(1, 9), (9, 1)])
def test_one_row_and_one_column_sources(hw, dev):
    assert check_dimg(rand_case(sum(hw), 1, hw[0], hw[1], 3, 13, 21, D5, dev), f"source {hw}") > 0


# ---------------------------------------------------------------------------
# 4. grouping, independence, strides, routes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["psv33", "psv"])
def test_the_grouping_changes_no_bit(name, gold, dev):
    args = inputs(gold, name, dev)
    B, Hs, Ws, C = args[0].shape
    Ht, Wt = args[4].shape[1:3]
    D = args[1].numel()
    L = _lib.load()
    full = L.mpiv_plane_sweep_backward_workspace_size(B, Hs, Ws, C, Ht, Wt, D)
    least = L.mpiv_plane_sweep_backward_workspace_size_min(B, Hs, Ws, C, Ht, Wt, D)
    assert least < full
    base = backward(*args)
    assert_bits(base[0], gold[f"{name}_dimg"], "d img")
    per_plane = (full - least) // (D - 1)
    for what, n in (("one plane per group", least), ("groups of 4 and a remainder", least + 3 * per_plane + 4096),
                    ("all but one plane", full - 256), ("all planes", full + 64)):
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)  # every stale float a NaN
        got = backward(*args, workspace=ws)
        for a, b, k in zip(got, base, ("dimg", "ddepths", "dki", "dproj")):
            assert same_bits(a, b), f"{name}, {what}: {k}"
    with pytest.raises(RuntimeError, match="workspace"):
        backward(*args, workspace=torch.empty(least - 256, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("name", ["psv", "one2"])
def test_each_gradient_alone_has_the_same_bits(name, gold, dev):
    args = inputs(gold, name, dev)
    base = backward(*args)
    for i, k in enumerate(("dimg", "ddepths", "dki", "dproj")):
        got = backward(*args, want=tuple(j == i for j in range(4)))
        assert [g is not None for g in got] == [j == i for j in range(4)]
        assert same_bits(got[i], base[i]), f"{k} alone"
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = backward(*args)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(on_side, base):
        assert same_bits(a, b), "side stream"
    with pytest.raises(RuntimeError, match="nothing to compute"):
        backward(*args, want=(False,) * 4)


def record_calls(monkeypatch):
    names = []
    real = _lib._call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", call)
    return names


def test_each_input_alone_and_nothing_changes_without_a_gradient(gold, dev, monkeypatch):
    """One input requiring grad launches the backward once with only its gradient; with nothing requiring
    grad, or under no_grad, the entries called are today's."""
    dout = T(gold, "psv_dout", dev)
    seen = []
    real = _lib._call

    def spy(name, *a):
        if name == "mpiv_plane_sweep_backward":
            seen.append(tuple(p is not None for p in a[14:18]))  # dimg, ddepths, dki, dproj
        return real(name, *a)
    monkeypatch.setattr(_lib, "_call", spy)
    for i, (want, what) in enumerate((((True, False, False, False), "img"), ((False, True, False, False), "depths"),
                                      ((False, False, False, True), "pose"), ((False, False, True, True), "K"))):
        grads = tuple(j == i for j in range(4))
        out, ts = public(gold, "psv", dev, dev, grads=grads)
        out.backward(dout)
        assert seen[-1] == want and len(seen) == i + 1, (what, seen)
        for j, t in enumerate(ts):
            assert (t.grad is not None) == (j == i), (what, j)
    monkeypatch.undo()
    names = record_calls(monkeypatch)
    public(gold, "psv", dev, dev, grads=(False,) * 4)
    with torch.no_grad():
        public(gold, "psv", dev, dev)
    public(gold, "psv", dev, "cpu", grads=(False,) * 4)
    public(gold, "one2", dev, dev, grads=(False,) * 4)
    public(gold, "psv", dev, dev, grads=(False,) * 4, depths_as_list=True)
    assert names == ["mpiv_plane_sweep_pose", "mpiv_plane_sweep_pose", "mpiv_plane_sweep", "mpiv_plane_sweep_pose",
                     "mpiv_plane_sweep_pose"], names
    del names[:]
    fni_call(fni_leaves(gold, dev, grads=False))
    with torch.no_grad():
        fni_call(fni_leaves(gold, dev))
    assert names == ["mpiv_plane_sweep_into"] * 4, names
    del names[:]
    out, _ = public(gold, "psv", dev, dev, grads=(True, True, False, False))
    out.backward(dout)
    assert names == ["mpiv_psv_proj_device", "mpiv_plane_sweep", "mpiv_plane_sweep_backward"], names
    del names[:]
    out, ts = public(gold, "psv", dev, dev, grads=(True, False, False, False), depths_as_list=True)
    out.backward(dout)
    assert names == ["mpiv_psv_proj_device", "mpiv_plane_sweep", "mpiv_plane_sweep_backward"], names
    assert_bits(ts[0].grad, gold["psv_dimg"], "d img, depths as a list")


def test_a_cpu_image_keeps_todays_route():
    img = torch.zeros((1, 4, 4, 3), requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mv.plane_sweep_torch(img, [1.0, 2.0], torch.eye(4)[None], torch.eye(3)[None])


# ---------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------

def test_public_call_with_device_cameras_is_capturable(gold, dev):
    """plane_sweep_torch with img and a depths tensor requiring grad and pose / K in HBM (the no-grad device
    route of the matrices): forward + backward captured on a side stream and replayed with new images,
    depths, poses and gradients."""
    img, depths, dout, pose, K = (T(gold, f"psv_{k}", dev) for k in ("img", "depths", "dout", "pose", "K"))
    pose2 = pose.clone()
    pose2[:, :3, 3] += 0.05
    sets = [(img, depths, pose, dout), (img.flip(2).contiguous(), depths * 1.25, pose2, dout * -0.5)]

    def step(img, depths, pose, dout):
        li, ld = img.detach().requires_grad_(), depths.detach().requires_grad_()
        out = mv.plane_sweep_torch(li, ld, pose, K)
        return (out.detach(),) + torch.autograd.grad(out, (li, ld), dout)

    want = [step(*s) for s in sets]
    assert_bits(want[0][1], gold["psv_dimg"], "d img")
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
    assert not same_bits(want[0][1], want[1][1])
