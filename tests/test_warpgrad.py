"""CPU tests of the inverse warp's differentiable route: the ABI surface of its entry, the host chain
from (Ki, proj) to pose and intrinsics (_host.psv_matrices_autograd), and the golden fixtures' own
assertions (tests/golden/warpgrad.npz, tools/gen_goldens_warpgrad.py)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, REPO, assert_bits

import mpi_vision_amd as mv
from mpi_vision_amd import _host, _lib

FULL = ["piw", "piw4", "piw2"]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "warp.npz")))
    g.update(np.load(os.path.join(GOLD, "warpgrad.npz")))
    return g


def cameras(gold, name):
    """(Ks, Kt, pose) of a golden case as fresh leaves."""
    two = name == "piw2"
    Ks = torch.tensor(gold[f"{name}_Ks" if two else f"{name}_K"])
    Kt = torch.tensor(gold[f"{name}_Kt"]) if two else Ks
    return Ks, Kt, torch.tensor(gold[f"{name}_pose"])


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "mpiv.h")) as f:
        header = f.read()
    names = ("mpiv_inverse_warp_backward", "mpiv_inverse_warp_backward_workspace_size")
    for n in names:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.EXPORTS
    assert "mpiv_inverse_warp_backward" in _lib._SIGS_WARP and "mpiv_inverse_warp_backward" not in _lib._SIGS
    assert len(_lib._SIGS_WARP["mpiv_inverse_warp_backward"]) == 21
    L = _lib.load_main()
    assert L.mpiv_abi_version() == 17 == _lib.ABI_VERSION
    assert L.mpiv_inverse_warp_backward.argtypes == _lib._SIGS_WARP["mpiv_inverse_warp_backward"]
    n = L.mpiv_inverse_warp_backward_workspace_size(2, 30, 44, 3, 30, 44)
    assert n >= 2 * 30 * 44 * 24 and L.mpiv_inverse_warp_backward_workspace_size(2, 30, 44, 3, 0, 44) == 0
    with open(os.path.join(REPO, "mpi_vision_amd", "csrc", "SOURCES")) as f:
        assert "warp_bwd.hip" in f.read().split()


def test_entry_refuses_what_it_cannot_index_without_a_device():
    """Argument checks run before anything is launched, so they need no GPU."""
    L = _lib.load_main()
    st4, st3 = (_lib.ctypes.c_int64 * 4)(1, 1, 1, 1), (_lib.ctypes.c_int64 * 3)(1, 1, 1)
    assert L.mpiv_inverse_warp_backward_workspace_size(1, 4, 4, 3, 1 << 16, 1 << 15) == 0
    assert L.mpiv_inverse_warp_backward_workspace_size(1, (1 << 16) - 1, 1 << 15, 1, 4, 4) == 0
    rc = L.mpiv_inverse_warp_backward(8, st4, 1, 4, 4, 3, 8, 8, 8, st3, 1 << 16, 1 << 15, 8, st4, 8, None, None, None,
                                      16, 1 << 20, None)
    assert rc != 0 and b"limited to" in L.mpiv_last_error()
    rc = L.mpiv_inverse_warp_backward(8, st4, 1, 4, 4, 3, 8, 8, 8, st3, 4, 4, 8, st4, None, None, None, None, 16,
                                      1 << 20, None)
    assert rc != 0 and b"no gradient" in L.mpiv_last_error()
    rc = L.mpiv_inverse_warp_backward(8, st4, 1, 4, 4, 3, 8, 8, 8, st3, 4, 4, 8, st4, 8, None, None, None, 16, 64, None)
    assert rc != 0 and b"workspace" in L.mpiv_last_error()


def layouts(K):
    """The same cameras as a stride-0 batch, a sliced block and (one camera) unbatched."""
    B = K.shape[0]
    out = {"dense": K.clone()}
    wide = torch.zeros((B, 3, 5))
    wide[:, :, 1:4] = K
    out["sliced"] = wide[:, :, 1:4]
    out["F-ordered"] = K.transpose(1, 2).contiguous().transpose(1, 2)
    if B == 1 or bool((K == K[:1]).all()):
        out["stride-0"] = K[0][None].expand(B, 3, 3)
        out["unbatched"] = K[0].clone()
    return out


@pytest.mark.parametrize("name", FULL + ["w1"])
def test_autograd_chain_values_are_psv_matrices_bits(name, gold):
    Ks, Kt, pose = cameras(gold, name)
    for what, kt in layouts(Kt).items():
        srcs = {"dense": Ks}
        if "stride-0" in layouts(Ks):
            srcs["stride-0"] = layouts(Ks)["stride-0"]
        for what_s, ks in srcs.items():
            want_ki, want_proj = _host.psv_matrices(ks, kt, pose)
            ki, proj = _host.psv_matrices_autograd(ks, kt, pose.clone().requires_grad_())
            assert ki.shape == want_ki.shape and proj.shape == want_proj.shape and proj.requires_grad
            assert_bits(ki, want_ki.numpy(), f"{name} ki, K_tgt {what}, K_src {what_s}")
            assert_bits(proj, want_proj.numpy(), f"{name} proj, K_tgt {what}, K_src {what_s}")
    ki, proj = _host.psv_matrices_autograd(Ks, Kt, pose)  # (exact-inverse cameras: the generating host's bits)
    assert_bits(ki, gold[f"{name}_ki"], "ki vs the reference's inverse")
    assert_bits(proj, gold[f"{name}_proj"], "proj vs the reference's K4 @ pose")


def test_gradient_reaches_a_strided_leaf_through_its_layout():
    """A stride-0 and a sliced K_tgt: the gradient of the base tensor is the dense one's (summed over the
    broadcast views)."""
    g = torch.Generator().manual_seed(3)
    K = torch.tensor([[32.0, 0, 12], [0, 64.0, 8.5], [0, 0, 1]])
    pose = torch.eye(4)[None].repeat(3, 1, 1)
    dki = torch.rand((3, 9), generator=g)
    dense = K[None].repeat(3, 1, 1).requires_grad_()
    _host.psv_matrices_autograd(dense.detach(), dense, pose)[0].backward(dki)
    leaf = K.clone().requires_grad_()
    _host.psv_matrices_autograd(K[None].repeat(3, 1, 1), leaf[None].expand(3, 3, 3), pose)[0].backward(dki)
    assert float((leaf.grad - dense.grad.sum(0)).abs().max()) <= 1e-6 * float(dense.grad.abs().max())
    one = K.clone().requires_grad_()
    _host.psv_matrices_autograd(K[None].repeat(3, 1, 1), one, pose)[0].backward(dki)
    assert float((one.grad - dense.grad.sum(0)).abs().max()) <= 1e-6 * float(dense.grad.abs().max())


@pytest.mark.parametrize("name", FULL + ["w1"])
def test_chain_gradients_from_the_golden_dki_dproj_are_the_references(name, gold):
    Ks, Kt, pose = cameras(gold, name)
    two = name == "piw2"
    Ks.requires_grad_()
    if two:
        Kt.requires_grad_()
    pose.requires_grad_()
    ki, proj = _host.psv_matrices_autograd(Ks, Kt, pose)
    torch.autograd.backward((ki, proj), (torch.tensor(gold[f"{name}_dki"]), torch.tensor(gold[f"{name}_dproj"])))
    assert_bits(pose.grad, gold[f"{name}_dpose"], f"{name} d pose")
    if two:
        assert_bits(Ks.grad, gold["piw2_dKs"], "d K_src")
        assert_bits(Kt.grad, gold["piw2_dKt"], "d K_tgt")
    else:
        assert_bits(Ks.grad, gold[f"{name}_dK"], f"{name} d K")


def test_ret_flows_still_raises():
    img = torch.zeros((1, 4, 4, 3), requires_grad=True)
    with pytest.raises(RuntimeError, match="ret_flows"):
        mv.projective_inverse_warp_torch(img, torch.ones((1, 4, 4)), torch.eye(4)[None], torch.eye(3)[None],
                                         ret_flows=True)
    with pytest.raises(RuntimeError, match="ret_flows"):
        mv.projective_inverse_warp_torch2(img, torch.ones((1, 4, 4)), torch.eye(4)[None], torch.eye(3)[None],
                                          torch.eye(3)[None], 4, 4, ret_flows=True)


def test_cpu_tensors_keep_todays_route():
    """The differentiable route needs a device image: a CPU image raises today's error, grad or not."""
    img = torch.zeros((1, 4, 4, 3), requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mv.projective_inverse_warp_torch(img, torch.ones((1, 4, 4)), torch.eye(4)[None], torch.eye(3)[None])


@pytest.mark.parametrize("name", FULL + ["w1"])
def test_goldens_own_assertions(name, gold):
    two = name == "piw2"
    dimg, ddepth, dout = (gold[f"{name}_{k}"] for k in ("dimg", "ddepth", "dout"))
    B, Ht, Wt = ddepth.shape
    N = Ht * Wt
    assert dout.shape[:3] == ddepth.shape and dimg.shape[0] == B and dimg.shape[3] == dout.shape[3]
    assert gold[f"{name}_dpix"].shape == (B, Ht, Wt, 2) and gold[f"{name}_dcam"].shape == (B, 4, Ht, Wt)
    assert gold[f"{name}_duvw"].shape == (B, 4, N) and not gold[f"{name}_duvw"][:, 3].any()
    g = N * U / (1 - N * U)
    for what, n in (("dki", 9), ("dproj", 16)):
        got, S64, A = (gold[f"{name}_{what}{s}"] for s in ("", "_S64", "_A"))
        assert got.shape == S64.shape == A.shape == (B, n) and S64.dtype == np.float64
        assert (np.abs(got - S64) <= g * A).all(), f"{name}: the reference's {what} is outside gamma_N * A"
    assert not gold[f"{name}_dproj"][:, 12:].any()
    for k in (("dKs", "dKt") if two else ("dK",)) + ("dpose",):
        assert np.isfinite(gold[f"{name}_{k}"]).all() and np.abs(gold[f"{name}_{k}"]).max() > 0
    if name == "w1":
        assert [int((dout[i] != 0).any(-1).sum()) for i in range(B)] == [1] * B
        for i, (x, y) in enumerate(gold["w1_pixels"]):
            assert dout[i, y, x].any()
        for what in ("dki", "dproj"):
            assert (gold[f"w1_{what}"] == gold[f"w1_{what}_S64"].astype(np.float32)).all()
        assert gold["w1_dproj"][0].any() and gold["w1_dproj"][2].any() and not gold["w1_dproj"][3].any()
    else:
        assert np.isfinite(ddepth).all() and np.isfinite(dimg).all()
        assert (ddepth != 0).mean() >= 0.5 and (np.abs(dimg).sum(-1) != 0).mean() >= 0.5
    # exact-inverse cameras: power-of-two focal lengths, dyadic principal points
    for k in (("Ks", "Kt") if two else ("K",)):
        K = gold[f"{name}_{k}"]
        assert (np.log2(K[:, 0, 0]) % 1 == 0).all() and (np.log2(K[:, 1, 1]) % 1 == 0).all()
        assert (K[:, :2, 2] * 2 % 1 == 0).all()
