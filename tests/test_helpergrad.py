"""CPU tests of the sampler's and the compositor's differentiable routes: the ABI surface of the two
adjoint entries (helper_bwd.hip), their argument checks (which run before anything is launched, so they
need no GPU), and the golden fixtures' own assertions (tests/golden/helpergrad.npz,
tools/gen_goldens_helpergrad.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, REPO

from mpi_vision_amd import _lib

sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_goldens_helpergrad as gen  # noqa: E402

NEW = ("mpiv_grid_sample_backward", "mpiv_grid_sample_backward_workspace_size", "mpiv_over_composite_backward",
       "mpiv_over_composite_backward_workspace_size")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "helpergrad.npz")))


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "mpiv.h")) as f:
        header = f.read()
    L = _lib.load_main()
    for n in NEW:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), f"{n} is not exported by the cross-compiled library"
    for n in ("mpiv_grid_sample_backward", "mpiv_over_composite_backward"):
        assert n in _lib._SIGS_HELPER_BWD and n not in _lib._SIGS
        assert getattr(L, n).argtypes == _lib._SIGS_HELPER_BWD[n]
    assert len(_lib._SIGS_HELPER_BWD["mpiv_grid_sample_backward"]) == 17
    assert len(_lib._SIGS_HELPER_BWD["mpiv_over_composite_backward"]) == 11
    assert L.mpiv_abi_version() == 17 == _lib.ABI_VERSION
    with open(os.path.join(REPO, "mpi_vision_amd", "csrc", "SOURCES")) as f:
        assert "helper_bwd.hip" in f.read().split()


def test_workspace_sizes():
    L = _lib.load_main()
    n = L.mpiv_grid_sample_backward_workspace_size(2, 3, 30, 44, 13, 21)
    assert n >= 2 * 13 * 21 * 24  # positions, two key and two id arrays
    assert n == L.mpiv_inverse_warp_backward_workspace_size(2, 30, 44, 3, 13, 21)  # the same stages
    assert L.mpiv_grid_sample_backward_workspace_size(2, 3, 30, 44, 0, 21) == 0
    # sizes the 31-bit ids cannot index
    assert L.mpiv_grid_sample_backward_workspace_size(1, 3, 4, 4, 1 << 16, 1 << 15) == 0
    assert L.mpiv_grid_sample_backward_workspace_size(1, 1, (1 << 16) - 1, 1 << 15, 4, 4) == 0
    # the compositor: 12 B per pixel and chunk of 8 layers but the first; none for P <= 9
    size = L.mpiv_over_composite_backward_workspace_size
    assert [size(P, 1000) for P in (1, 2, 9, 10, 17, 18, 33)] == [0, 0, 0, 12000, 12000, 24000, 36000]
    assert size(33, 1 << 31) == 0 and size(0, 10) == 0 and size(3, 0) == 0 and size(1 << 24, 10) == 0
    assert size(33, (1 << 31) - 1) == 3 * 12 * ((1 << 31) - 1)


def test_entries_refuse_what_they_cannot_index_without_a_device():
    """Argument checks run before anything is launched, so they need no GPU."""
    L = _lib.load_main()
    st4, st2 = (ctypes.c_int64 * 4)(1, 1, 1, 1), (ctypes.c_int64 * 2)(3, 1)
    gs = L.mpiv_grid_sample_backward
    assert gs(8, st4, 1, 3, 4, 4, 8, st4, 1 << 16, 1 << 15, 8, st4, None, 8, 16, 1 << 20, None) != 0
    assert b"limited to" in L.mpiv_last_error()
    assert gs(8, st4, 1, 1, (1 << 16) - 1, 1 << 15, 8, st4, 4, 4, 8, st4, None, 8, 16, 1 << 20, None) != 0
    assert b"limited to" in L.mpiv_last_error()
    assert gs(8, st4, 1, 3, 4, 4, 8, st4, 4, 4, 8, st4, None, None, 16, 1 << 20, None) != 0
    assert b"no gradient" in L.mpiv_last_error()
    assert gs(8, st4, 1, 3, 4, 4, 8, st4, 4, 4, 8, st4, 8, None, 16, 64, None) != 0
    assert b"workspace" in L.mpiv_last_error()
    assert gs(8, st4, 1, 3, 4, 4, 8, st4, 4, 4, 8, st4, 8, 8, None, 0, None) != 0
    assert b"workspace" in L.mpiv_last_error()
    assert gs(None, st4, 1, 3, 4, 4, 8, st4, 4, 4, 8, st4, 8, 8, 16, 1 << 20, None) != 0
    assert b"null pointer" in L.mpiv_last_error()
    assert gs(8, st4, 1, 3, 4, 0, 8, st4, 4, 4, 8, st4, 8, 8, 16, 1 << 20, None) != 0
    assert b"bad shape" in L.mpiv_last_error()
    oc = L.mpiv_over_composite_backward
    assert oc(8, 33, 1 << 31, 4, 1, 8, st2, 16, 16, 1 << 20, None) != 0
    assert b"limited to" in L.mpiv_last_error()
    assert oc(8, 33, 1000, 4, 1, 8, st2, 16, 16, 36000 - 1, None) != 0
    assert b"workspace" in L.mpiv_last_error()
    assert oc(8, 10, 1000, 4, 1, 8, st2, 16, None, 0, None) != 0
    assert b"workspace" in L.mpiv_last_error()
    assert oc(8, 9, 1000, 4, 1, 8, st2, None, None, 0, None) != 0
    assert b"null pointer" in L.mpiv_last_error()
    assert oc(8, 0, 1000, 4, 1, 8, st2, 16, None, 0, None) != 0
    assert b"bad shape" in L.mpiv_last_error()


def test_cpu_tensors_keep_todays_error():
    """The differentiable routes need device tensors: a CPU tensor raises today's error, grad or not."""
    for grad in (False, True):
        imgs = torch.zeros((1, 4, 4, 3), requires_grad=grad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            _lib.bilinear_sample(imgs, torch.zeros((1, 2, 2, 2)), True)
        with pytest.raises(RuntimeError, match="no CPU path"):
            _lib.over_composite([torch.zeros((1, 2, 2, 4), requires_grad=grad)] * 2)
    with pytest.raises(UnboundLocalError):
        _lib.over_composite([])


@pytest.mark.parametrize("name", ["bw", "rs"])
def test_sampler_goldens_own_assertions(name, gold):
    imgs, coords, dout = gen.helper_inputs(name)
    assert gen.sha(imgs, coords, dout) == str(gold[f"{name}_sha"]), "the regenerated inputs are not the golden's"
    assert float(coords.min()) < -0.2 and float(coords.max()) > 1.2
    assert gold[f"{name}_out"].shape == tuple(dout.shape)
    for k, t in (("dimgs", imgs), ("dcoords", coords)):
        g = gold[f"{name}_{k}"]
        assert g.shape == tuple(t.shape) and np.isfinite(g).all() and (g != 0).mean() > 0.3, k


@pytest.mark.parametrize("P", gen.OVER_P)
def test_compositor_goldens_own_assertions(P, gold):
    layers, dout = gen.over_inputs(P)
    assert gen.sha(torch.stack(layers), dout) == str(gold[f"oc{P}_sha"]), "the regenerated inputs are not the golden's"
    alpha = torch.stack(layers)[..., 3]
    assert bool((alpha == 0).any()) and bool((alpha == 1).any())
    assert bool((dout[0, 0] == 0).all()) and not bool(torch.signbit(dout[0, 0]).any())
    assert bool(torch.signbit(dout[0, 1]).all()) and bool((dout[0, 1] == 0).all())
    assert gold[f"oc{P}_out"].shape == (2, 13, 21, 3) and len(str(gold[f"oc{P}_dsha"])) == 64
    if P <= 2:
        block = gold[f"oc{P}_dlayers"]
        assert block.shape == (P, 2, 13, 21, 4) and gen.sha(torch.tensor(block)) == str(gold[f"oc{P}_dsha"])
        first, last = block[0], block[-1]
    else:
        first, last = gold[f"oc{P}_d0"], gold[f"oc{P}_dlast"]
    assert (last != 0).mean() > 0.3 and not first[..., 3].any() and not np.signbit(first[..., 3]).any()
    if P > 1:  # a -0 cotangent survives in layer 0's colour and nowhere else
        assert np.signbit(first[0, 1, :, :3]).any() and not np.signbit(last[0, 1]).any()
