"""CPU: the ABI surface of training through a half MPI (mpiv_render_train_f16,
mpiv_render_backward[_watched|_cam]_f16), their argument validation, and the golden fixture
tests/golden/f16grad.npz (tools/gen_goldens_f16grad.py) pinned to the CPU oracle: the half gradient is
the oracle's fp32 gradient on the widened MPI, rounded to half once."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD, assert_bits
from test_abi import declared_symbols

from mpi_vision_amd import _lib  # noqa: E402
from oracle import oracle  # noqa: E402

ENTRIES = ("mpiv_render_train_f16", "mpiv_render_backward_f16", "mpiv_render_backward_watched_f16",
           "mpiv_render_backward_cam_f16")
CASES = ("ga", "gsub", "ginf", "gp17")
SHARED = {"gsub": "ga", "ginf": "ga"}  # these differ from ga in dout alone: the rest is stored once


def case_arrays(npz, name):
    """{key: array} of one f16grad.npz case; gsub and ginf take what they do not store from ga."""
    keys = ("mpi", "pose", "K", "depths", "H", "out", "dout", "grad")
    base = SHARED.get(name, name)
    return {k: npz[f"{name}_{k}"] if f"{name}_{k}" in npz.files else npz[f"{base}_{k}"] for k in keys}


@pytest.fixture(scope="module")
def f16grad():
    return np.load(os.path.join(GOLD, "f16grad.npz"))


def test_entries_declared_exported_and_bound():
    """Additive: the header declares the four entries, the library exports them, _lib binds them in a
    dict of their own with the float entries' argument lists, and the ABI version stays 17."""
    L = _lib.load()
    for name in ENTRIES:
        assert name in declared_symbols() and hasattr(L, name) and name in _lib.EXPORTS, name
        assert name in _lib._SIGS_F16_TRAIN and name not in _lib._SIGS, name
        assert getattr(L, name).argtypes == _lib._SIGS_F16_TRAIN[name]
    assert _lib._SIGS_F16_TRAIN["mpiv_render_train_f16"] == _lib._SIGS["mpiv_render_train"]
    assert _lib._SIGS_F16_TRAIN["mpiv_render_backward_cam_f16"] == _lib._SIGS_CAM["mpiv_render_backward_cam"]


def test_abi_version_is_still_17():
    assert _lib.ABI_VERSION == 17 and _lib.load().mpiv_abi_version() == 17


def _err(L):
    return L.mpiv_last_error().decode()


def test_arguments_rejected_before_any_launch():
    """The layout rule is 8-byte aligned texels with strides[3] == 4 and strides[4] == 1, strides in half
    elements; like their siblings the entries validate and report through mpiv_last_error."""
    L = _lib.load()
    H, W, P = 4, 4, 2
    st = (ctypes.c_int64 * 5)(H * W * P * 4, W * P * 4, P * 4, 4, 1)
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(256 + 4)
    nbytes = L.mpiv_render_backward_workspace_size(H, W, P)
    train, bwd = L.mpiv_render_train_f16, L.mpiv_render_backward_f16
    assert train(None, st, 1, H, W, P, p, p, p, None) == -1 and "mpiv_render_train_f16: null pointer" in _err(L)
    assert train(p, st, 1, 1, W, P, p, p, p, None) == -1 and "bad shape" in _err(L)
    assert train(odd, st, 1, H, W, P, p, p, p, None) == -1 and "8-byte texels" in _err(L)
    bad = (ctypes.c_int64 * 5)(H * W * P * 4, W * P * 4, P * 4, 1, P)  # planes not contiguous per pixel
    assert train(p, bad, 1, H, W, P, p, p, p, None) == -1 and "read in place" in _err(L)
    assert bwd(None, st, 1, H, W, P, p, p, None, p, p, nbytes, None) == -1 and "null pointer" in _err(L)
    assert bwd(odd, st, 1, H, W, P, p, p, None, p, p, nbytes, None) == -1 and "8-byte aligned texels" in _err(L)
    assert bwd(p, st, 1, H, W, P, p, p, None, odd, p, nbytes, None) == -1 and "must be 8-byte" in _err(L)
    assert bwd(p, st, 1, H, W, P, p, p, None, p, p, 16, None) == -1 and "workspace too small" in _err(L)
    assert (L.mpiv_render_backward_cam_f16(p, st, 1, H, W, P, p, p, None, p, None, p, nbytes, 0, None) == -1
            and "mpiv_render_backward_cam_f16: null pointer" in _err(L))
    # the float entries keep their own rule (16-byte texels) and messages
    assert L.mpiv_render_backward(ctypes.c_void_p(256 + 8), st, 1, H, W, P, p, p, None, p, p, nbytes, None) == -1
    assert "16-byte aligned texels" in _err(L)


def test_layout_predicate_for_half():
    """bwd_layout_ok on a half tensor: 8-byte aligned texels, otherwise the float limits."""
    import torch
    buf = torch.zeros(2 + 3 * 5 * 7 * 4 + 8, dtype=torch.float16)
    x = buf[:3 * 5 * 7 * 4].view(1, 3, 5, 7, 4)
    assert _lib.bwd_layout_ok(x) and _lib.bwd_layout_ok(x[:, 1:, 1:-1]) and _lib._f16_in_place(x) is x
    y = buf[2:2 + 3 * 5 * 7 * 4].view(1, 3, 5, 7, 4)  # a data pointer that is only 4-byte aligned
    assert y.data_ptr() % 8 == 4 and y.is_contiguous() and not _lib.bwd_layout_ok(y)
    c = _lib._f16_in_place(y)
    assert c.dtype == torch.float16 and c.data_ptr() % 8 == 0 and torch.equal(c, y)
    z = x.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)  # planes not contiguous per pixel
    assert not _lib.bwd_layout_ok(z) and _lib._f16_in_place(z).dtype == torch.float16
    f = torch.zeros((1, 3, 5, 7, 4))
    # a float tensor keeps the 16-byte rule: an 8-byte aligned data pointer is not read in place
    assert _lib.bwd_layout_ok(f) and not _lib.bwd_layout_ok(f.view(-1)[2:2 + 2 * 5 * 7 * 4].view(1, 2, 5, 7, 4))


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_the_oracles_gradient_rounded_once(name, f16grad):
    """Every f16grad.npz case: the frame is the oracle's render of the widened MPI and the half gradient
    is oracle.render_backward(mpi.astype(float32), H, dout).astype(float16), bit for bit."""
    c = case_arrays(f16grad, name)
    assert c["mpi"].dtype == np.float16 and c["grad"].dtype == np.float16
    B, P = c["dout"].shape[0], c["mpi"].shape[3]
    homs = c["H"].transpose(1, 0, 2, 3).reshape(B, P, 9)
    wide = c["mpi"].astype(np.float32)
    assert_bits(oracle.render(wide, homs), c["out"], f"{name} forward")
    with np.errstate(over="ignore"):
        want = oracle.render_backward(wide, homs, c["dout"]).astype(np.float16)
    assert want.shape == c["grad"].shape
    assert np.array_equal(want.view(np.uint16), c["grad"].view(np.uint16)), f"{name}: half gradient bits"


def test_fixture_covers_subnormals_overflow_and_three_chunks(f16grad):
    sub = np.abs(f16grad["gsub_grad"].astype(np.float32))
    assert ((sub > 0) & (sub < 2.0 ** -14)).sum() > sub.size // 2  # half subnormals dominate
    assert np.isinf(f16grad["ginf_grad"]).sum() >= 1 and not np.isnan(f16grad["ginf_grad"]).any()
    assert f16grad["gp17_mpi"].shape == (1, 24, 32, 17, 4)
    assert os.path.getsize(os.path.join(GOLD, "f16grad.npz")) < (1 << 20)
