"""CPU: the ABI surface of the alpha-only plane-colour render (mpiv_pack_planes_alpha,
mpiv_render_packed_alpha, the "render_packed_alpha" dry run), its argument validation, the route table
the GPU tests use, the golden fixture, and the drop-in wrappers' argument errors."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import planecolor_cases as pc
from conftest import assert_bits, load_test_mpi
from test_abi import declared_symbols

from mpi_vision_amd import _lib  # noqa: E402
from mpi_vision_amd import utils as mvu  # noqa: E402
from oracle import oracle  # noqa: E402

ENTRIES = ("mpiv_pack_planes_alpha", "mpiv_render_packed_alpha")


def test_entries_declared_exported_and_bound():
    """Additive: the header declares the two entries, the library exports them, _lib binds them in a
    dict of their own (tests/stream_cases.py holds one replay case per _SIGS entry), the ABI version
    stays 17."""
    import stream_cases
    L = _lib.load()
    for name in ENTRIES:
        assert name in declared_symbols() and hasattr(L, name) and name in _lib.EXPORTS, name
        assert name in _lib._SIGS_ALPHA and name not in _lib._SIGS, name
        assert getattr(L, name).argtypes == _lib._SIGS_ALPHA[name]
    assert _lib.ABI_VERSION == 17 and L.mpiv_abi_version() == 17
    assert set(_lib._SIGS) == stream_cases.COVERED | set(stream_cases.EXCLUDED)
    assert {e for c in stream_cases.CASES for e in c.entries} >= stream_cases.COVERED


def _err(L):
    return L.mpiv_last_error().decode()


def test_pack_arguments_rejected():
    L = _lib.load()
    st = (ctypes.c_int64 * 4)(64, 16, 4, 1)
    p = ctypes.c_void_p(256)
    pack = L.mpiv_pack_planes_alpha
    for args in ((None, st, 4, 4, 2, 3, p, None), (p, None, 4, 4, 2, 3, p, None), (p, st, 4, 4, 2, 3, None, None)):
        assert pack(*args) == -1 and "mpiv_pack_planes_alpha: null pointer" in _err(L)
    for shape in ((0, 4, 2), (4, 0, 2), (4, 4, 0), (4, 4, -1)):  # P < 1 included
        assert pack(p, st, *shape, 3, p, None) == -1 and "bad shape" in _err(L), shape
    for ch in (-1, 4):
        assert pack(p, st, 4, 4, 2, ch, p, None) == -1 and f"channel {ch} is not in 0..3" in _err(L)
    assert pack(p, st, 4, 4, 2, 3, ctypes.c_void_p(258), None) == -1 and "packed must be 4-byte aligned" in _err(L)
    # (23171 + 4)^2 * 4 bytes pass the 32-bit buffer offsets' limit; 23166 + 4 do not
    assert pack(p, st, 23171, 23171, 2, 3, p, None) == -1 and "padded plane larger than 2 GiB" in _err(L)


def test_render_arguments_rejected():
    L = _lib.load()
    p = ctypes.c_void_p(256)
    render = L.mpiv_render_packed_alpha
    for k in (0, 4, 5, 7):  # packed, colors, homs, out
        args = [p, 4, 4, 2, p, p, 1, p, None]
        args[k] = None
        assert render(*args) == -1 and "mpiv_render_packed_alpha: null pointer" in _err(L), k
    for H, W, P, V in ((1, 4, 2, 1), (4, 1, 2, 1), (4, 4, 0, 1), (4, 4, -3, 1), (4, 4, 2, 0)):
        assert render(p, H, W, P, p, p, V, p, None) == -1 and "bad shape (H, W >= 2)" in _err(L), (H, W, P, V)
    assert render(ctypes.c_void_p(257), 4, 4, 2, p, p, 1, p, None) == -1
    assert "packed must be 4-byte aligned" in _err(L)
    assert render(p, 23171, 23171, 2, p, p, 1, p, None) == -1 and "padded plane larger than 2 GiB" in _err(L)
    assert render(p, 2, 1 << 22, 2, p, p, 1, p, None) == -1 and "a side >= 2^22" in _err(L)
    with pytest.raises(RuntimeError, match="padded plane larger than 2 GiB"):
        _lib.route("render_packed_alpha", 23171, 23171, 2, 1)
    with pytest.raises(RuntimeError, match="wrong argument count"):
        _lib.route("render_packed_alpha", 64, 64, 2)


def test_route_table():
    """The dry run names the kernel and its grid; the GPU tests' shapes (planecolor_cases.ROUTES) reach
    every instantiation the dispatcher can launch; the thresholds sit where the table says."""
    seen = set()
    for (H, W, P), V, route in pc.ROUTES:
        name, grid = _lib.route("render_packed_alpha", H, W, P, V)
        assert name == pc.kernel_name(route), ((H, W, P), V, name)
        R = int(route.split(",")[0])
        assert grid == -(-W // 64) * -(-H // (4 * R)) * V * 256
        seen.add(route)
    assert seen == pc.INSTANTIATIONS
    # one view fewer than 2048 blocks: 4 rows in flight; the stretched launch falls back to 2 plain rows
    assert _lib.route("render_packed_alpha", 20, 18, 3, 1023)[0] == pc.kernel_name("4, true, 4")
    assert _lib.route("render_packed_alpha", 36, 64, 2, 1023)[0] == pc.kernel_name("2, false, 2")
    # config 4 at one view and on a camera path
    assert _lib.route("render_packed_alpha", 1024, 1024, 128, 1) == (pc.kernel_name("4, true, 4"), 16 * 64 * 256)
    assert _lib.route("render_packed_alpha", 1024, 1024, 128, 125)[0] == pc.kernel_name("4, true, 2")


@pytest.mark.parametrize("name", ["pa", "pb"])
def test_goldens_pinned(name):
    """Guards the fixture: the oracle on the constructed float MPI at the reference's homographies gives
    the reference's frame bit for bit."""
    g = pc.golden()
    alpha, colors = g[f"{name}_alpha"], g[f"{name}_colors"]
    assert_bits(oracle.render(pc.constructed(alpha, colors), pc.golden_homs(name)), g[f"{name}_out"], name)
    if name == "pa":
        assert_bits(colors, pc.depth_colors(g["pa_depths"]), "pa colours are (1/d, d, 1)")
    else:
        assert np.signbit(colors[3, 1]) and colors[3, 1] == 0.0, "pb has a -0.0 colour"


def test_golden_test_mpi_pinned(large):
    g = pc.golden()
    alpha = np.broadcast_to(load_test_mpi().numpy()[..., 3], (2, 400, 640, 10))
    homs = np.ascontiguousarray(large["c1_H"].transpose(1, 0, 2, 3)).reshape(2, 10, 9)
    frame = oracle.render(pc.constructed(alpha, pc.depth_colors(large["c1_depths"])), homs)
    assert hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest() == str(g["tm_sha"])
    assert_bits(frame[:, 184:216, 304:336], g["tm_crop"], "centre crop")


@pytest.mark.parametrize("fn", ["colors", "depth"])
def test_wrappers_raise(fn):
    """No CPU path; fp32 only; `planes` must be a tensor (the reference's AttributeError)."""
    mpi = torch.rand((1, 8, 8, 3, 4))
    pose, K, planes = torch.eye(4)[None], torch.eye(3)[None], torch.tensor([4.0, 2.0, 1.0])

    def call(m, pl):
        if fn == "depth":
            return mvu.mpi_render_depth_torch(m, pose, pl, K)
        return mvu.mpi_render_plane_colors_torch(m, torch.ones((3, 3)), pose, pl, K)

    with pytest.raises(RuntimeError, match="no CPU path"):
        call(mpi, planes)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(mpi[..., 3:], planes)
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        call(mpi.half(), planes)
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        call(mpi.double(), planes)
    with pytest.raises(AttributeError):
        call(mpi, [4.0, 2.0, 1.0])
    with pytest.raises(RuntimeError, match=r"\[B, H, W, P, 4\] or \[B, H, W, P, 1\]"):
        call(mpi[..., :3], planes)
