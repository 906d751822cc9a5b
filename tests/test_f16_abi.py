"""CPU: the half-precision MPI entry points (render_f16.hip) reject bad arguments with -1 and a
message before any HIP call, mpiv_route reports the f16 kernel the dispatcher would launch, and
the Python layer refuses CPU tensors and other dtypes."""
import ctypes

import pytest
import torch

from mpi_vision_amd import _lib

P16 = ctypes.c_void_p(16)
ST4 = (ctypes.c_int64 * 4)(1, 1, 1, 1)


def _pack(mpi=P16, st=ST4, H=4, W=4, P=2, packed=P16):
    return ("mpiv_pack_planes_f16", [mpi, st, H, W, P, packed, None])


def _unpack(packed=P16, H=4, W=4, P=2, out=P16):
    return ("mpiv_unpack_planes_f16", [packed, H, W, P, out, None])


def _render(packed=P16, H=4, W=4, P=2, homs=P16, V=1, out=P16):
    return ("mpiv_render_packed_f16", [packed, H, W, P, homs, V, out, None])


def _ct(packed=P16, H=4, W=4, P=8, a=0, b=8, back=1, homs=P16, V=1, ct=P16):
    return ("mpiv_render_packed_f16_ct", [packed, H, W, P, a, b, back, homs, V, ct, None])


def _rejected(call, message):
    name, args = call
    L = _lib.load()
    assert getattr(L, name)(*args) == -1, name
    err = L.mpiv_last_error().decode()
    assert message in err and name in err, err


@pytest.mark.parametrize("call", [
    _pack(mpi=None), _pack(st=None), _pack(packed=None), _unpack(packed=None), _unpack(out=None),
    _render(packed=None), _render(homs=None), _render(out=None), _ct(packed=None), _ct(homs=None), _ct(ct=None)],
    ids=lambda c: c[0])
def test_null_pointers_rejected(call):
    _rejected(call, "null pointer")


@pytest.mark.parametrize("call", [
    _pack(H=0), _pack(W=0), _pack(P=0), _unpack(H=0), _unpack(P=0),
    _render(H=1), _render(W=1), _render(P=0), _render(V=0), _ct(H=1), _ct(W=1), _ct(P=0), _ct(V=0)],
    ids=lambda c: c[0])
def test_bad_shapes_rejected(call):
    _rejected(call, "bad shape")


@pytest.mark.parametrize("a,b", [(5, 3), (-1, 4), (0, 9), (4, 4)])
def test_bad_plane_range_rejected(a, b):
    _rejected(_ct(a=a, b=b), "plane range")


@pytest.mark.parametrize("call", [
    _pack(packed=ctypes.c_void_p(4)), _unpack(packed=ctypes.c_void_p(4)), _unpack(out=ctypes.c_void_p(8)),
    _render(packed=ctypes.c_void_p(4)), _ct(packed=ctypes.c_void_p(4)), _ct(ct=ctypes.c_void_p(8))],
    ids=lambda c: c[0])
def test_misaligned_rejected(call):
    _rejected(call, "alignment")


def test_accepts_8_byte_aligned_packed_in_the_dry_run():
    """8-byte (not 16-byte) alignment is the contract: nothing is launched by mpiv_route."""
    name, grid = _lib.route("render_packed_f16", 16, 16, 2, 1)
    assert name.startswith("render_f16_kernel<") and grid > 0


def _grid(H, W, R, V):
    return -(-W // 64) * -(-H // (4 * R)) * V * 256


@pytest.mark.parametrize("entry,ct", [("render_packed_f16", "false"), ("render_packed_f16_ct", "true")])
def test_routes(entry, ct):
    """Config 4 at one view: 4 rows with vertical tap reuse, 4 rows in flight (1024 blocks leave
    the SIMDs few waves); at 125 views: 2 in flight.  A stretched small launch takes 2 plain rows,
    a stretched launch that fills the chip the reuse kernel."""
    assert _lib.route(entry, 1024, 1024, 128, 1) == (f"render_f16_kernel<{ct}, 4, true, 4>", _grid(1024, 1024, 4, 1))
    assert _lib.route(entry, 1024, 1024, 128, 125) == (f"render_f16_kernel<{ct}, 4, true, 2>",
                                                       _grid(1024, 1024, 4, 125))
    assert _lib.route(entry, 576, 1024, 32, 1) == (f"render_f16_kernel<{ct}, 2, false, 2>", _grid(576, 1024, 2, 1))
    assert _lib.route(entry, 576, 1024, 32, 64) == (f"render_f16_kernel<{ct}, 4, true, 2>", _grid(576, 1024, 4, 64))
    with pytest.raises(RuntimeError, match="bad shape"):
        _lib.route(entry, 1, 1024, 128, 1)


def test_python_layer_refuses_cpu_and_other_dtypes():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.pack_planes_f16(torch.zeros((4, 4, 2, 4), dtype=torch.float16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.render_packed_f16(torch.zeros((2, 8, 8, 4), dtype=torch.float16), torch.zeros((1, 2, 9)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.unpack_planes_f16(torch.zeros((2, 8, 8, 4), dtype=torch.float16))
    for bad in (torch.zeros((4, 4, 2, 4)), torch.zeros((4, 4, 2, 4), dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match="float16"):
            _lib.pack_planes_f16(bad)
    with pytest.raises(RuntimeError, match="float16"):
        _lib.render_packed_f16(torch.zeros((2, 8, 8, 4)), torch.zeros((1, 2, 9)))
