"""ctypes binding to libmpiv.so (C ABI: include/mpiv.h) + tensor plumbing.

Every function here launches a hand-written gfx950 kernel on the caller's
current torch stream.  There is no CPU fallback: without a ROCm device or
without the built library these functions raise.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import hashlib
import os
import weakref

import torch
from torch.autograd.function import once_differentiable

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPIV_LIB: another build of the same ABI (kernel A/B tools only, tools/gpu_ab_lib.sh);
# its build id is not checked against the sources in this tree
LIB_PATH = os.environ.get("MPIV_LIB") or os.path.join(_HERE, "libmpiv.so")
# the A/B flavour of the same sources (Makefile: -DMPIV_AB=1): the production kernels plus the
# variants kept for measurement; loaded only while a debug option selects one of them
AB_PATH = os.path.join(_HERE, "libmpiv_ab.so")
_CSRC = os.path.join(_HERE, "csrc")

_c_i64p = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p
_int = ctypes.c_int
_i64 = ctypes.c_int64

# name -> argtypes (mirrors include/mpiv.h)
_SIGS = {
    "mpiv_render": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp],
    "mpiv_pack_planes": [_vp, _c_i64p, _int, _int, _int, _vp, _vp],
    "mpiv_render_packed": [_vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_render_packed_lds": [_vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_render_packed_ct": [_vp, _int, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_render_packed_ct_rows": [_vp, _int, _int, _int, _int, _int, _int, _vp, _int, _int, _int, _vp, _vp],
    "mpiv_combine_ct": [_vp, _int, _i64, _vp, _vp],
    "mpiv_plane_sweep": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "mpiv_plane_sweep_pose": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _i64, _vp, _vp, _vp, _int, _int, _int,
                              _vp, _vp],
    "mpiv_inverse_warp": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _c_i64p, _int, _int, _vp, _vp],
    "mpiv_grid_sample": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _c_i64p, _int, _int, _vp, _c_i64p, _vp],
    "mpiv_over_composite": [_vp, _int, _i64, _i64, _i64, _vp, _vp],
    "mpiv_transform_points": [_vp, _int, _i64, _vp, _vp, _vp],
    "mpiv_normalize_homogeneous": [_vp, _i64, _int, _vp, _vp],
    "mpiv_pixel2cam": [_vp, _vp, _vp, _int, _i64, _int, _vp, _vp],
    "mpiv_cam2pixel": [_vp, _vp, _int, _i64, _vp, _vp],
    "mpiv_plane_coords": [_vp, _int, _i64, _vp, _int, _int, _vp, _vp],
    "mpiv_selftest_div_const": [_int, _vp, _vp],
    "mpiv_selftest_tickets": [_int, _int, _int, ctypes.c_uint, _vp, _vp, _vp],
    "mpiv_probe_gather": [_vp, ctypes.c_size_t, _int, _int, _vp, _vp],
    "mpiv_mark": [_int, _vp],
    "mpiv_route": [ctypes.c_char_p, _c_i64p, _int, ctypes.c_char_p, _int, _c_i64p],
    "mpiv_pad_texels": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp],
    "mpiv_plane_sweep_padded": [_vp, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int, _vp, _vp],
    "mpiv_preprocess": [_vp, _i64, _vp, _vp],
    "mpiv_deprocess_u8": [_vp, _i64, _vp, _vp],
    "mpiv_render_backward": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp],
    "mpiv_render_backward_watched": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                     _vp],
    "mpiv_render_backward_status": [_vp, _int, _int, _int, ctypes.POINTER(_int), _vp],
    "mpiv_render_train": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _vp],
    "mpiv_render_packed_census": [_vp, _int, _int, _int, _vp, _int, _vp, _vp, _vp],
    "mpiv_plane_sweep_into": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int, _vp, _i64, _i64,
                              _vp],
    "mpiv_plane_sweep_padded_into": [_vp, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int, _vp, _i64, _i64,
                                     _vp],
    "mpiv_assemble_mpi": [_vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp],
    "mpiv_assemble_mpi_packed": [_vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp],
    "mpiv_assemble_mpi_sampled": [_vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp],
    "mpiv_render_homographies": [_vp, _vp, _vp, _vp, _int, _int, _vp],
    "mpiv_render_homographies_device": [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp],
    "mpiv_psv_proj": [_vp, _i64, _vp, _int, _vp],
    "mpiv_psv_proj_device": [_vp, _i64, _vp, _int, _vp, _vp],
    "mpiv_pack_planes_u8": [_vp, _c_i64p, _int, _int, _int, _vp, _vp],
    "mpiv_render_net_output": [_vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp],
    "mpiv_render_net_output_train": [_vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _vp],
    "mpiv_render_packed_u8": [_vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_render_packed_u8_ct": [_vp, _int, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_synth_mpi_packed_u8": [ctypes.c_uint32, _int, _int, _int, _int, _vp, _vp],
    "mpiv_unpack_planes_u8": [_vp, _int, _int, _int, _vp, _vp],
    "mpiv_synth_mpi_packed": [ctypes.c_uint32, _int, _int, _int, _int, _vp, _vp],
    "mpiv_assemble_mpi_backward": [_vp, _c_i64p, _vp, _c_i64p, _vp, _c_i64p, _int, _int, _int, _int, _vp, _vp,
                                   _vp],
    "mpiv_tile_order": [_int, _int, _int, ctypes.POINTER(ctypes.c_int32)],
    "mpiv_pack_planes_f16": [_vp, _c_i64p, _int, _int, _int, _vp, _vp],
    "mpiv_unpack_planes_f16": [_vp, _int, _int, _int, _vp, _vp],
    "mpiv_render_packed_f16": [_vp, _int, _int, _int, _vp, _int, _vp, _vp],
    "mpiv_render_packed_f16_ct": [_vp, _int, _int, _int, _int, _int, _int, _vp, _int, _vp, _vp],
}
# mpiv_render_backward_cam (render_bwd_cam.hip): bound like the entries above.  It is listed on its own
# because tests/stream_cases.py holds one replay case per _SIGS entry; this entry's side-stream and
# graph-replay cases are in tests/test_camgrad_gpu.py.
_SIGS_CAM = {
    "mpiv_render_backward_cam": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                 _int, _vp],
}
# the alpha-only render under per-plane colours (render_texel.hip TexA32): on their own for the same
# reason; their side-stream and graph-replay cases are in tests/test_planecolor_gpu.py.
_SIGS_ALPHA = {
    "mpiv_pack_planes_alpha": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp],
    "mpiv_render_packed_alpha": [_vp, _int, _int, _int, _vp, _vp, _int, _vp, _vp],
}
# training through a half MPI read in place (render_chunk.hip InF16): the float entries' arguments with
# half rgba_layers / d rgba_layers; on their own for the same reason, their side-stream and graph-replay
# cases are in tests/test_f16_train_gpu.py.
_SIGS_F16_TRAIN = {
    "mpiv_render_train_f16": _SIGS["mpiv_render_train"],
    "mpiv_render_backward_f16": _SIGS["mpiv_render_backward"],
    "mpiv_render_backward_watched_f16": _SIGS["mpiv_render_backward_watched"],
    "mpiv_render_backward_cam_f16": _SIGS_CAM["mpiv_render_backward_cam"],
}
# the inverse warp's adjoint (warp_bwd.hip): on its own for the same reason; its side-stream and graph-replay
# cases are in tests/test_warpgrad_gpu.py.
_SIGS_WARP = {
    "mpiv_inverse_warp_backward": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _c_i64p, _int, _int, _vp,
                                   _c_i64p, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp],
}
# the plane sweep's adjoint (psv_bwd.hip): on its own for the same reason; its side-stream and graph-replay
# cases are in tests/test_psvgrad_gpu.py.
_SIGS_PSV = {
    "mpiv_plane_sweep_backward": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _vp, _vp, _int, _int, _int, _vp,
                                  _c_i64p, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp],
}
# the sampler's and the compositor's adjoints (helper_bwd.hip): on their own for the same reason; their
# side-stream and graph-replay cases are in tests/test_helpergrad_gpu.py.
_SIGS_HELPER_BWD = {
    "mpiv_grid_sample_backward": [_vp, _c_i64p, _int, _int, _int, _int, _vp, _c_i64p, _int, _int, _vp, _c_i64p, _vp,
                                  _vp, _vp, ctypes.c_size_t, _vp],
    "mpiv_over_composite_backward": [_vp, _int, _i64, _i64, _i64, _vp, _c_i64p, _vp, _vp, ctypes.c_size_t, _vp],
}
# the matmul helpers with the chain as an argument (geometry.hip dot<>): on their own for the same reason.
# They launch the kernels of the entries without `plain`, whose side-stream and graph-replay cases cover
# them; tests/test_geometry_gpu.py runs both chains.
_SIGS_CHAIN = {
    "mpiv_transform_points_chain": [_vp, _int, _i64, _vp, _int, _vp, _vp],
    "mpiv_pixel2cam_chain": [_vp, _vp, _vp, _int, _i64, _int, _int, _vp, _vp],
    "mpiv_cam2pixel_chain": [_vp, _vp, _int, _i64, _int, _vp, _vp],
    "mpiv_plane_coords_chain": [_vp, _int, _i64, _vp, _int, _int, _int, _vp, _vp],
}
# the packed renders into a target frame of its own size (render.hip RenderGeomT): on their own for the same
# reason; their side-stream and graph-replay cases are in tests/test_target_gpu.py.
_SIGS_TGT = {
    "mpiv_render_packed_tgt": [_vp, _int, _int, _int, _vp, _int, _int, _int, _vp, _vp],
    "mpiv_render_packed_u8_tgt": [_vp, _int, _int, _int, _vp, _int, _int, _int, _vp, _vp],
    "mpiv_render_packed_f16_tgt": [_vp, _int, _int, _int, _vp, _int, _int, _int, _vp, _vp],
}
EXPORTS = tuple(_SIGS) + tuple(_SIGS_CAM) + tuple(_SIGS_ALPHA) + tuple(_SIGS_TGT) + tuple(_SIGS_F16_TRAIN) + tuple(_SIGS_WARP) + tuple(_SIGS_PSV) + tuple(_SIGS_HELPER_BWD) + tuple(_SIGS_CHAIN) + (
                          "mpiv_grid_sample_backward_workspace_size", "mpiv_over_composite_backward_workspace_size",
                          "mpiv_plane_sweep_backward_workspace_size", "mpiv_plane_sweep_backward_workspace_size_min",
                          "mpiv_inverse_warp_backward_workspace_size","mpiv_abi_version", "mpiv_last_error", "mpiv_render_backward_workspace_size",
                          "mpiv_render_backward_abort_flag",
                          "mpiv_render_backward_workspace_size_min", "mpiv_render_backward_cam_workspace_size",
                          "mpiv_render_backward_cam_workspace_size_min", "mpiv_build_id", "mpiv_debug_set")
ABI_VERSION = 17

_lib = None
_lib_ab = None
_override = None  # the A/B library while a debug option selects an A/B kernel

# How mpi_render_view_torch renders a non-broadcast MPI batch: "auto" (the in-place
# chunked kernel when the layout allows it, else pack per view when P >= 8, else read in
# place), "pack", or "native" (mpiv_render, which picks its in-place kernel itself).
RENDER_POLICY = "auto"

_KOOB = 0x7FFFFF00
_CHUNK_LDS = 65536


def chunk_layout_ok(rgba_layers: torch.Tensor) -> bool:
    """True when mpiv_render reads this [B,H,W,P,4] tensor with render_chunk_kernel
    (abi.hip: planes contiguous per pixel, 16-B texels, offsets below the buffer range)."""
    B, H, W, P, C = rgba_layers.shape
    st = rgba_layers.stride()
    if C != 4 or H < 2 or W < 2 or st[4] != 1 or st[3] != 4 or any(s % 4 for s in st[:3]):
        return False
    if rgba_layers.data_ptr() % 16:
        return False
    CH = 4 if P <= 4 else 8
    rec = ((H - 1) * st[1] + (W - 1) * st[2]) * 4 + CH * 16
    return (rec < _KOOB and st[1] // 4 < (1 << 22) and st[2] // 4 < (1 << 22)
            and 4 * 64 * (CH + 1) * 16 + P * 36 <= _CHUNK_LDS)


def source_hash() -> str | None:
    """sha256 (first 16 hex digits) of the library sources listed in csrc/SOURCES, in order
    -- the id the Makefile compiles into libmpiv.so; None when the sources are absent."""
    try:
        with open(os.path.join(_CSRC, "SOURCES")) as f:
            names = f.read().split()
        h = hashlib.sha256()
        for n in names:
            with open(os.path.join(_CSRC, n), "rb") as f:
                h.update(f.read())
        return h.hexdigest()[:16]
    except OSError:
        return None


def _open(path: str, check_id: bool):
    if not os.path.exists(path):
        raise RuntimeError(f"mpi_vision_amd: {path} is missing -- build it first "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    L = ctypes.CDLL(path)
    L.mpiv_build_id.restype = ctypes.c_char_p
    want = source_hash()
    if check_id and want is not None and L.mpiv_build_id().decode() != want:
        raise RuntimeError(f"mpi_vision_amd: {path} was built from other sources (build id "
                           f"{L.mpiv_build_id().decode()}, sources {want}) -- rebuild it "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    L.mpiv_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.mpiv_debug_set.restype = ctypes.c_int
    for name, args in (*_SIGS.items(), *_SIGS_CAM.items(), *_SIGS_ALPHA.items(), *_SIGS_F16_TRAIN.items(),
                       *_SIGS_WARP.items(), *_SIGS_PSV.items(), *_SIGS_HELPER_BWD.items(), *_SIGS_CHAIN.items(),
                       *_SIGS_TGT.items()):
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    L.mpiv_abi_version.restype = ctypes.c_int
    L.mpiv_last_error.restype = ctypes.c_char_p
    L.mpiv_render_backward_workspace_size.argtypes = [_int, _int, _int]
    L.mpiv_render_backward_workspace_size.restype = ctypes.c_size_t
    L.mpiv_render_backward_workspace_size_min.argtypes = [_int, _int, _int]
    L.mpiv_render_backward_workspace_size_min.restype = ctypes.c_size_t
    for fn in (L.mpiv_render_backward_cam_workspace_size, L.mpiv_render_backward_cam_workspace_size_min):
        fn.argtypes = [_int, _int, _int]
        fn.restype = ctypes.c_size_t
    L.mpiv_inverse_warp_backward_workspace_size.argtypes = [_int] * 6
    L.mpiv_inverse_warp_backward_workspace_size.restype = ctypes.c_size_t
    for fn in (L.mpiv_plane_sweep_backward_workspace_size, L.mpiv_plane_sweep_backward_workspace_size_min):
        fn.argtypes = [_int] * 7
        fn.restype = ctypes.c_size_t
    L.mpiv_grid_sample_backward_workspace_size.argtypes = [_int] * 6
    L.mpiv_grid_sample_backward_workspace_size.restype = ctypes.c_size_t
    L.mpiv_over_composite_backward_workspace_size.argtypes = [_int, _i64]
    L.mpiv_over_composite_backward_workspace_size.restype = ctypes.c_size_t
    L.mpiv_render_backward_abort_flag.argtypes = [_int]
    L.mpiv_render_backward_abort_flag.restype = ctypes.c_void_p
    if L.mpiv_abi_version() != ABI_VERSION:
        raise RuntimeError(f"mpi_vision_amd: {path} ABI version mismatch")
    return L


def load_main():
    """The production libmpiv.so (raises if it has not been built, or was built from other
    sources than the ones in this tree)."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH, not os.environ.get("MPIV_LIB"))
    return _lib


def load_ab():
    """libmpiv_ab.so, the A/B flavour (same sources, -DMPIV_AB=1).  Under MPIV_LIB (an A/B
    tool's own build, which compiles every variant) that library serves both roles."""
    global _lib_ab
    if os.environ.get("MPIV_LIB"):
        return load_main()
    if _lib_ab is None:
        _lib_ab = _open(AB_PATH, True)
    return _lib_ab


def load():
    """The library entry points run through: libmpiv.so, or libmpiv_ab.so while a debug
    option selects an A/B kernel (set_debug)."""
    return _override if _override is not None else load_main()


# MPIV_ROCTX=1: every entry-point call is wrapped in a roctx range named after it, so
# `rocprofv3 --marker-trace --kernel-trace` attributes each kernel to its drop-in call
# (tracing only; off by default: no overhead on the launch path).
_ROCTX = None
if os.environ.get("MPIV_ROCTX") == "1":
    try:
        _ROCTX = ctypes.CDLL("/opt/rocm/lib/libroctx64.so")
        _ROCTX.roctxRangePushA.argtypes = [ctypes.c_char_p]
    except OSError:
        _ROCTX = None


# entry points whose only kernels are A/B variants (libmpiv.so refuses them)
_AB_ENTRIES = frozenset({"mpiv_render_packed_lds"})


def _call(name, *args):
    """Call an entry point (an A/B-only one on libmpiv_ab.so).  Tensor arguments are passed as their device pointers and
    stay referenced (alive) for the duration of the call, so temporaries built inline
    cannot be freed and their memory reused by a later argument's allocation."""
    L = load_ab() if name in _AB_ENTRIES else load()
    # (tensor arguments as plain ints: every pointer parameter's argtype is c_void_p)
    cargs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if _ROCTX is not None:
        _ROCTX.roctxRangePushA(name.encode())
        try:
            rc = getattr(L, name)(*cargs)
        finally:
            _ROCTX.roctxRangePop()
    else:
        rc = getattr(L, name)(*cargs)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {L.mpiv_last_error().decode()}")


_DEBUG_GEN = 0  # bumped by every set_debug / reset_debug: memos of option-dependent values key on it


def set_debug(**opts):
    """Select non-default kernel variants (tests and A/B tools only; mpiv_debug_set).
    Options that pick a kernel kept for A/B measurement are refused by the production
    library; then the A/B flavour takes them and runs every entry point until reset_debug()."""
    global _override, _DEBUG_GEN
    _DEBUG_GEN += 1
    L = load_main()
    need_ab = False
    for k, v in opts.items():
        if L.mpiv_debug_set(k.encode(), int(v)) != 0:
            msg = L.mpiv_last_error().decode()
            if "libmpiv_ab.so" not in msg:
                L.mpiv_debug_set(b"reset", 0)
                raise ValueError(msg)
            need_ab = True
    if need_ab or (_override is not None and _override is not L):
        # the A/B flavour runs (now, or still from an earlier call): the options go to it too,
        # so successive calls accumulate on whichever library serves the entry points
        if need_ab:
            L.mpiv_debug_set(b"reset", 0)
        A = load_ab()
        for k, v in opts.items():
            if A.mpiv_debug_set(k.encode(), int(v)) != 0:
                msg = A.mpiv_last_error().decode()
                A.mpiv_debug_set(b"reset", 0)
                raise ValueError(msg)
        _override = A


def reset_debug():
    """Every option back to its production default; entry points back on libmpiv.so."""
    global _override, _DEBUG_GEN
    _DEBUG_GEN += 1
    for L in (_lib, _lib_ab):
        if L is not None:
            L.mpiv_debug_set(b"reset", 0)
    _override = None


@contextlib.contextmanager
def debug(**opts):
    """set_debug(**opts) for the duration of the block, e.g.
    ``with _lib.debug(render_mv=1, box_shrink=2): ...``; reset_debug() on exit."""
    try:
        set_debug(**opts)
        yield
    finally:
        reset_debug()


def tile_order(ntiles: int, tiles_x: int, order: int) -> list[int]:
    """The sampling kernels' tile order on the host (mpiv_tile_order, no GPU needed): entry t is the
    raster tile rendered at position t of the XCD-contiguous numbering; order -1 band, 1 interleaved."""
    L = load_main()
    out = (ctypes.c_int32 * max(ntiles, 1))()
    rc = L.mpiv_tile_order(ntiles, tiles_x, order, out)
    if rc != 0:
        raise RuntimeError(f"mpiv_tile_order failed ({rc}): {L.mpiv_last_error().decode()}")
    return list(out[:ntiles])


def route(entry: str, *args: int) -> tuple[str, int]:
    """(kernel name, grid work-items) of the kernel an entry point's production dispatch
    would launch for these sizes (mpiv_route: a dry run, nothing launched, no GPU needed)."""
    L = load_main()
    buf = ctypes.create_string_buffer(160)
    grid = ctypes.c_int64(0)
    a = (ctypes.c_int64 * len(args))(*args)
    rc = L.mpiv_route(entry.encode(), a, len(args), buf, len(buf), ctypes.byref(grid))
    if rc != 0:
        raise RuntimeError(f"mpiv_route failed ({rc}): {L.mpiv_last_error().decode()}")
    return buf.value.decode(), grid.value


def _strides(t: torch.Tensor, dims=None):
    st = t.stride() if dims is None else [t.stride(d) for d in dims]
    return (ctypes.c_int64 * len(st))(*st)


def _dev(*tensors, f16_first: bool = False):
    """All tensors must be fp32 on one ROCm device; returns that device.  f16_first: the first one (the
    MPI of the training entries) may be float16 instead."""
    dev = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError("mpi_vision_amd kernels need ROCm device tensors "
                               f"(got a tensor on {t.device}); there is no CPU path")
        if t.dtype != torch.float32 and not (f16_first and t is tensors[0] and t.dtype == torch.float16):
            raise RuntimeError(f"expected scalar type Float but found {t.dtype}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} and {t.device}")
    return dev


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev):
    """The current stream of dev as the hipStream_t the entry points take (the raw handle, without
    building a torch Stream object: this runs on every launch)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(dev.index if dev.index is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def host_under_capture(what: str) -> None:
    """Raise if the current stream is capturing a HIP graph: `what` names a per-call matrix argument
    that lives on the host.  Its upload would be recorded as a copy from a temporary host buffer
    (page-locked: gone by the first replay; pageable: not capturable at all), and every replay would
    read whatever is there then."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"mpi_vision_amd: {what} is a host (CPU) tensor; under a HIP-graph capture every per-call "
                           "matrix must be a device tensor (a static input of the graph), because a captured "
                           "upload would read a temporary host buffer on every replay")


def _up(x: torch.Tensor, dev, what: str = "a matrix argument") -> torch.Tensor:
    """Upload a small host-computed matrix buffer (contiguous fp32).  A page-locked host
    buffer is copied asynchronously on the current stream (torch's pinned allocator keeps
    it alive until that copy has run).  Under a HIP-graph capture a host buffer raises
    (host_under_capture), before anything is launched."""
    if x.device.type == "cpu":
        host_under_capture(what)
        if x.is_pinned() and x.dtype == torch.float32 and x.is_contiguous():
            return x.to(device=dev, non_blocking=True)
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _p(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr())


def _check_out(out: torch.Tensor, shape, dev, what: str) -> torch.Tensor:
    """A caller-supplied output must be a contiguous fp32 tensor of exactly `shape` on
    `dev` (the kernels write it densely; anything else would be out-of-bounds writes)."""
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or not out.is_contiguous()
            or out.dtype != torch.float32 or out.device != dev):
        got = (tuple(out.shape), out.dtype, out.device, out.is_contiguous()) if isinstance(out, torch.Tensor) \
            else type(out).__name__
        raise RuntimeError(f"{what}: out must be a contiguous float32 {tuple(shape)} tensor on {dev}, got {got}")
    return out


# ---------------------------------------------------------------------------
# render
# ---------------------------------------------------------------------------

PAD = 2  # zero-border texels around every packed plane (include/mpiv.h)


def packed_shape(H: int, W: int, P: int):
    return (P, H + 2 * PAD, W + 2 * PAD, 4)


def packed_hw(packed: torch.Tensor):
    """(P, H, W) of a packed MPI [P, H+4, W+4, 4]."""
    if packed.dim() != 4 or packed.shape[-1] != 4 or not packed.is_contiguous():
        raise RuntimeError(f"packed MPI must be a contiguous [P, H+4, W+4, 4] tensor, got {tuple(packed.shape)}")
    return packed.shape[0], packed.shape[1] - 2 * PAD, packed.shape[2] - 2 * PAD


def pack_planes(view: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """One MPI view [H, W, P, 4] (any strides) -> packed plane-major [P, H+4, W+4, 4]
    with a 2-texel zero border (image texel (x, y) of plane p at [p, y+2, x+2])."""
    dev = _dev(view)
    H, W, P, C = view.shape
    if C != 4:
        raise RuntimeError(f"MPI texels must have 4 channels (RGBA), got {C}")
    packed = torch.empty(packed_shape(H, W, P), device=dev, dtype=torch.float32) if out is None else \
        _check_out(out, packed_shape(H, W, P), dev, "pack_planes")
    _call("mpiv_pack_planes", view, _strides(view), H, W, P, packed, _stream(dev))
    return packed


def synth_mpi_packed(seed: int, H: int, W: int, p_begin: int, p_end: int, device,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """Planes [p_begin, p_end) of the counter-based synthetic MPI `seed` (synth.hip),
    generated on `device` straight into the packed layout [p_end-p_begin, H+4, W+4, 4]."""
    dev = torch.device(device)
    shape = packed_shape(H, W, p_end - p_begin)
    packed = torch.empty(shape, device=dev, dtype=torch.float32) if out is None else \
        _check_out(out, shape, dev, "synth_mpi_packed")
    _dev(packed)
    _call("mpiv_synth_mpi_packed", ctypes.c_uint32(seed & 0xFFFFFFFF), H, W, p_begin, p_end, packed, _stream(dev))
    return packed


# ---- narrow-texel MPIs: 8-bit and half-precision RGBA (csrc/render_texel.hip) ----
#
# Views per launch from which a narrow MPI is rendered through its exact float copy (the float rows
# kernel; the copy is memoised, packed_float_copy).  These are steady-state kernel times: the
# thresholds are for a packed MPI that is rendered again and again.
# u8: the float rows kernel at 125 views: 26.6 ms vs 29.8 for the u8 kernel, VALU-bound on the exact
# per-tap conversion; at one view the u8 kernel reads 4x fewer bytes and wins, 0.31 vs 0.38 ms.
U8_FLOAT_MIN_VIEWS = int(os.environ.get("MPIV_U8_FLOAT_MIN_VIEWS", "32"))
# f16: on config 4 the f16 kernel wins up to 4 views (one view 0.265 vs 0.376 ms for the float kernel),
# the float rows kernel from 8 (1.49 vs 1.56 ms; 125 views 20.2 vs 23.4), on config 2 from 8 too
# (0.147 vs 0.190) (profiles/f16_render.jsonl, DESIGN.md §4 "f16 texels").  A caller that packs,
# renders ONE launch and drops the MPI (mpi_render_view_f16) pays the copy (0.52 ms at config 4) every
# time: copy + float kernel beat the f16 kernel only from F16_FLOAT_ONCE_MIN_VIEWS views (config 4 at
# 32 views 5.50 + 0.52 vs 6.00 ms, a tie; at 64 views 10.46 + 0.52 vs 11.96).
F16_FLOAT_MIN_VIEWS = int(os.environ.get("MPIV_F16_FLOAT_MIN_VIEWS", "8"))
F16_FLOAT_ONCE_MIN_VIEWS = 64

# A format: its name in the entry points (mpiv_pack_planes_<name>, mpiv_unpack_planes_<name>,
# mpiv_render_packed_<name>[_ct]), the dtype of the caller's [H, W, P, 4] view, the packed tensor
# ([P, H+4, W+4] + tail, of dtype packed) and the float-route threshold.
_Tex = collections.namedtuple("_Tex", "name view packed tail float_min_views")
_U8 = _Tex("u8", torch.uint8, torch.int32, (), U8_FLOAT_MIN_VIEWS)  # a texel: one word, RGBA bytes, R lowest
_F16 = _Tex("f16", torch.float16, torch.float16, (4,), F16_FLOAT_MIN_VIEWS)  # a texel: 4 halves, 8 B


def _dt(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def _tex_pack(t: _Tex, view: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
    what = f"pack_planes_{t.name}"
    if not isinstance(view, torch.Tensor):
        raise TypeError(f"expected a torch.Tensor, got {type(view).__name__}")
    if view.dtype != t.view:
        raise RuntimeError(f"{what} expects a {_dt(t.view)} [H, W, P, 4] tensor, got {view.dtype}")
    if view.device.type != "cuda":
        raise RuntimeError("mpi_vision_amd kernels need ROCm device tensors; there is no CPU path")
    dev = view.device
    H, W, P, C = view.shape
    if C != 4:
        raise RuntimeError(f"MPI texels must have 4 channels (RGBA), got {C}")
    shape = (P, H + 2 * PAD, W + 2 * PAD) + t.tail
    if out is None:
        packed = torch.empty(shape, device=dev, dtype=t.packed)
    elif tuple(out.shape) != shape or out.dtype != t.packed or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"{what}: out must be a contiguous {_dt(t.packed)} {shape} tensor on {dev}")
    else:
        packed = out
    _call(f"mpiv_{what}", view, _strides(view), H, W, P, packed, _stream(dev))
    if out is not None:
        _wrote(packed)
    return packed


def _tex_hw(t: _Tex, packed: torch.Tensor):
    """(P, H, W) of a packed narrow MPI, after checking that it is one."""
    if not isinstance(packed, torch.Tensor):
        raise TypeError(f"expected a torch.Tensor, got {type(packed).__name__}")
    if (packed.dtype != t.packed or packed.dim() != 3 + len(t.tail) or tuple(packed.shape[3:]) != t.tail
            or not packed.is_contiguous()):
        layout = ", ".join(("P", "H+4", "W+4") + tuple(map(str, t.tail)))
        raise RuntimeError(f"packed {t.name} MPI must be a contiguous {_dt(t.packed)} [{layout}] tensor, got "
                           f"{packed.dtype} {tuple(packed.shape)}")
    if packed.device.type != "cuda":
        raise RuntimeError("mpi_vision_amd kernels need ROCm device tensors; there is no CPU path")
    return packed.shape[0], packed.shape[1] - 2 * PAD, packed.shape[2] - 2 * PAD


def _tex_unpack(t: _Tex, packed: torch.Tensor) -> torch.Tensor:
    P, H, W = _tex_hw(t, packed)
    out = torch.empty(packed_shape(H, W, P), device=packed.device, dtype=torch.float32)
    _call(f"mpiv_unpack_planes_{t.name}", packed, H, W, P, out, _stream(packed.device))
    return out


def _render_views(what: str, packed: torch.Tensor, phw, homs: torch.Tensor, out: torch.Tensor | None, size=None):
    """mpiv_<what>: a packed MPI of any format + homs [V,P,9] (host or device) -> [V,H,W,3]; with
    size = (Ht, Wt), mpiv_<what>_tgt: a target frame of its own size [V,Ht,Wt,3]."""
    P, H, W = phw
    dev = packed.device
    V = homs.shape[0]
    h = _up(homs.reshape(V, P, 9), dev, "homs")
    Ht, Wt = (H, W) if size is None else _target_size(size)
    if out is None:
        out = torch.empty((V, Ht, Wt, 3), device=dev, dtype=torch.float32)
    else:
        _check_out(out, (V, Ht, Wt, 3), dev, what)
    if V == 0:
        return out
    if size is None:
        _call(f"mpiv_{what}", packed, H, W, P, h, V, out, _stream(dev))
    else:
        _call(f"mpiv_{what}_tgt", packed, H, W, P, h, V, Ht, Wt, out, _stream(dev))
    return out


def _target_size(size):
    """(Ht, Wt) of a render's size= argument: two positive ints."""
    try:
        Ht, Wt = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"size must be (target height, target width), got {size!r}") from None
    if Ht <= 0 or Wt <= 0:
        raise RuntimeError(f"size must be (target height, target width) > 0, got {size!r}")
    return Ht, Wt


def _render_views_ct(what: str, packed: torch.Tensor, phw, homs: torch.Tensor, back: bool, p_begin: int,
                     p_end: int | None, out: torch.Tensor | None):
    """mpiv_<what>: the plane-range partial (C, T) [V,H,W,4] of a packed MPI of any format."""
    P, H, W = phw
    dev = packed.device
    p_end = P if p_end is None else p_end
    V = homs.shape[0]
    h = _up(homs.reshape(V, P, 9), dev, "homs")
    if out is None:
        out = torch.empty((V, H, W, 4), device=dev, dtype=torch.float32)
    else:
        _check_out(out, (V, H, W, 4), dev, what)
    _call(f"mpiv_{what}", packed, H, W, P, p_begin, p_end, int(back), h, V, out, _stream(dev))
    return out


def _tex_render(t: _Tex, packed: torch.Tensor, homs: torch.Tensor, out: torch.Tensor | None,
                route_float: bool | None, size=None) -> torch.Tensor:
    phw = _tex_hw(t, packed)
    if route_float is None:
        route_float = homs.shape[0] >= t.float_min_views
    if route_float:
        if homs.device.type == "cpu":
            host_under_capture("homs")  # (before the float copy is launched)
        return render_packed(packed_float_copy(packed), homs, out=out, size=size)
    return _render_views(f"render_packed_{t.name}", packed, phw, homs, out, size)


def pack_planes_u8(view: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """One 8-bit MPI view [H, W, P, 4] uint8 (any strides) -> packed u8 planes
    [P, H+4, W+4] int32 (RGBA bytes of each texel, R lowest) with the zero border."""
    return _tex_pack(_U8, view, out)


def pack_planes_f16(view: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """One half-precision MPI view [H, W, P, 4] float16 (any strides) -> packed f16 planes
    [P, H+4, W+4, 4] float16 (8-B texels) with the zero border."""
    return _tex_pack(_F16, view, out)


def synth_mpi_packed_u8(seed: int, H: int, W: int, p_begin: int, p_end: int, device) -> torch.Tensor:
    """Planes [p_begin, p_end) of the counter-based synthetic u8 MPI `seed`, packed u8."""
    dev = torch.device(device)
    packed = torch.empty((p_end - p_begin, H + 2 * PAD, W + 2 * PAD), device=dev, dtype=torch.int32)
    _call("mpiv_synth_mpi_packed_u8", ctypes.c_uint32(seed & 0xFFFFFFFF), H, W, p_begin, p_end, packed,
          _stream(dev))
    return packed


def _u8_hw(packed: torch.Tensor):
    return _tex_hw(_U8, packed)


def _f16_hw(packed: torch.Tensor):
    return _tex_hw(_F16, packed)


def unpack_planes_u8(packed: torch.Tensor) -> torch.Tensor:
    """packed u8 [P,H+4,W+4] -> the packed float MPI [P,H+4,W+4,4] of u8.float() / 255 (exact)."""
    return _tex_unpack(_U8, packed)


def unpack_planes_f16(packed: torch.Tensor) -> torch.Tensor:
    """packed f16 [P,H+4,W+4,4] -> the packed float MPI [P,H+4,W+4,4] of mpi.float() (exact)."""
    return _tex_unpack(_F16, packed)


_U8_FLOAT: dict = {}  # device -> (key, weak reference to the u8 / f16 MPI, its float copy)


def _wrote(t: torch.Tensor) -> None:
    """A kernel wrote t through ctypes (an out= argument): bump its version counter as a torch
    in-place op would, so memos keyed on it (u8_float_copy) see the new contents."""
    torch.autograd.graph.increment_version(t)


def packed_float_copy(packed: torch.Tensor) -> torch.Tensor:
    """The packed float copy of a packed u8 or f16 MPI (by its dtype: int32 words / float16 texels),
    memoised per device on the tensor object, its storage, version counter and the current stream
    (a camera path converts its MPI once; an in-place edit, a refill through pack_planes_u8(out=) /
    pack_planes_f16(out=) or a new MPI converts again; a copy is only read on the stream that made
    it).  One entry per device, whatever the format: the copy is 4x the u8 MPI, 2x the f16 one
    (2.2 GB at config 4); it is dropped when its MPI is freed, or by clear_float_copies().  Under a
    HIP-graph capture the memo is neither read nor written: the conversion is captured."""
    dev = packed.device
    unpack = unpack_planes_f16 if packed.dtype == torch.float16 else unpack_planes_u8
    if torch.cuda.is_current_stream_capturing():
        # HIP-graph capture: the conversion is part of the graph, into a fresh tensor of the graph's own
        # pool -- the packed MPI is a static input whose contents change between replays, so a memo hit
        # must not skip it, and the memo's copy (freed by the next MPI) must not be captured
        return unpack(packed)
    key = (id(packed), packed.data_ptr(), packed._version, tuple(packed.shape),
           torch.cuda.current_stream(dev).cuda_stream)
    ent = _U8_FLOAT.get(dev)
    if ent is not None and ent[0] == key and ent[1]() is packed:
        return ent[2]
    _U8_FLOAT.pop(dev, None)  # free the old copy first
    f = unpack(packed)
    _U8_FLOAT[dev] = (key, weakref.ref(packed), f)
    weakref.finalize(packed, _drop_u8_float, dev, key)
    return f


def u8_float_copy(packed: torch.Tensor) -> torch.Tensor:
    """packed_float_copy of a packed u8 MPI."""
    _u8_hw(packed)
    return packed_float_copy(packed)


def f16_float_copy(packed: torch.Tensor) -> torch.Tensor:
    """packed_float_copy of a packed f16 MPI."""
    _f16_hw(packed)
    return packed_float_copy(packed)


def _drop_u8_float(dev, key) -> None:
    ent = _U8_FLOAT.get(dev)
    if ent is not None and ent[0] == key:
        del _U8_FLOAT[dev]


def clear_float_copies(device=None) -> None:
    """Free the memoised float copies of u8 and f16 MPIs (all devices, or `device`'s)."""
    if device is None:
        _U8_FLOAT.clear()
    else:
        _U8_FLOAT.pop(torch.device(device), None)


clear_u8_float_copies = clear_float_copies


def render_packed_u8(packed: torch.Tensor, homs: torch.Tensor, out: torch.Tensor | None = None,
                     route_float: bool | None = None, size=None) -> torch.Tensor:
    """packed u8 [P,H+4,W+4] + homs [V,P,9] -> [V,H,W,3] fp32, bit-identical to rendering the
    float MPI u8.float() / 255 (render_texel.hip).  Launches of >= U8_FLOAT_MIN_VIEWS views
    (route_float None) render the MPI's exact float copy (u8_float_copy, converted once per MPI)
    with the float kernel instead: the same bits, faster where the texture path binds.
    size = (Ht, Wt): a target frame of its own size [V,Ht,Wt,3] (render_packed)."""
    return _tex_render(_U8, packed, homs, out, route_float, size)


def render_packed_u8_ct(packed: torch.Tensor, homs: torch.Tensor, back: bool, p_begin: int = 0,
                        p_end: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Plane-range partial (C, T) [V,H,W,4] of a packed u8 MPI (plane sharding)."""
    return _render_views_ct("render_packed_u8_ct", packed, _u8_hw(packed), homs, back, p_begin, p_end, out)


def render_packed_f16(packed: torch.Tensor, homs: torch.Tensor, out: torch.Tensor | None = None,
                      route_float: bool | None = None, size=None) -> torch.Tensor:
    """packed f16 [P,H+4,W+4,4] + homs [V,P,9] -> [V,H,W,3] fp32, bit-identical to rendering the
    float MPI mpi.float() (render_texel.hip: half the texel bytes of the float render).  Launches of
    >= F16_FLOAT_MIN_VIEWS views (route_float None) render the MPI's exact float copy
    (f16_float_copy, converted once per MPI) with the float kernel instead: the same bits, faster
    where the texture path binds (it costs the float copy's memory, 2x the f16 MPI).
    size = (Ht, Wt): a target frame of its own size [V,Ht,Wt,3] (render_packed)."""
    return _tex_render(_F16, packed, homs, out, route_float, size)


def render_packed_f16_ct(packed: torch.Tensor, homs: torch.Tensor, back: bool, p_begin: int = 0,
                         p_end: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Plane-range partial (C, T) [V,H,W,4] of a packed f16 MPI (plane sharding)."""
    return _render_views_ct("render_packed_f16_ct", packed, _f16_hw(packed), homs, back, p_begin, p_end, out)


def pack_planes_alpha(view: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The alpha of one fp32 MPI view -- channel 3 of [H, W, P, 4], read in place through the view's
    strides, or a [H, W, P, 1] tensor -- -> packed alpha planes [P, H+4, W+4] float32 with the +0
    border (the packed u8 layout's geometry: 4 B per texel)."""
    dev = _dev(view)
    if view.dim() != 4 or view.shape[3] not in (1, 4):
        raise RuntimeError(f"pack_planes_alpha expects a [H, W, P, 4] or [H, W, P, 1] tensor, got {tuple(view.shape)}")
    H, W, P, C = view.shape
    shape = (P, H + 2 * PAD, W + 2 * PAD)
    if out is None:
        packed = torch.empty(shape, device=dev, dtype=torch.float32)
    else:
        packed = _check_out(out, shape, dev, "pack_planes_alpha")
    _call("mpiv_pack_planes_alpha", view, _strides(view), H, W, P, C - 1, packed, _stream(dev))
    if out is not None:
        _wrote(packed)
    return packed


def _alpha_hw(packed: torch.Tensor):
    """(P, H, W) of packed alpha planes, after checking that they are."""
    _dev(packed)
    if packed.dim() != 3 or not packed.is_contiguous():
        raise RuntimeError("packed alpha planes must be a contiguous float32 [P, H+4, W+4] tensor, got "
                           f"{tuple(packed.shape)}")
    return packed.shape[0], packed.shape[1] - 2 * PAD, packed.shape[2] - 2 * PAD


def render_packed_alpha(packed: torch.Tensor, colors: torch.Tensor, homs: torch.Tensor,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """packed alpha planes [P,H+4,W+4] + one colour per plane `colors` [P,3] + homs [V,P,9] (host or
    device) -> [V,H,W,3] fp32: bit-identical to render_packed on the float MPI whose RGB is colors[p]
    all over plane p and whose alpha is the packed channel, from a quarter of its bytes
    (render_texel.hip TexA32).  A colour tap outside the plane is +0 (the reference's zero padding),
    so the frame is NOT colour x coverage; -0, Inf and NaN colours propagate as in the float render."""
    P, H, W = _alpha_hw(packed)
    dev = packed.device
    if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (P, 3):
        raise RuntimeError(f"render_packed_alpha: colors must be a [{P}, 3] tensor, got "
                           f"{tuple(colors.shape) if isinstance(colors, torch.Tensor) else type(colors).__name__}")
    c = _up(colors, dev, "colors")
    V = homs.shape[0]
    h = _up(homs.reshape(V, P, 9), dev, "homs")
    if out is None:
        out = torch.empty((V, H, W, 3), device=dev, dtype=torch.float32)
    else:
        _check_out(out, (V, H, W, 3), dev, "render_packed_alpha")
    if V == 0:
        return out
    _call("mpiv_render_packed_alpha", packed, H, W, P, c, h, V, out, _stream(dev))
    return out


def unpack_planes(packed: torch.Tensor) -> torch.Tensor:
    """Inverse view of pack_planes: [P, H+4, W+4, 4] -> [H, W, P, 4] (a strided view)."""
    P, H, W = packed_hw(packed)
    return packed[:, PAD:PAD + H, PAD:PAD + W].permute(1, 2, 0, 3)


def render_packed(packed: torch.Tensor, homs: torch.Tensor, out: torch.Tensor | None = None,
                  size=None) -> torch.Tensor:
    """packed [P,H+4,W+4,4] + homs [V,P,9] (host or device) -> [V,H,W,3].
    size = (Ht, Wt): a target frame of its own size [V,Ht,Wt,3] (mpiv_render_packed_tgt): target
    pixel (x, y) of the Ht x Wt grid through homs, the source pixel coordinate it lands on
    normalised by the target's (Ht - 1, Wt - 1) as the reference's planar_transform_torch does and
    sampled over the packed H x W planes.  None: the same-size launch, untouched."""
    _dev(packed)
    return _render_views("render_packed", packed, packed_hw(packed), homs, out, size)


def render_packed_ct(packed: torch.Tensor, homs: torch.Tensor, back: bool, p_begin: int = 0,
                     p_end: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Plane-range partial (C, T) [V,H,W,4] for plane sharding."""
    _dev(packed)
    return _render_views_ct("render_packed_ct", packed, packed_hw(packed), homs, back, p_begin, p_end, out)


def render_packed_ct_rows(packed: torch.Tensor, homs: torch.Tensor, back: bool, y_begin: int, y_end: int,
                          out: torch.Tensor, p_begin: int = 0, p_end: int | None = None) -> torch.Tensor:
    """Rows [y_begin, y_end) of render_packed_ct's partial into out [V,H,W,4] (other rows
    untouched): one row band of a plane shard (mpiv_render_packed_ct_rows, same bits)."""
    dev = _dev(packed)
    P, H, W = packed_hw(packed)
    p_end = P if p_end is None else p_end
    V = homs.shape[0]
    h = _up(homs.reshape(V, P, 9), dev, "homs")
    _check_out(out, (V, H, W, 4), dev, "render_packed_ct_rows")
    _call("mpiv_render_packed_ct_rows", packed, H, W, P, p_begin, p_end, int(back), h, V, y_begin, y_end, out,
          _stream(dev))
    return out


def combine_ct(parts: torch.Tensor) -> torch.Tensor:
    """parts [G, ..., 4] ordered back->front -> [..., 3]."""
    dev = _dev(parts)
    parts = parts.contiguous()
    G = parts.shape[0]
    n = parts[0].numel() // 4
    out = torch.empty(tuple(parts.shape[1:-1]) + (3,), device=dev, dtype=torch.float32)
    _call("mpiv_combine_ct", parts, G, n, out, _stream(dev))
    return out


def render(rgba_layers: torch.Tensor, homs: torch.Tensor) -> torch.Tensor:
    """rgba_layers [B,H,W,P,4], homs [B,P,9] -> [B,H,W,3].

    A stride-0 (broadcast) batch is packed once into the plane-major layout and
    all B views render from it; otherwise the native-layout kernel reads the
    reference's tensor in place."""
    dev = _dev(rgba_layers)
    if rgba_layers.dim() != 5 or rgba_layers.shape[-1] != 4:
        raise RuntimeError(f"rgba_layers must be [B,H,W,P,4], got {tuple(rgba_layers.shape)}")
    B, H, W, P, _ = rgba_layers.shape
    if homs.shape[0] != B or homs.shape[1] != P:
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {homs.shape[0]}/{homs.shape[1]}")
    if B > 1 and rgba_layers.stride(0) == 0:
        return render_packed(pack_planes(rgba_layers[0]), homs)
    h = _up(homs, dev, "homs")
    out = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32)
    if RENDER_POLICY == "auto" and chunk_layout_ok(rgba_layers):
        # in place, whole 128-B pixel lines per tap instruction (render_chunk.hip): no pack
        _call("mpiv_render", rgba_layers, _strides(rgba_layers), B, H, W, P, h, out, _stream(dev))
        return out
    if RENDER_POLICY == "pack" or (RENDER_POLICY == "auto" and P >= 8 and (H + 4) * (W + 4) * 16 < 0x7FFFFF00):
        # per view: pack its MPI plane-major (one coalesced transpose pass) and render
        # from the packed copy -- the gathers of the in-place layout touch one 128-B
        # line per 16-B texel, which is slower than paying the pack
        packed = torch.empty(packed_shape(H, W, P), device=dev, dtype=torch.float32)
        for b in range(B):
            _call("mpiv_pack_planes", rgba_layers[b], _strides(rgba_layers[b]), H, W, P, packed, _stream(dev))
            _call("mpiv_render_packed", packed, H, W, P, h[b:b + 1], 1, out[b:b + 1], _stream(dev))
        return out
    _call("mpiv_render", rgba_layers, _strides(rgba_layers), B, H, W, P, h, out, _stream(dev))
    return out


def bwd_layout_ok(rgba_layers: torch.Tensor) -> bool:
    """True when mpiv_render_backward reads this [B,H,W,P,4] tensor in place (abi.hip:
    16-B texels with planes contiguous per pixel, row and pixel strides below 2^22 texels; a
    view of 2 GiB or more is read through 64-bit tap addresses, so its span is not limited).
    A float16 tensor: the same limits for mpiv_render_backward_f16, with 8-B aligned texels."""
    B, H, W, P, C = rgba_layers.shape
    st = rgba_layers.stride()
    if C != 4 or st[4] != 1 or st[3] != 4 or any(s % 4 for s in st[:3]) or st[1] < 0 or st[2] < 0:
        return False
    texel = 4 * rgba_layers.element_size()
    return rgba_layers.data_ptr() % texel == 0 and st[1] // 4 < (1 << 22) and st[2] // 4 < (1 << 22)


def _f16(t: torch.Tensor) -> bool:
    """A half MPI: the _f16 twins of the training entries (render_chunk.hip InF16) serve it."""
    return t.dtype == torch.float16


def _f16_in_place(t: torch.Tensor) -> torch.Tensor:
    """The half tensor itself where mpiv_render_*_f16 read it in place, else a contiguous HALF copy (never
    a float one); a densely laid out tensor whose data pointer is not 8-byte aligned is its own
    .contiguous(), so that one is cloned."""
    if bwd_layout_ok(t):
        return t
    c = t.contiguous()
    return c if c.data_ptr() % 8 == 0 else c.clone()


def train_layout_ok(rgba_layers: torch.Tensor) -> bool:
    """True when mpiv_render_train reads this [B,H,W,P,4] tensor in place and returns checkpoints:
    bwd_layout_ok's layout with H, W >= 2, the view's homographies in LDS beside the sample slots
    (P <= 796) and the backward's size ceiling (H*W < 2^26, P*H*W < 2^31)."""
    B, H, W, P, C = rgba_layers.shape
    return (bwd_layout_ok(rgba_layers) and H >= 2 and W >= 2 and 4 * 64 * 9 * 16 + P * 36 <= _CHUNK_LDS
            and H * W < (1 << 26) and P * H * W < (1 << 31))


def bwd_flag_offset(H: int, W: int, P: int) -> int:
    """Byte offset of the fallback flag in mpiv_render_backward's workspace (abi.hip
    bwd_layout): 1 after a call whose last view went through the bucket fallback."""
    return 2 * 64 * 8  # the two pair counters (64 slots of 8 B each) precede it (round 4 layout)


def render_train(rgba_layers: torch.Tensor, homs: torch.Tensor, broadcast_in_place: bool = False):
    """The forward for training: (frames [B,H,W,3], checkpoints [B,ceil(P/8),H,W,4]) from
    mpiv_render_train -- frames bit-identical to render() -- or (render(), None) when the
    layout is not read in place (a broadcast batch renders from one packed copy instead, unless
    broadcast_in_place: the camera gradient's backward wants the checkpoints of every view)."""
    dev = _dev(rgba_layers, f16_first=True)
    B, H, W, P, _ = rgba_layers.shape
    if homs.shape[0] != B or homs.shape[1] != P:
        raise RuntimeError(f"shape mismatch: MPI batch/planes {B}/{P} vs poses/planes {homs.shape[0]}/{homs.shape[1]}")
    if _f16(rgba_layers):
        # a half MPI (mpiv_render_train_f16, fp32 frames and checkpoints): there is no packed half route
        # with checkpoints, so a broadcast batch is read in place too, and any other layout through a
        # contiguous HALF copy -- never a float one.  Past the in-place limits the frame alone comes without
        # checkpoints: a degenerate frame (H or W < 2, which the packed f16 render does not take either)
        # from the float render on a widened copy of its one row or column, anything else (P > 796, the
        # backward's size ceiling) from the packed f16 render; the backward reads the half tensor in place.
        if H < 2 or W < 2:
            return render(rgba_layers.float(), homs), None
        if not (4 * 64 * 9 * 16 + P * 36 <= _CHUNK_LDS and H * W < (1 << 26) and P * H * W < (1 << 31)):
            return render_f16_views(rgba_layers, homs), None
        src = _f16_in_place(rgba_layers)
        h = _up(homs, dev, "homs")
        out = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32)
        ckpt = torch.empty((B, (P + 7) // 8, H, W, 4), device=dev, dtype=torch.float32)
        _call("mpiv_render_train_f16", src, _strides(src), B, H, W, P, h, out, ckpt, _stream(dev))
        return out, ckpt
    if (B > 1 and rgba_layers.stride(0) == 0 and not broadcast_in_place) or not train_layout_ok(rgba_layers):
        return render(rgba_layers, homs), None
    h = _up(homs, dev, "homs")
    out = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32)
    ckpt = torch.empty((B, (P + 7) // 8, H, W, 4), device=dev, dtype=torch.float32)
    _call("mpiv_render_train", rgba_layers, _strides(rgba_layers), B, H, W, P, h, out, ckpt, _stream(dev))
    return out, ckpt


def render_f16_views(rgba_layers_f16: torch.Tensor, homs: torch.Tensor) -> torch.Tensor:
    """Frames [B,H,W,3] of a half MPI [B,H,W,P,4] under homs [B,P,9] through the packed f16 render
    (render_texel.hip): utils.mpi_render_view_f16's inference body.  One MPI under many views (a stride-0
    batch) is packed once; a batch of MPIs view by view through one packed buffer."""
    B, H, W, P, _ = rgba_layers_f16.shape
    homs = homs.reshape(B, P, 9)
    if B > 1 and rgba_layers_f16.stride(0) == 0:  # one MPI, many views: pack once
        return render_packed_f16(pack_planes_f16(rgba_layers_f16[0]), homs, route_float=B >= F16_FLOAT_ONCE_MIN_VIEWS)
    out = torch.empty((B, H, W, 3), device=rgba_layers_f16.device, dtype=torch.float32)
    packed = None
    for b in range(B):
        packed = pack_planes_f16(rgba_layers_f16[b], out=packed)
        render_packed_f16(packed, homs[b:b + 1], out=out[b:b + 1], route_float=False)
    return out


# MPIV_BWD_MIN_WS=1: render_backward allocates the smallest workspace (plane groups: config 4
# 1.3 GB instead of 3.0, bit-identical gradients, a few percent slower)
BWD_MIN_WS = os.environ.get("MPIV_BWD_MIN_WS") == "1"

# MPIV_BWD_CHECK=1: every render_backward reads the fallback's abort count back (one stream
# synchronisation per call) and raises if a view's gradient was NaN-filled (render_bwd.hip)
BWD_CHECK = os.environ.get("MPIV_BWD_CHECK") == "1"


def render_backward_status(workspace: torch.Tensor, H: int, W: int, P: int) -> int:
    """Views of the last render_backward on this workspace whose bucket fallback aborted
    (their gradients are NaN); synchronises the current stream (mpiv_render_backward_status)."""
    n = _int(0)
    _call("mpiv_render_backward_status", workspace, H, W, P, ctypes.byref(n), _stream(workspace.device))
    return n.value


_BWD_WS: dict = {}


def _bwd_ws_sizes(L, H: int, W: int, P: int, cam: bool = False):
    """(minimum, fastest) workspace bytes of mpiv_render_backward (cam: mpiv_render_backward_cam) for one
    H x W x P view, memoised."""
    key = (L._name, H, W, P, _DEBUG_GEN, cam)  # (the sizes follow debug options such as bwd_group)
    v = _BWD_WS.get(key)
    if v is None:
        if cam:
            v = (L.mpiv_render_backward_cam_workspace_size_min(H, W, P),
                 L.mpiv_render_backward_cam_workspace_size(H, W, P))
        else:
            v = (L.mpiv_render_backward_workspace_size_min(H, W, P), L.mpiv_render_backward_workspace_size(H, W, P))
        _BWD_WS[key] = v
    return v


class _AbortMonitor:
    """The default (check=None) render_backward's abort report, surfaced without a synchronisation
    (ADVICE r4): the call runs mpiv_render_backward_watched, whose NaN fill of an aborted view also
    sets the device's page-locked, device-mapped abort flag (mpiv_render_backward_abort_flag) from the
    device; the next default render_backward (or render_backward_raise_pending) reads the flag on the
    host -- a memory read, no copy, event or synchronisation (round 5's stream-ordered copy and event
    cost ~30 us per call) -- and raises.  So an aborted fallback (never expected: render_bwd.hip) fails
    the training loop at the latest one step later instead of silently feeding NaN gradients to the
    optimiser."""

    def __init__(self, dev, L):
        self.dev = dev
        ptr = L.mpiv_render_backward_abort_flag(dev.index if dev.index is not None else torch.cuda.current_device())
        if not ptr:
            raise RuntimeError("mpiv_render_backward_abort_flag: no page-locked abort flag for " + str(dev))
        self.flag = ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int))

    def raise_completed(self, wait: bool = False):
        if wait:
            torch.cuda.synchronize(self.dev)
        if self.flag[0]:
            self.flag[0] = 0
            raise RuntimeError("mpiv_render_backward: the bucket fallback aborted on a view of an earlier backward "
                               "(its gradient was NaN)")


_ABORTS: dict = {}


def render_backward_raise_pending(dev=None) -> None:
    """Wait for every earlier default render_backward on `dev` (all devices if None) and raise if
    any of them NaN-filled a view (the check the next call would make)."""
    for (d, _), mon in list(_ABORTS.items()):
        if dev is None or d == torch.device(dev):
            mon.raise_completed(wait=True)


def render_backward(rgba_layers: torch.Tensor, homs: torch.Tensor, dout: torch.Tensor,
                    workspace: torch.Tensor | None = None, ckpt: torch.Tensor | None = None,
                    check: bool | None = None, want_dhoms: bool = False, want_dmpi: bool = True):
    """d(mpi_render_view_torch)/d(rgba_layers): rgba_layers [B,H,W,P,4] (read in place when
    its planes are contiguous per pixel, incl. a stride-0 broadcast batch; other layouts
    are made contiguous first), homs [B,P,9] (the forward's), dout [B,H,W,3] ->
    [B,H,W,P,4] contiguous, one gradient per view (a broadcast input's views are summed
    by autograd's expand backward, as in the reference).  Bit-exact to the reference's
    CPU autograd (render_bwd.hip).  A float16 rgba_layers (mpiv_render_backward*_f16) is read in place at
    8 B per texel and its gradient comes back in float16: RN_half of the float route's gradient on
    rgba_layers.float(), bit for bit, with no float copy of the MPI and no fp32 gradient (other layouts
    go through a contiguous HALF copy); dhoms are the float route's bits.
    ckpt: render_train()'s checkpoints of the same views
    (skips recomputing the forward composite).  check (default MPIV_BWD_CHECK): read the
    fallback's abort count back and raise if any view aborted (costs a synchronisation); left at
    None without MPIV_BWD_CHECK, the count is read back asynchronously and a later call raises
    (_AbortMonitor); False: not watched at all.
    want_dhoms: also return d(render)/d(homs) [B,P,9] on the device (render_bwd_cam.hip; per-sample
    terms bit-exact to the reference, the frame sum in a fixed order of its own): the result is then the
    pair (grad, dhoms).  want_dmpi=False (with want_dhoms): a fixed MPI -- grad is None and the gather /
    check / fallback half of the backward does not run.  workspace then needs
    mpiv_render_backward_cam_workspace_size_min bytes."""
    if not want_dmpi and not want_dhoms:
        raise RuntimeError("render_backward: nothing to compute (want_dmpi and want_dhoms are both False)")
    dev = _dev(rgba_layers, dout, f16_first=True)
    B, H, W, P, _ = rgba_layers.shape
    if tuple(dout.shape) != (B, H, W, 3):
        raise RuntimeError(f"grad_output must be [{B},{H},{W},3], got {tuple(dout.shape)}")
    src = _f16_in_place(rgba_layers) if _f16(rgba_layers) else (
        rgba_layers if bwd_layout_ok(rgba_layers) else rgba_layers.contiguous())
    L = load()
    # a caller's workspace of at least the minimum (plane groups, render_bwd.hip); our own: the
    # one-group size (the fastest schedule) unless MPIV_BWD_MIN_WS=1
    need, full = _bwd_ws_sizes(L, H, W, P, want_dhoms)
    ws = workspace if workspace is not None else torch.empty(need if BWD_MIN_WS else full, dtype=torch.uint8,
                                                             device=dev)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need or ws.device != dev:
        raise RuntimeError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on {dev}")
    sfx = "_f16" if _f16(rgba_layers) else ""
    grad = torch.empty((B, H, W, P, 4), device=dev, dtype=rgba_layers.dtype) if want_dmpi else None
    h = _up(homs.reshape(B, P, 9), dev, "homs")
    dout = dout.contiguous()
    if ckpt is not None and (tuple(ckpt.shape) != (B, (P + 7) // 8, H, W, 4) or not ckpt.is_contiguous()
                             or ckpt.device != dev or ckpt.dtype != torch.float32):
        raise RuntimeError(f"ckpt must be render_train()'s contiguous [{B},{(P + 7) // 8},{H},{W},4] tensor")
    watch = check is None and not BWD_CHECK
    if watch:
        # (one flag per device and library: the A/B build, when a test selects it, has its own)
        key = (dev, L._name)
        mon = _ABORTS.get(key)
        if mon is None:
            mon = _ABORTS.setdefault(key, _AbortMonitor(dev, L))
        mon.raise_completed()  # an earlier call's abort, read without waiting
    dhoms = None
    if want_dhoms:
        dhoms = torch.empty((B, P, 9), device=dev, dtype=torch.float32)
        _call("mpiv_render_backward_cam" + sfx, src, _strides(src), B, H, W, P, h, dout, ckpt, grad, dhoms, ws,
              ws.numel(), 1 if watch else 0, _stream(dev))
    else:
        _call(("mpiv_render_backward_watched" if watch else "mpiv_render_backward") + sfx, src, _strides(src), B, H, W,
              P, h, dout, ckpt, grad, ws, ws.numel(), _stream(dev))
    if BWD_CHECK if check is None else check:
        n = render_backward_status(ws, H, W, P)
        if n:
            raise RuntimeError(f"mpiv_render_backward: the bucket fallback aborted on {n} of {B} views "
                               "(their gradients are NaN)")
    return (grad, dhoms) if want_dhoms else grad


def _render_forward(ctx, rgba_layers, homs, in_place: bool):
    """The forward of RenderFunction / RenderF16Function.  in_place: read a stride-0 broadcast batch in place
    too, so that every view has its checkpoints."""
    ctx.homs = homs.detach()
    ctx.homs_shape = tuple(homs.shape)
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:  # keep the composite checkpoints for the backward
        out, ckpt = render_train(rgba_layers, ctx.homs, broadcast_in_place=in_place)
        ctx.save_for_backward(rgba_layers, ckpt)
        return out
    ctx.save_for_backward(rgba_layers, None)
    return render(rgba_layers, ctx.homs)


class RenderFunction(torch.autograd.Function):
    """Autograd node of the fused render: forward = render(), backward = render_backward() w.r.t.
    rgba_layers and, when the homographies require grad (a device tensor at the end of
    _host.render_homographies_autograd's chain from tgt_pose, planes and intrinsics), w.r.t. them.
    Float MPIs only: render_train() and render_backward() also serve half tensors, so the refusal of
    anything but fp32 (mpi_render_view_torch's, as in the reference) is made here."""

    @staticmethod
    def forward(ctx, rgba_layers, homs):
        _dev(rgba_layers)  # raises for a non-fp32 MPI
        # (a camera gradient reads a stride-0 broadcast MPI in place: every view has its checkpoints)
        return _render_forward(ctx, rgba_layers, homs, in_place=ctx.needs_input_grad[1])

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        rgba_layers, ckpt = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            grad, dhoms = render_backward(rgba_layers, ctx.homs, dout, ckpt=ckpt, want_dhoms=True,
                                          want_dmpi=ctx.needs_input_grad[0])
            return grad, dhoms.reshape(ctx.homs_shape)
        grad = render_backward(rgba_layers, ctx.homs, dout, ckpt=ckpt) if ctx.needs_input_grad[0] else None
        return grad, None


class RenderF16Function(RenderFunction):
    """RenderFunction for a half MPI (utils.mpi_render_view_f16 when something requires grad), the only
    node that admits one: the half tensor is read in place by render_train() (fp32 frame, bit-identical to
    the float route on rgba_layers.float()) and by the inherited backward, whose render_backward() returns a
    HALF gradient w.r.t. rgba_layers -- RN_half of the float route's, bit for bit -- and the float route's
    own bits w.r.t. the homographies.  No fp32 gradient exists at any point, and no float copy of the MPI
    except for a degenerate frame (H or W < 2: render_train widens its one row or column for the frame)."""

    @staticmethod
    def forward(ctx, rgba_layers, homs):
        if not _f16(rgba_layers):
            raise RuntimeError(f"expected scalar type Half but found {rgba_layers.dtype}")
        return _render_forward(ctx, rgba_layers, homs, in_place=True)


# ---------------------------------------------------------------------------
# MPI assembly from the network output (notebook mpi_from_net_output)
# ---------------------------------------------------------------------------

def _net_args(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int):
    dev = _dev(mpi_pred, fg)
    if mpi_pred.dim() != 4 or mpi_pred.shape[1] != 2 * P + 3:
        raise RuntimeError(f"mpi_pred must be [B, 2*{P}+3, H, W], got {tuple(mpi_pred.shape)}")
    B, _, H, W = mpi_pred.shape
    if tuple(fg.shape) != (B, H, W, 3):
        raise RuntimeError(f"ref_img must be [{B},{H},{W},3], got {tuple(fg.shape)}")
    return dev, B, H, W


def assemble_mpi(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int) -> torch.Tensor:
    """[B,2P+3,H,W] prediction + [B,H,W,3] reference image -> MPI [B,H,W,P,4]."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    out = torch.empty((B, H, W, P, 4), device=dev, dtype=torch.float32)
    _call("mpiv_assemble_mpi", mpi_pred, _strides(mpi_pred), fg, _strides(fg), B, H, W, P, out, _stream(dev))
    return out


def assemble_mpi_sampled(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int, homs: torch.Tensor) -> torch.Tensor:
    """assemble_mpi for the backward of a render with homs [B,P,9] only: texel rows no output pixel
    of that render can sample are left unwritten (mpiv_assemble_mpi_sampled)."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    h = _up(homs.reshape(B, P, 9), dev, "homs")
    out = torch.empty((B, H, W, P, 4), device=dev, dtype=torch.float32)
    _call("mpiv_assemble_mpi_sampled", mpi_pred, _strides(mpi_pred), fg, _strides(fg), B, H, W, P, h, out,
          _stream(dev))
    return out


def assemble_mpi_packed(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int, b: int,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """Batch element b of the assembled MPI, straight into the packed layout [P,H+4,W+4,4]."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    if not 0 <= b < B:
        raise IndexError(f"batch index {b} out of range for {B}")
    packed = torch.empty(packed_shape(H, W, P), device=dev, dtype=torch.float32) if out is None else \
        _check_out(out, packed_shape(H, W, P), dev, "assemble_mpi_packed")
    _call("mpiv_assemble_mpi_packed", mpi_pred, _strides(mpi_pred), fg, _strides(fg), b, H, W, P, packed,
          _stream(dev))
    return packed


def render_net_output(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int, homs: torch.Tensor) -> torch.Tensor:
    """Frames [B,H,W,3] of the MPIs assembled from [B,2P+3,H,W] + [B,H,W,3], view b from
    batch element b with homs [B,P,9], in one kernel (render_netout_kernel); bit-identical
    to render(assemble_mpi(...), homs)."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    h = _up(homs.reshape(B, P, 9), dev, "homs")
    out = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32)
    _call("mpiv_render_net_output", mpi_pred, _strides(mpi_pred), fg, _strides(fg), B, H, W, P, h, out,
          _stream(dev))
    return out


def netout_ckpt_ok(H: int, W: int, P: int) -> bool:
    """True when the fused training forward keeps composite checkpoints: exactly when
    render_train() would for the assembled (contiguous) MPI -- the backward reads it in place."""
    return H >= 2 and W >= 2 and 4 * 64 * 9 * 16 + P * 36 <= _CHUNK_LDS


def render_net_output_train(mpi_pred: torch.Tensor, fg: torch.Tensor, P: int, homs: torch.Tensor):
    """The fused net-output render's training forward: (frames [B,H,W,3], checkpoints
    [B,ceil(P/8),H,W,4]) -- the frames of render_net_output() and the checkpoints render_train()
    writes for the assembled MPI, bit for bit (mpiv_render_net_output_train); (frames, None) where
    render_train() keeps none."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    if not netout_ckpt_ok(H, W, P):
        return render_net_output(mpi_pred, fg, P, homs), None
    h = _up(homs.reshape(B, P, 9), dev, "homs")
    out = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32)
    ckpt = torch.empty((B, (P + 7) // 8, H, W, 4), device=dev, dtype=torch.float32)
    _call("mpiv_render_net_output_train", mpi_pred, _strides(mpi_pred), fg, _strides(fg), B, H, W, P, h, out, ckpt,
          _stream(dev))
    return out, ckpt


class NetOutputRenderFunction(torch.autograd.Function):
    """Autograd node of the fused assembly + render (the training losses' two lines, ipynb cell 12
    L7-11 / L38-42: mpi_from_net_output then mpi_render_view_torch) that never keeps the
    [B,H,W,P,4] MPI between forward and backward.  Forward: render_netout_kernel with the
    composite checkpoints (saves pred, ref image, checkpoints: (2P+3+3)*4 + ceil(P/8)*16 B per pixel
    instead of the MPI's P*16 + the checkpoints).  Backward: the MPI re-assembled (assemble.hip; the
    texel rows the render samples only, mpiv_assemble_mpi_sampled),
    render_backward with those checkpoints, the assembly adjoint -- the two-step chain's own
    kernels in its order, so d pred / d ref_img are bit-identical to it and to the reference's
    autograd (tests/golden/netout_train.npz).  Homographies that require grad (a device tensor, see
    RenderFunction) get theirs from the same chain (render_bwd_cam.hip)."""

    @staticmethod
    def forward(ctx, mpi_pred, fg, homs, P):
        ctx.P = P
        ctx.homs = homs.detach()
        ctx.homs_shape = tuple(homs.shape)
        out, ckpt = render_net_output_train(mpi_pred, fg, P, ctx.homs)
        ctx.save_for_backward(mpi_pred, fg, ckpt)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        mpi_pred, fg, ckpt = ctx.saved_tensors
        want_mpi = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_cam = ctx.needs_input_grad[2]
        if not (want_mpi or want_cam):
            return None, None, None, None
        # only the texel rows the render samples (round 6): the chain reads no other
        rgba = assemble_mpi_sampled(mpi_pred, fg, ctx.P, ctx.homs)
        dhoms = None
        if want_cam:
            drgba, dhoms = render_backward(rgba, ctx.homs, dout, ckpt=ckpt, want_dhoms=True, want_dmpi=want_mpi)
            dhoms = dhoms.reshape(ctx.homs_shape)
        else:
            drgba = render_backward(rgba, ctx.homs, dout, ckpt=ckpt)
        del rgba  # the re-assembled MPI lives only for the chain
        if not want_mpi:
            return None, None, dhoms, None
        res = assemble_mpi_backward(drgba, mpi_pred, fg, ctx.P, want_dfg=ctx.needs_input_grad[1])
        dpred, dfg = res if ctx.needs_input_grad[1] else (res, None)
        return (dpred if ctx.needs_input_grad[0] else None), dfg, dhoms, None


def assemble_mpi_backward(drgba: torch.Tensor, mpi_pred: torch.Tensor, fg: torch.Tensor, P: int,
                          want_dfg: bool = False):
    """d pred [B,2P+3,H,W] (and, with want_dfg, (d pred, d fg [B,H,W,3])) for d rgba."""
    dev, B, H, W = _net_args(mpi_pred, fg, P)
    _dev(drgba)
    if tuple(drgba.shape) != (B, H, W, P, 4):
        raise RuntimeError(f"grad must be [{B},{H},{W},{P},4], got {tuple(drgba.shape)}")
    dpred = torch.empty((B, 2 * P + 3, H, W), device=dev, dtype=torch.float32)
    dfg = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32) if want_dfg else None
    _call("mpiv_assemble_mpi_backward", drgba, _strides(drgba), mpi_pred, _strides(mpi_pred), fg, _strides(fg),
          B, H, W, P, dpred, dfg, _stream(dev))
    return (dpred, dfg) if want_dfg else dpred


class AssembleFunction(torch.autograd.Function):
    """Autograd node of the assembly: gradients w.r.t. the network prediction and, when
    it requires grad, the reference image (both bit-exact to the notebook's autograd)."""

    @staticmethod
    def forward(ctx, mpi_pred, fg, P):
        ctx.save_for_backward(mpi_pred, fg)
        ctx.P = P
        return assemble_mpi(mpi_pred, fg, P)

    @staticmethod
    @once_differentiable
    def backward(ctx, drgba):
        mpi_pred, fg = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        res = assemble_mpi_backward(drgba, mpi_pred, fg, ctx.P, want_dfg=ctx.needs_input_grad[1])
        dpred, dfg = res if ctx.needs_input_grad[1] else (res, None)
        return (dpred if ctx.needs_input_grad[0] else None), dfg, None


# ---------------------------------------------------------------------------
# plane sweep / inverse warp
# ---------------------------------------------------------------------------

_DEPTHS_DEV: dict = {}


def _depths_on(depth_planes, dev, sid=None) -> torch.Tensor:
    """The sweep depths as a contiguous fp32 tensor on `dev`.  The reference iterates
    `for depth in depth_planes` and adds each to an fp32 zero map (utils.py:466-467), so a
    list of floats and a tensor (the notebook passes torch.Tensor(inv_depths(...)).to(device),
    ipynb cell 8 L73) both mean their values rounded to fp32.  A device tensor is used where
    it is (no per-element reads back to the host); a list is uploaded once per distinct value
    list and device (memoised)."""
    if isinstance(depth_planes, torch.Tensor):
        return depth_planes.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    # keyed on the values (numbers hash and compare by value, so a list of Python or numpy
    # floats finds the same entry), the device and the stream: the copy is allocated on (and
    # its memory, once evicted, reused in the order of) the stream that made it, so each stream
    # reads only its own copy
    if sid is None:
        sid = torch.cuda.current_stream(dev).cuda_stream
    key = (tuple(depth_planes), dev.index, sid)
    if torch.cuda.is_current_stream_capturing():
        # HIP-graph capture: a host list cannot be uploaded inside the capture (a pageable copy), and the
        # memo's tensor must not be captured (the eviction frees it under the graph).  After a warm-up
        # with this list (on any stream) the depths are constants of the graph, written into a fresh
        # tensor of its own pool from the captured kernel arguments (_host.captured_constant).
        if not any(k[0] == key[0] and k[1] == key[1] for k in _DEPTHS_DEV):
            raise RuntimeError("mpi_vision_amd: a Python list of depths under a HIP-graph capture: run the call once "
                               "outside the capture first (the warm-up), or pass the depths as a device tensor "
                               "(a static input of the graph)")
        from ._host import captured_constant
        return captured_constant(torch.tensor([float(x) for x in key[0]], dtype=torch.float32), dev)
    d = _DEPTHS_DEV.get(key)
    if d is None:
        if len(_DEPTHS_DEV) >= 64:
            _DEPTHS_DEV.clear()
        d = torch.tensor([float(x) for x in key[0]], dtype=torch.float32).to(dev)
        _DEPTHS_DEV[key] = d
    return d


def _require_depths(depth_planes) -> None:
    # the reference concatenates one slice per depth (utils.py:466-470): no depths is
    # torch.cat.s ValueError, raised here before anything is launched
    if len(depth_planes) == 0:
        raise ValueError("torch.cat(): expected a non-empty list of Tensors")


def plane_sweep(img: torch.Tensor, depth_planes, ki: torch.Tensor, proj: torch.Tensor, tgt_h: int,
                tgt_w: int) -> torch.Tensor:
    """[B,Hs,Ws,C] -> PSV [B,tgt_h,tgt_w,D*C] in one launch (mpiv_plane_sweep): C <= 4 through
    the depth-per-lane LDS kernel reading the source in place (any strides, no padded
    copy), C > 4 through the generic strided kernel."""
    _require_depths(depth_planes)
    dev = _dev(img)
    B, Hs, Ws, C = img.shape
    dd = _depths_on(depth_planes, dev)
    D = dd.shape[0]
    out = torch.empty((B, tgt_h, tgt_w, D * C), device=dev, dtype=torch.float32)
    kid, projd = _up(ki, dev, "ki"), _up(proj, dev, "proj")
    _call("mpiv_plane_sweep", img, _strides(img), B, Hs, Ws, C, kid, projd, dd, D, tgt_h, tgt_w, out, _stream(dev))
    return out


_PROJ_SCRATCH: dict = {}
_STRIDES4: dict = {}


def plane_sweep_pose(img: torch.Tensor, depth_planes, ki: torch.Tensor, Ks: torch.Tensor, pose: torch.Tensor,
                     tgt_h: int, tgt_w: int, stream=None) -> torch.Tensor:
    """plane_sweep with proj = K4_src @ pose formed on the device in the same call
    (mpiv_plane_sweep_pose): img [B,Hs,Ws,C] or, unbatched, [Hs,Ws,C] (plane_sweep_torch_one's
    call: B = 1, the result still [1,...]); ki [B,9] on the device, Ks [3,3] (one camera) or
    [B,3,3] with 3x3 blocks contiguous, pose [B,4,4] (or [4,4]) contiguous fp32 on the device.
    The [B,16] proj lands in a scratch buffer kept per device and stream (reused in stream
    order; under a HIP-graph capture in a fresh tensor of the graph's pool).  The notebook's
    dataset calls this once per sample at 224x224x10, where the kernel is ~12 us, so the host
    path is kept to a handful of torch calls."""
    _require_depths(depth_planes)
    dev = _dev(img, Ks, pose)
    if img.dim() == 3:
        Hs, Ws, C = img.shape
        B = 1
        st = img.stride()
        st = (Hs * st[0], st[0], st[1], st[2])
    else:
        B, Hs, Ws, C = img.shape
        st = img.stride()
    cst = _STRIDES4.get(st)
    if cst is None:
        if len(_STRIDES4) >= 256:
            _STRIDES4.clear()
        cst = _STRIDES4[st] = (ctypes.c_int64 * 4)(*st)
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    sid = stream.cuda_stream
    dd = _depths_on(depth_planes, dev, sid)
    D = dd.shape[0]
    if torch.cuda.is_current_stream_capturing():
        # HIP-graph capture: proj goes to a fresh tensor of the graph's own pool (the memoised scratch is
        # replaced, and freed, by a later eager call with a larger batch; a replay would write into it)
        scratch = torch.empty(B * 16, device=dev, dtype=torch.float32)
    else:
        key = (dev.index, sid)
        scratch = _PROJ_SCRATCH.get(key)
        if scratch is None or scratch.numel() < B * 16:
            scratch = _PROJ_SCRATCH[key] = torch.empty(max(B, 8) * 16, device=dev, dtype=torch.float32)
    ks_b = 0 if Ks.dim() == 2 else Ks.stride(0)
    out = torch.empty((B, tgt_h, tgt_w, D * C), device=dev, dtype=torch.float32)
    _call("mpiv_plane_sweep_pose", img, cst, B, Hs, Ws, C, ki, Ks, ks_b, pose, scratch, dd, D, tgt_h, tgt_w,
          out, _vp(sid))
    return out


def plane_sweep_padded(img: torch.Tensor, depth_planes, ki: torch.Tensor, proj: torch.Tensor, tgt_h: int,
                       tgt_w: int) -> torch.Tensor:
    """plane_sweep through a padded 16-B texel copy of the source (mpiv_pad_texels +
    mpiv_plane_sweep_padded; C <= 4): the pixel-per-lane / tile / grouped kernels' input
    (A/B and tests)."""
    _require_depths(depth_planes)
    dev = _dev(img)
    B, Hs, Ws, C = img.shape
    dd = _depths_on(depth_planes, dev)
    D = dd.shape[0]
    out = torch.empty((B, tgt_h, tgt_w, D * C), device=dev, dtype=torch.float32)
    img4 = pad_texels(img)
    _call("mpiv_plane_sweep_padded", img4, B, Hs, Ws, C, _up(ki, dev, "ki"), _up(proj, dev, "proj"), dd, D,
          tgt_h, tgt_w, out, _stream(dev))
    return out


def pad_texels(img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[B,Hs,Ws,C<=4] (any strides) -> [B,Hs+4,Ws+4,4] 16-B texels with a 2-texel zero
    border (mpiv_pad_texels layout)."""
    dev = _dev(img)
    B, Hs, Ws, C = img.shape
    shape = (B, Hs + 4, Ws + 4, 4)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise RuntimeError(f"pad_texels: out must be a contiguous {shape} tensor")
    _call("mpiv_pad_texels", img, _strides(img), B, Hs, Ws, C, out, _stream(dev))
    return out


def preprocess(image: torch.Tensor) -> torch.Tensor:
    dev = _dev(image)
    src = image.contiguous()
    out = torch.empty_like(src)
    _call("mpiv_preprocess", src, src.numel(), out, _stream(dev))
    return out


def deprocess_u8(image: torch.Tensor) -> torch.Tensor:
    dev = _dev(image)
    src = image.contiguous()
    out = torch.empty(src.shape, device=dev, dtype=torch.uint8)
    _call("mpiv_deprocess_u8", src, src.numel(), out, _stream(dev))
    return out


def network_input(ref_image, psv_src_images, rel_poses, depth_planes, intrinsics) -> torch.Tensor:
    """format_network_input_torch: [B,H,W,3] ref + S PSVs of the 3-channel slices of
    psv_src_images, each swept directly into its channel range of one output."""
    from ._host import psv_matrices
    if len(rel_poses):
        _require_depths(depth_planes)
    dev = _dev(ref_image, psv_src_images)
    B, H, W, _ = ref_image.shape
    S = len(rel_poses)
    dd = _depths_on(depth_planes, dev) if S else None
    D = dd.shape[0] if S else len(depth_planes)
    Ctot = 3 + S * D * 3
    out = torch.empty((B, H, W, Ctot), device=dev, dtype=torch.float32)
    out[..., :3].copy_(ref_image)  # the concat's first slice is a plain copy (utils.py:491)
    for i, pose in enumerate(rel_poses):
        src = psv_src_images[:, :, :, i * 3:(i + 1) * 3]  # a strided channel slice, read in place
        ki, proj = psv_matrices(intrinsics, intrinsics, pose, pin=True)
        _call("mpiv_plane_sweep_into", src, _strides(src), B, H, W, 3, _up(ki, dev, "ki"), _up(proj, dev, "proj"),
              dd, D, H, W, out[..., 3 + i * D * 3:], H * W * Ctot, Ctot, _stream(dev))
    return out


def inverse_warp_depthmap(img, depth, ki, proj, tgt_h, tgt_w):
    dev = _dev(img, depth)
    B, Hs, Ws, C = img.shape
    if tuple(depth.shape) != (B, tgt_h, tgt_w):
        raise RuntimeError(f"depth must be [{B},{tgt_h},{tgt_w}], got {tuple(depth.shape)}")
    out = torch.empty((B, tgt_h, tgt_w, C), device=dev, dtype=torch.float32)
    _call("mpiv_inverse_warp", img, _strides(img), B, Hs, Ws, C, _up(ki, dev, "ki"), _up(proj, dev, "proj"),
          depth, _strides(depth), tgt_h, tgt_w, out, _stream(dev))
    return out


def inverse_warp_backward(img, depth, ki, proj, dout, want=(True, True, True, True), workspace=None):
    """The adjoint of inverse_warp_depthmap (mpiv_inverse_warp_backward, warp_bwd.hip): for dout
    [B,Ht,Wt,C] (read by its element strides: a stride-0 or permuted gradient is not copied) returns
    (dimg [B,Hs,Ws,C], ddepth [B,Ht,Wt], dki [B,9], dproj [B,16]) on the device, None where `want` says
    so.  dimg and ddepth are the reference's CPU autograd bits; dki and dproj are reproducible frame sums.
    One call on the current stream; the workspace (mpiv_inverse_warp_backward_workspace_size bytes) is
    the caller's or a torch.empty on the same stream."""
    dev = _dev(img, depth, dout)
    B, Hs, Ws, C = img.shape
    _, Ht, Wt = depth.shape
    if tuple(dout.shape) != (B, Ht, Wt, C):
        raise RuntimeError(f"grad_output must be [{B},{Ht},{Wt},{C}], got {tuple(dout.shape)}")
    if not any(want):
        raise RuntimeError("inverse_warp_backward: nothing to compute")
    need = load().mpiv_inverse_warp_backward_workspace_size(B, Hs, Ws, C, Ht, Wt)
    ws = workspace if workspace is not None else torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != dev:
        raise RuntimeError(f"workspace must be a contiguous uint8 tensor on {dev}")
    new = lambda on, *shape: torch.empty(shape, device=dev, dtype=torch.float32) if on else None  # noqa: E731
    dimg, ddepth, dki, dproj = new(want[0], B, Hs, Ws, C), new(want[1], B, Ht, Wt), new(want[2], B, 9), new(want[3], B, 16)
    _call("mpiv_inverse_warp_backward", img, _strides(img), B, Hs, Ws, C, _up(ki, dev, "ki"), _up(proj, dev, "proj"),
          depth, _strides(depth), Ht, Wt, dout, _strides(dout), ddepth, dimg, dki, dproj, ws, ws.numel(), _stream(dev))
    return dimg, ddepth, dki, dproj


class InverseWarpFunction(torch.autograd.Function):
    """Autograd node of the depth-map inverse warp: forward = inverse_warp_depthmap() (the same launch and
    the same bits as the no-grad call), backward = inverse_warp_backward() w.r.t. whichever of img, depth,
    ki [B,9] and proj [B,16] require grad (ki and proj then are device tensors at the end of
    _host.psv_matrices_autograd's chain from pose and intrinsics)."""

    @staticmethod
    def forward(ctx, img, depth, ki, proj, tgt_h, tgt_w):
        dev = _dev(img, depth)
        ki_d, proj_d = _up(ki.detach(), dev, "ki"), _up(proj.detach(), dev, "proj")
        ctx.save_for_backward(img, depth, ki_d, proj_d)
        ctx.mat_shapes = (tuple(ki.shape), tuple(proj.shape))
        return inverse_warp_depthmap(img, depth, ki_d, proj_d, tgt_h, tgt_w)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        img, depth, ki, proj = ctx.saved_tensors
        dimg, ddepth, dki, dproj = inverse_warp_backward(img, depth, ki, proj, dout, ctx.needs_input_grad[:4])
        if dki is not None:
            dki = dki.reshape(ctx.mat_shapes[0])
        if dproj is not None:
            dproj = dproj.reshape(ctx.mat_shapes[1])
        return dimg, ddepth, dki, dproj, None, None


def plane_sweep_backward(img, depths, ki, proj, dout, want=(True, True, True, True), workspace=None):
    """The adjoint of plane_sweep (mpiv_plane_sweep_backward, psv_bwd.hip): img [B,Hs,Ws,C] (any strides),
    depths a fp32 device tensor [D], dout [B,Ht,Wt,D*C] (read by its element strides: a channel slice of a
    wider gradient is not copied).  Returns (dimg [B,Hs,Ws,C], ddepths [D], dki [B,9], dproj [B,16]) on the
    device, None where `want` says so.  dimg is the reference's CPU autograd bits (the D per-depth
    gradients added in descending d); ddepths, dki and dproj are reproducible sums.  One call on the
    current stream; the workspace is the caller's (any size from
    mpiv_plane_sweep_backward_workspace_size_min up: the planes are taken in groups that fit, with the same
    bits) or a torch.empty of mpiv_plane_sweep_backward_workspace_size bytes on the same stream."""
    dev = _dev(img, depths, dout)
    B, Hs, Ws, C = img.shape
    D = depths.numel()
    if depths.dtype != torch.float32 or not depths.is_contiguous():
        raise RuntimeError("plane_sweep_backward: depths must be a contiguous fp32 tensor")
    if D == 0 or dout.dim() != 4 or dout.shape[0] != B or dout.shape[3] != D * C:
        raise RuntimeError(f"grad_output must be [{B},Ht,Wt,{D * C}], got {tuple(dout.shape)}")
    Ht, Wt = dout.shape[1], dout.shape[2]
    if not any(want):
        raise RuntimeError("plane_sweep_backward: nothing to compute")
    if workspace is None:
        need = load().mpiv_plane_sweep_backward_workspace_size(B, Hs, Ws, C, Ht, Wt, D)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    else:
        ws = workspace
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != dev:
        raise RuntimeError(f"workspace must be a contiguous uint8 tensor on {dev}")
    new = lambda on, *shape: torch.empty(shape, device=dev, dtype=torch.float32) if on else None  # noqa: E731
    dimg, ddepths, dki, dproj = new(want[0], B, Hs, Ws, C), new(want[1], D), new(want[2], B, 9), new(want[3], B, 16)
    _call("mpiv_plane_sweep_backward", img, _strides(img), B, Hs, Ws, C, _up(ki, dev, "ki"), _up(proj, dev, "proj"),
          depths, D, Ht, Wt, dout, _strides(dout), dimg, ddepths, dki, dproj, ws, ws.numel(), _stream(dev))
    return dimg, ddepths, dki, dproj


class PlaneSweepFunction(torch.autograd.Function):
    """Autograd node of the plane sweep: forward = plane_sweep()'s entry call (the same launch and the
    same bits as the no-grad call), backward = plane_sweep_backward() w.r.t. whichever of img, depths [D],
    ki [B,9] and proj [B,16] require grad (ki and proj then are device tensors at the end of
    _host.psv_matrices_autograd's chain from pose and intrinsics).  img is [B,Hs,Ws,C] with any strides;
    the depths enter as a tensor (a Python list has no gradient: the caller passes its device copy)."""

    @staticmethod
    def forward(ctx, img, depths, ki, proj, tgt_h, tgt_w):
        dev = _dev(img)
        dd = depths.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        ki_d, proj_d = _up(ki.detach(), dev, "ki"), _up(proj.detach(), dev, "proj")
        ctx.save_for_backward(img, dd, ki_d, proj_d)
        ctx.shapes = (tuple(depths.shape), tuple(ki.shape), tuple(proj.shape))
        ctx.depths_on = (depths.device, depths.dtype)
        B, Hs, Ws, C = img.shape
        D = dd.shape[0]
        out = torch.empty((B, tgt_h, tgt_w, D * C), device=dev, dtype=torch.float32)
        _call("mpiv_plane_sweep", img, _strides(img), B, Hs, Ws, C, ki_d, proj_d, dd, D, tgt_h, tgt_w, out, _stream(dev))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        img, dd, ki, proj = ctx.saved_tensors
        dimg, ddepths, dki, dproj = plane_sweep_backward(img, dd, ki, proj, dout, ctx.needs_input_grad[:4])
        if ddepths is not None:
            ddepths = ddepths.reshape(ctx.shapes[0]).to(device=ctx.depths_on[0], dtype=ctx.depths_on[1])
        if dki is not None:
            dki = dki.reshape(ctx.shapes[1])
        if dproj is not None:
            dproj = dproj.reshape(ctx.shapes[2])
        return dimg, ddepths, dki, dproj, None, None


class NetworkInputFunction(torch.autograd.Function):
    """Autograd node of format_network_input_torch's tensor: forward = network_input()'s calls (the
    reference image copied into the leading channels, each source's strided channel slice swept straight
    into its channel range: the same launches and bits), backward = the leading slice of dout for
    ref_image and, per source, plane_sweep_backward() of its slice of psv_src_images against its own
    channel slice of dout, both read in place by their strides.  mats = (ki_0, proj_0, ki_1, proj_1, ...),
    one pair per source ([B,9], [B,16]; device tensors at the end of the host chain when a camera requires
    grad).  A depths tensor that requires grad gets the sum of the sources' ddepths."""

    @staticmethod
    def forward(ctx, ref_image, psv_src_images, depths, *mats):
        dev = _dev(ref_image, psv_src_images)
        S = len(mats) // 2
        dd = depths.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        mats_d = [_up(m.detach(), dev, "ki" if i % 2 == 0 else "proj") for i, m in enumerate(mats)]
        ctx.save_for_backward(psv_src_images, dd, *mats_d)
        ctx.shapes = (tuple(depths.shape), [tuple(m.shape) for m in mats])
        ctx.depths_on = (depths.device, depths.dtype)
        B, H, W, _ = ref_image.shape
        D = dd.shape[0]
        Ctot = 3 + S * D * 3
        out = torch.empty((B, H, W, Ctot), device=dev, dtype=torch.float32)
        out[..., :3].copy_(ref_image)
        for i in range(S):
            src = psv_src_images[:, :, :, i * 3:(i + 1) * 3]
            _call("mpiv_plane_sweep_into", src, _strides(src), B, H, W, 3, mats_d[2 * i], mats_d[2 * i + 1], dd, D, H, W,
                  out[..., 3 + i * D * 3:], H * W * Ctot, Ctot, _stream(dev))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        psv_src_images, dd, *mats = ctx.saved_tensors
        S, D = len(mats) // 2, dd.shape[0]
        need = ctx.needs_input_grad
        dref = dout[..., :3] if need[0] else None
        want_d = need[2]
        dimgs, dmats, ddepths = [], [None] * (2 * S), None
        for i in reversed(range(S)):  # (autograd's order: the source swept last comes first)
            want = (need[1], want_d, need[3 + 2 * i], need[4 + 2 * i])
            if not any(want):
                continue
            src = psv_src_images[:, :, :, i * 3:(i + 1) * 3]
            dimg, dde, dki, dproj = plane_sweep_backward(src, dd, mats[2 * i], mats[2 * i + 1],
                                                         dout[..., 3 + i * D * 3:3 + (i + 1) * D * 3], want)
            dimgs.insert(0, dimg)
            if dde is not None:
                ddepths = dde if ddepths is None else ddepths + dde
            if dki is not None:
                dmats[2 * i] = dki.reshape(ctx.shapes[1][2 * i])
            if dproj is not None:
                dmats[2 * i + 1] = dproj.reshape(ctx.shapes[1][2 * i + 1])
        dsrc = torch.cat(dimgs, -1) if need[1] and S else None
        if need[1] and dsrc is not None and dsrc.shape[-1] != psv_src_images.shape[-1]:
            pad = torch.zeros(dsrc.shape[:-1] + (psv_src_images.shape[-1] - dsrc.shape[-1],), device=dsrc.device)
            dsrc = torch.cat([dsrc, pad], -1)  # (channels beyond the S sources are not read)
        if ddepths is not None:
            ddepths = ddepths.reshape(ctx.shapes[0]).to(device=ctx.depths_on[0], dtype=ctx.depths_on[1])
        return (dref, dsrc, ddepths, *dmats)


# ---------------------------------------------------------------------------
# sampler / compositor primitives
# ---------------------------------------------------------------------------

def _sample_args(imgs: torch.Tensor, coords: torch.Tensor, channels_last_out: bool):
    """(im4 [N,Hi,Wi,C], co4 [N,Ho,Wo,2], lead dims) of a sampler call."""
    if channels_last_out:
        if imgs.dim() != 4 or coords.dim() != 4:
            raise RuntimeError("resampler_wrapper_torch expects imgs [N,H,W,C] and coords [N,H,W,2]")
        lead = [imgs.shape[0]]
        im4 = imgs
        co4 = coords
    else:
        lead = list(imgs.shape[:-3])
        n = lead[0]  # IndexError for 3-d input, like the reference (utils.py:117)
        for s in lead[1:]:
            n *= s
        im4 = imgs.reshape([n] + list(imgs.shape[-3:]))
        co4 = coords.reshape([n] + list(coords.shape[-3:]))
    if co4.shape[0] != im4.shape[0] or co4.shape[-1] != 2:
        raise RuntimeError(f"grid_sample: coords {tuple(coords.shape)} do not match images {tuple(imgs.shape)}")
    return im4, co4, lead


def _bilinear_sample(imgs: torch.Tensor, coords: torch.Tensor, channels_last_out: bool) -> torch.Tensor:
    dev = _dev(imgs, coords)
    im4, co4, lead = _sample_args(imgs, coords, channels_last_out)
    N, Hi, Wi, C = im4.shape
    Ho, Wo = co4.shape[1], co4.shape[2]
    if channels_last_out:
        out = torch.empty((N, Ho, Wo, C), device=dev, dtype=torch.float32)
        ost = _strides(out, (0, 3, 1, 2))
    else:
        out = torch.empty((N, C, Ho, Wo), device=dev, dtype=torch.float32)
        ost = _strides(out)
    _call("mpiv_grid_sample", im4, _strides(im4, (0, 3, 1, 2)), N, C, Hi, Wi, co4, _strides(co4), Ho, Wo,
          out, ost, _stream(dev))
    if channels_last_out:
        return out
    return out.reshape(lead + [C, Ho, Wo])


def bilinear_sample(imgs: torch.Tensor, coords: torch.Tensor, channels_last_out: bool) -> torch.Tensor:
    """channels_last_out=False: bilinear_wrapper_torch semantics ([..., Hs, Ws, C] ->
    [..., C, Ht, Wt]); True: resampler_wrapper_torch ([N,H,W,C] -> [N,H',W',C]).  Differentiable w.r.t.
    imgs and coords (GridSampleFunction) when either requires grad; otherwise the plain launch."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (imgs, coords)):
        return GridSampleFunction.apply(imgs, coords, channels_last_out)
    return _bilinear_sample(imgs, coords, channels_last_out)


def grid_sample_backward(imgs, coords, dout, channels_last_out: bool, want=(True, True), workspace=None):
    """The adjoint of bilinear_sample (mpiv_grid_sample_backward, helper_bwd.hip): for dout in the
    forward's output shape (read by its element strides: a stride-0 or permuted gradient of 4-d inputs is
    not copied) returns (d imgs in imgs' shape, d coords in coords' shape), None where `want` says so;
    ATen's CPU grid_sampler_2d_backward bits.  One call on the current stream; the workspace
    (mpiv_grid_sample_backward_workspace_size bytes, for d imgs only) is the caller's or a torch.empty on
    the same stream."""
    dev = _dev(imgs, coords, dout)
    im4, co4, lead = _sample_args(imgs, coords, channels_last_out)
    N, Hi, Wi, C = im4.shape
    Ho, Wo = co4.shape[1], co4.shape[2]
    oshape = [N, Ho, Wo, C] if channels_last_out else lead + [C, Ho, Wo]
    if list(dout.shape) != oshape:
        raise RuntimeError(f"grad_output must be {oshape}, got {list(dout.shape)}")
    if not any(want):
        raise RuntimeError("grid_sample_backward: nothing to compute")
    if channels_last_out:
        dst = _strides(dout, (0, 3, 1, 2))
    else:
        dout = dout.reshape(N, C, Ho, Wo)
        dst = _strides(dout)
    ws = None
    if want[0]:
        need = load().mpiv_grid_sample_backward_workspace_size(N, C, Hi, Wi, Ho, Wo)
        ws = workspace if workspace is not None else torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != dev:
            raise RuntimeError(f"workspace must be a contiguous uint8 tensor on {dev}")
    din = torch.empty((N, Hi, Wi, C), device=dev, dtype=torch.float32) if want[0] else None
    dco = torch.empty((N, Ho, Wo, 2), device=dev, dtype=torch.float32) if want[1] else None
    _call("mpiv_grid_sample_backward", im4, _strides(im4, (0, 3, 1, 2)), N, C, Hi, Wi, co4, _strides(co4), Ho, Wo,
          dout, dst, din, dco, ws, ws.numel() if ws is not None else 0, _stream(dev))
    return (din.reshape(imgs.shape) if want[0] else None), (dco.reshape(coords.shape) if want[1] else None)


class GridSampleFunction(torch.autograd.Function):
    """Autograd node of the sampler: forward = the plain mpiv_grid_sample launch (the same bits as the
    no-grad call), backward = grid_sample_backward() w.r.t. whichever of imgs and coords require grad."""

    @staticmethod
    def forward(ctx, imgs, coords, channels_last_out):
        ctx.save_for_backward(imgs, coords)
        ctx.channels_last_out = channels_last_out
        return _bilinear_sample(imgs, coords, channels_last_out)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        imgs, coords = ctx.saved_tensors
        dimgs, dcoords = grid_sample_backward(imgs, coords, dout, ctx.channels_last_out, ctx.needs_input_grad[:2])
        return dimgs, dcoords, None


def _flat_pixels(t: torch.Tensor):
    """(pixel_stride, channel_stride) if the leading dims of t [..., 4] collapse to one
    uniform pixel stride, else None."""
    ps = t.stride(-2) if t.dim() >= 2 else 0
    expect = ps
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            return None
        expect *= t.shape[d]
    return ps, t.stride(-1)


def _over_layers(rgbas):
    """(layers, pixel stride, channel stride, n, shape) of an over_composite call: the layers as they
    are when one stride pair describes them all, else contiguous copies."""
    rgbas = list(rgbas)
    if not rgbas:
        raise UnboundLocalError("over_composite: empty list")  # the reference fails the same way
    _dev(*rgbas)
    shape = rgbas[0].shape
    if shape[-1] != 4:
        raise RuntimeError(f"over_composite expects RGBA layers, got {tuple(shape)}")
    layers = []
    for t in rgbas:
        if t.shape != shape:
            raise RuntimeError(f"over_composite: layer shapes differ {tuple(shape)} vs {tuple(t.shape)}")
        layers.append(t)
    # one (pixel stride, channel stride) pair must describe every layer; else copy
    if None in {_flat_pixels(t) for t in layers} or len({_flat_pixels(t) for t in layers}) != 1:
        layers = [t.contiguous() for t in layers]
    ps, cs = _flat_pixels(layers[0])
    return layers, ps, cs, layers[0].numel() // 4, shape


def _over_composite(rgbas) -> torch.Tensor:
    layers, ps, cs, n, shape = _over_layers(rgbas)
    dev = layers[0].device
    host_under_capture("over_composite's layer pointer table (built on the host per call)")
    ptrs = torch.tensor([t.data_ptr() for t in layers], dtype=torch.int64).to(dev)
    out = torch.empty(tuple(shape[:-1]) + (3,), device=dev, dtype=torch.float32)
    _call("mpiv_over_composite", ptrs, len(layers), n, ps, cs, out, _stream(dev))
    # temporaries (pointer table, contiguous copies) may be freed now: the caching
    # allocator only hands their memory to later work on this same stream
    return out


def over_composite(rgbas) -> torch.Tensor:
    """over_composite (utils.py:136-157).  Differentiable w.r.t. every layer (OverCompositeFunction)
    when one requires grad; otherwise the plain launch."""
    rgbas = list(rgbas)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in rgbas):
        return OverCompositeFunction.apply(*rgbas)
    return _over_composite(rgbas)


def over_composite_backward(rgbas, dout, workspace=None) -> torch.Tensor:
    """The adjoint of over_composite (mpiv_over_composite_backward, helper_bwd.hip): d layers as one
    [P, ..., 4] block, the reference's CPU autograd bits.  dout [..., 3] is read by its strides where its
    leading dims collapse to one pixel stride (stride 0 included), else copied.  One call on the current
    stream; the workspace (mpiv_over_composite_backward_workspace_size bytes) is the caller's or a
    torch.empty on the same stream."""
    layers, ps, cs, n, shape = _over_layers(rgbas)
    dev = _dev(dout, *layers)
    if tuple(dout.shape) != tuple(shape[:-1]) + (3,):
        raise RuntimeError(f"grad_output must be {tuple(shape[:-1]) + (3,)}, got {tuple(dout.shape)}")
    if _flat_pixels(dout) is None:
        dout = dout.contiguous()
    P = len(layers)
    need = load().mpiv_over_composite_backward_workspace_size(P, n)
    ws = workspace  # (P <= 9 needs none)
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    if ws is not None and (ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != dev):
        raise RuntimeError(f"workspace must be a contiguous uint8 tensor on {dev}")
    host_under_capture("over_composite's layer pointer table (built on the host per call)")
    ptrs = torch.tensor([t.data_ptr() for t in layers], dtype=torch.int64).to(dev)
    dlayers = torch.empty((P,) + tuple(shape), device=dev, dtype=torch.float32)
    dst = (ctypes.c_int64 * 2)(*_flat_pixels(dout))
    _call("mpiv_over_composite_backward", ptrs, P, n, ps, cs, dout, dst, dlayers, ws,
          ws.numel() if ws is not None else 0, _stream(dev))
    return dlayers


class OverCompositeFunction(torch.autograd.Function):
    """Autograd node of over_composite(*layers): forward = the plain mpiv_over_composite launch,
    backward = over_composite_backward(); the per-layer gradients are views of its one block (layers that
    are views of one tensor, or one tensor listed twice, accumulate through autograd as usual)."""

    @staticmethod
    def forward(ctx, *layers):
        ctx.save_for_backward(*layers)
        return _over_composite(layers)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dlayers = over_composite_backward(ctx.saved_tensors, dout)
        return tuple(dlayers[p] if need else None for p, need in enumerate(ctx.needs_input_grad))


# ---------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------

def aten_plain(contraction: int, rows: int, cols: int) -> bool:
    """How the reference's torch.matmul rounds a batched product on the CPU: ATen's bmm runs a naive loop
    (plain products summed in ascending k) below 400 multiply-adds per batch element and hands larger
    products to MKL sgemm (a chain of fused multiply-adds).  The kernels take the chain as an argument."""
    return contraction * rows * cols < 400


def transform_points(points: torch.Tensor, homography: torch.Tensor) -> torch.Tensor:
    dev = _dev(points, homography)
    hshape = list(homography.shape)
    M = 1
    for s in hshape[:-2]:
        M *= s
    pts = points.reshape(hshape[:-2] + [-1, 3]).contiguous()
    n = pts.shape[-2]
    out = torch.empty_like(pts)
    # [M,n,3] @ [M,3,3]^T; a homography without batch dimensions is `mm`: MKL at every n
    plain = len(hshape) > 2 and aten_plain(3, n, 3)
    _call("mpiv_transform_points_chain", pts, M, n, homography.reshape(M, 9).contiguous(), int(plain), out,
          _stream(dev))
    return out.reshape(points.shape)


def normalize_homogeneous(points: torch.Tensor) -> torch.Tensor:
    dev = _dev(points)
    k = points.shape[-1] - 1
    if k < 1:
        raise RuntimeError("normalize_homogeneous_torch needs at least 2 coordinates")
    work = points if points.is_contiguous() else points.contiguous()
    out = torch.empty(tuple(points.shape[:-1]) + (k,), device=dev, dtype=torch.float32)
    _call("mpiv_normalize_homogeneous", work, work.numel() // (k + 1), k, out, _stream(dev))
    if work is not points:  # keep the reference's in-place w update visible
        points.copy_(work)
    return out


def pixel2cam(depth, pixel_coords, intrinsics, is_homogeneous=True):
    dev = _dev(depth, pixel_coords)
    B, H, W = depth.shape
    n = H * W
    from ._host import _cpu32
    ki = torch.inverse(_cpu32(intrinsics)).reshape(B, 9)
    rows = 4 if is_homogeneous else 3
    cam = torch.empty((B, rows, H, W), device=dev, dtype=torch.float32)
    _call("mpiv_pixel2cam_chain", depth.contiguous(), pixel_coords.reshape(B, 3, n).contiguous(),
          _up(ki, dev, "inverse(intrinsics)"), B, n, int(bool(is_homogeneous)), int(aten_plain(3, 3, n)), cam,
          _stream(dev))  # [B,3,3] @ [B,3,n]
    return cam


def cam2pixel(cam_coords, proj):
    dev = _dev(cam_coords, proj)
    B, _, H, W = cam_coords.shape
    n = H * W
    out = torch.empty((B, H, W, 2), device=dev, dtype=torch.float32)
    _call("mpiv_cam2pixel_chain", cam_coords.reshape(B, 4, n).contiguous(), proj.reshape(B, 16).contiguous(), B,
          n, int(aten_plain(4, 4, n)), out, _stream(dev))  # [B,4,4] @ [B,4,n]
    return out


def warp_planes(imgs: torch.Tensor, pixel_coords_trg: torch.Tensor, hom: torch.Tensor) -> torch.Tensor:
    """transform_plane_imgs_torch: imgs [..., Hs, Ws, C], target points [..., Ht, Wt, 3],
    hom [..., 3, 3] -> [..., C, Ht, Wt]."""
    dev = _dev(imgs, pixel_coords_trg)
    hshape = list(hom.shape)
    M = 1
    for s in hshape[:-2]:
        M *= s
    Ht, Wt = pixel_coords_trg.shape[-3], pixel_coords_trg.shape[-2]
    pts = pixel_coords_trg.reshape(M, Ht * Wt, 3).contiguous()
    coords = torch.empty((M, Ht, Wt, 2), device=dev, dtype=torch.float32)
    plain = len(hshape) > 2 and aten_plain(3, Ht * Wt, 3)  # transform_points_torch's product
    _call("mpiv_plane_coords_chain", pts, M, Ht * Wt, _up(hom.reshape(M, 9), dev, "hom"), Ht, Wt, int(plain),
          coords, _stream(dev))
    return bilinear_sample(imgs, coords.reshape(list(pixel_coords_trg.shape[:-1]) + [2]), channels_last_out=False)
