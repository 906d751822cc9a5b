"""Training through MPI views of 2 GiB and more (no device needed): the ABI's gating and dry-run
routes, the chunk_wide test hook and the Python layout tests.

A view whose taps reach the buffer unit's out-of-range offset (0x7FFFFF00 bytes) is read through the
wide instantiations of the in-place readers (64-bit tap addresses); narrower views keep the kernels
they had, whose names are pinned here as the parent build printed them."""
import pytest
import torch

from mpi_vision_amd import _lib

WIDE = (1, 1024, 1024, 136)     # 2.28 GB per view: one 8-plane chunk more than config 4
CONFIG4 = (1, 1024, 1024, 128)  # 1.6 KB below the buffer range
SMALL = (1, 40, 24, 11)


def test_abi_version_is_17():
    assert _lib.ABI_VERSION == 17
    assert _lib.load_main().mpiv_abi_version() == 17


def test_render_train_routes():
    assert _lib.route("render_train", *WIDE)[0] == "render_chunk_strip_kernel<16, 2, true>"
    # the narrow instantiation, as before (tests/test_bench.py pins the config-4 name too)
    assert _lib.route("render_train", *CONFIG4) == ("render_chunk_strip_kernel<16, 2>", 32 * 64 * 256)
    assert _lib.route("render_train", *SMALL)[0] == "render_chunk_strip_kernel<16, 2>"


def test_render_backward_routes():
    assert _lib.route("render_backward", *WIDE) == ("bwd_chain_strip_kernel<8, true>", 32 * 128 * 256)
    assert _lib.route("render_backward", *CONFIG4) == ("bwd_chain_strip_kernel<8>", 32 * 128 * 256)
    assert _lib.route("render_backward", *SMALL)[0] == "bwd_chain_strip_kernel<8>"
    # a degenerate frame takes the generic recipe's chain
    assert _lib.route("render_backward", 1, 1, 40, 3)[0] == "bwd_chain_kernel<0, false, 1>"


def test_inference_route_of_a_wide_view_is_unchanged():
    assert _lib.route("render", *WIDE)[0] == "render_native_kernel<true, true>"


@pytest.mark.parametrize("entry", ["render_train", "render_backward"])
@pytest.mark.parametrize("shape", [(1, 2048, 2048, 512), (1, 8192, 8192, 8)], ids=["PHW=2^31", "HW=2^26"])
def test_the_ceiling_is_the_id_limit(entry, shape):
    with pytest.raises(RuntimeError, match=r"one view is limited to H\*W < 2\^26 and P\*H\*W < 2\^31"):
        _lib.route(entry, *shape)


def test_just_below_the_ceiling_routes_wide():
    # P*H*W = 2^31 - 2^22 plane-pixels, 32 GiB minus 64 MiB per view
    shape = (1, 2048, 2048, 511)
    assert _lib.route("render_train", *shape)[0] == "render_chunk_strip_kernel<16, 2, true>"
    assert _lib.route("render_backward", *shape)[0] == "bwd_chain_strip_kernel<8, true>"


def test_workspace_sizes_up_to_the_ceiling():
    """The sizes are 64-bit throughout: at least the d samples (16 B per plane-pixel of the resident
    planes) plus the checkpoints (16 B per pixel and chunk), and monotonic in P."""
    L = _lib.load_main()
    H = W = 2048
    prev = 0
    for P in (136, 256, 511):
        full = L.mpiv_render_backward_workspace_size(H, W, P)
        small = L.mpiv_render_backward_workspace_size_min(H, W, P)
        ck = (P + 7) // 8 * H * W * 16
        assert full >= P * H * W * 16 + ck
        assert ck + (1 << 25) * 16 // 2 < small < full
        assert full > prev
        prev = full


def test_chunk_wide_is_a_production_test_hook():
    L = _lib.load_main()
    try:
        assert L.mpiv_debug_set(b"chunk_wide", 1) == 0
        # (the dry run reports production routes only)
        with pytest.raises(RuntimeError, match="production routes only"):
            _lib.route("render_train", *SMALL)
        assert L.mpiv_debug_set(b"reset", 0) == 0
        assert _lib.route("render_train", *SMALL)[0] == "render_chunk_strip_kernel<16, 2>"
        with _lib.debug(chunk_wide=1):
            assert _lib.load() is L  # no A/B library needed
    finally:
        L.mpiv_debug_set(b"reset", 0)


ROW = 15_000_000  # floats between image rows: rows 36..47 of a 48-row view lie beyond 2^31 bytes


def _flat():
    """A 2.9 GB flat allocation that exists as metadata only: the layout tests read shapes and strides."""
    return torch.empty(48 * ROW, dtype=torch.float32, device="meta")


def test_layout_tests_accept_a_wide_strided_view():
    flat = _flat()
    view = flat.as_strided((1, 48, 24, 11, 4), (0, ROW, 44, 4, 1))
    assert 47 * ROW * 4 > 1 << 31
    assert _lib.bwd_layout_ok(view)
    assert _lib.train_layout_ok(view)
    assert not _lib.chunk_layout_ok(view)  # render()'s inference policy keeps its meaning


def test_layout_tests_keep_their_other_limits():
    flat = torch.empty(48 * (4 << 22), dtype=torch.float32, device="meta")
    ok = flat.as_strided((1, 48, 24, 11, 4), (0, ROW, 44, 4, 1))
    assert _lib.bwd_layout_ok(ok)
    assert not _lib.bwd_layout_ok(flat.as_strided((1, 48, 24, 11, 4), (0, 4 << 22, 44, 4, 1)))  # row stride 2^22 texels
    assert not _lib.bwd_layout_ok(flat.as_strided((1, 48, 24, 11, 4), (0, ROW + 2, 44, 4, 1)))  # unaligned rows
    assert not _lib.bwd_layout_ok(flat.as_strided((1, 48, 24, 11, 4), (0, ROW, 48, 1, 12)))     # planar
    assert not _lib.train_layout_ok(flat.as_strided((1, 48, 24, 800, 4), (0, ROW, 3200, 4, 1)))  # P > 796
    assert not _lib.train_layout_ok(flat.as_strided((1, 1, 24, 11, 4), (0, ROW, 44, 4, 1)))      # H < 2
