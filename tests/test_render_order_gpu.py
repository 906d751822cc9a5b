"""The sampling kernels' tile order (render.hip xcd_tile_order, option render_order).

Which tile a block renders changes where the work runs, never what is computed: with the band order
(-1) and the interleaved order (1) every kernel that takes the order must write the same frames, bit
for bit, as the CPU oracle on the same [V,P,9] homographies -- every pixel of them, which output
buffers prefilled with NaN show (a tile rendered twice leaves another one unwritten) -- and its
counting build must count the same gathers.  Shapes (H x W): 6 x 4 tiles of 64 x 24, 28 tiles (no
multiple of 8), tiles_x = 8 (where the rotation of the tile rows matters) and fewer than 8 tiles, at
3 and at 40 views; the automatic choice also at 1 and at 64 (the measured threshold, abi.hip
kOrderMinViews: launches of 64 views and more take the interleaved order).

These tests do not show which order option 0 takes (both give the same bits); the per-XCD busy
counters of a profile do."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import assert_bits

pytestmark = pytest.mark.gpu

from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

P = 4
SHAPES = [(136, 200), (160, 200), (100, 512), (40, 70)]
SHAPE_IDS = ["136x200", "160x200", "100x512", "40x70"]
# the four above are stretched and small, which the automatic routes send to the one-row kernel (float)
# and to two plain rows (u8); a near-square frame takes the rows kernels with vertical tap reuse
MORE = SHAPES + [(150, 160)]
MORE_IDS = SHAPE_IDS + ["150x160"]
VIEWS = [3, 40]
# render_vshare -> (R, rows in flight): the shipped flavours
VSHARE = {3: (8, 4), 4: (6, 3), 5: (9, 3), 11: (4, 4)}
NAN = float("nan")


def _poses(n):
    out = []
    for k in range(n):
        a = 2.0 * math.pi * (100 + 37 * k) / 1000
        t = (0.05 * math.sin(a), 0.02 * math.cos(a), 0.03 * math.sin(math.pi * k / n))
        out.append(configs.pose_from(configs.rot_y(1.0 * math.sin(a)), t))
    return out


@functools.lru_cache(maxsize=None)
def _homs(hw, V):
    H, W = hw
    f = configs.focal_from_fov(W)
    K = configs.f32([configs.intrinsics_matrix(f, f, W / 2.0, H / 2.0)] * V)
    return _host.render_homographies(configs.f32(_poses(V)), configs.f32(configs.inv_depths(1, 100, P)), K, V)


@functools.lru_cache(maxsize=None)
def _mpi(hw):
    return configs.synthetic_mpi(1, hw[0], hw[1], P, 2000 + hw[0])


@functools.lru_cache(maxsize=None)
def _packed(hw):
    return _lib.pack_planes(_mpi(hw)[0].to("cuda:0"))


def _full(hw, V):
    return np.broadcast_to(_mpi(hw).numpy(), (V,) + hw + (P, 4))


@functools.lru_cache(maxsize=None)
def _want(hw, V):
    return oracle.render(_full(hw, V), _homs(hw, V).numpy())


def _render(hw, V):
    out = torch.full((V,) + hw + (3,), NAN, device="cuda:0")
    return _lib.render_packed(_packed(hw), _homs(hw, V), out=out).cpu().numpy()


def _census(hw, V):
    dev = torch.device("cuda:0")
    out = torch.full((V,) + hw + (3,), NAN, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib._call("mpiv_render_packed_census", _packed(hw), hw[0], hw[1], P, _homs(hw, V).reshape(V, P, 9).to(dev), V,
               out, n, _lib._stream(dev))
    return out.cpu().numpy(), int(n.item())


@pytest.mark.parametrize("vshare", sorted(VSHARE), ids=[f"r{r}d{d}" for _, (r, d) in sorted(VSHARE.items())])
@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("hw", SHAPES, ids=SHAPE_IDS)
def test_rows_kernel_every_flavour(hw, V, vshare, dev, kopts):
    """render_rows_kernel at every shipped (R, D): both orders equal the oracle and each other, and the
    counting build gives the same frames and the same gather count."""
    want = _want(hw, V)
    counts = {}
    for order in (-1, 1):
        kopts(render_order=order, render_vshare=vshare)
        assert_bits(_render(hw, V), want, f"render_order={order}")
        frames, counts[order] = _census(hw, V)
        assert_bits(frames, want, f"census build, render_order={order}")
    print(f"gather instructions: {counts}")
    assert counts[-1] == counts[1] > 0


@pytest.mark.parametrize("same", [1, 2], ids=["same", "oob"])
@pytest.mark.parametrize("V", VIEWS)
def test_rows_kernel_same_row_flavours(V, same, dev, kopts):
    """The same-row tap reuse flavours of (6, 3), with and without OOB, on the 28-tile shape."""
    hw = SHAPES[1]
    want = _want(hw, V)
    counts = {}
    for order in (-1, 1):
        kopts(render_order=order, render_vshare=4, render_same=same)
        assert_bits(_render(hw, V), want, f"render_order={order}")
        frames, counts[order] = _census(hw, V)
        assert_bits(frames, want, f"census build, render_order={order}")
    assert counts[-1] == counts[1] > 0


@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("hw", MORE, ids=MORE_IDS)
def test_plane_range_partial_and_row_band(hw, V, dev, kopts):
    """The (C, T) flavour: the partial of planes [1, P) equals the oracle's under both orders, and a row
    band that starts off a tile boundary and ends inside a tile (its tiles counted inside the band)
    equals the same rows of it and leaves the other rows alone."""
    H, W = hw
    homs = _homs(hw, V)
    want = oracle.render_ct(_full(hw, V), homs.numpy(), 1, P, back=False)
    y_lo, y_hi = 5, H - 7
    for order in (-1, 1):
        kopts(render_order=order)
        ct = torch.full((V, H, W, 4), NAN, device=dev)
        _lib.render_packed_ct(_packed(hw), homs, False, 1, P, out=ct)
        assert_bits(ct, want, f"ct [1,{P}), render_order={order}")
        band = torch.full((V, H, W, 4), NAN, device=dev)
        _lib.render_packed_ct_rows(_packed(hw), homs, False, y_lo, y_hi, band, 1, P)
        assert_bits(band[:, y_lo:y_hi], want[:, y_lo:y_hi], f"rows [{y_lo},{y_hi}), render_order={order}")
        assert torch.isnan(band[:, :y_lo]).all() and torch.isnan(band[:, y_hi:]).all(), order


@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("hw", SHAPES, ids=SHAPE_IDS)
def test_one_row_kernel(hw, V, dev, kopts):
    """render_packed_kernel (render_tile=-1: one row per work-item, 64 x 4 tiles)."""
    want = _want(hw, V)
    for order in (-1, 1):
        kopts(render_order=order, render_tile=-1)
        assert_bits(_render(hw, V), want, f"render_order={order}")


@pytest.mark.parametrize("flight", [0, 2])
@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("hw", MORE, ids=MORE_IDS)
def test_u8_kernel(hw, V, flight, dev, kopts):
    """render_u8_kernel: both orders equal the oracle's render of u8 / 255 (150 x 160, 3 x 10 tiles of
    64 x 16: the flavour with vertical tap reuse, 4 and 2 rows in flight; the others two plain rows)."""
    H, W = hw
    g = torch.Generator().manual_seed(3 + H)
    u8 = torch.randint(0, 256, (H, W, P, 4), generator=g, dtype=torch.uint8)
    u8[:, :, 0, 3] = 255
    pk = _lib.pack_planes_u8(u8.to(dev))
    fl = (u8.numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)
    homs = _homs(hw, V)
    want = oracle.render(np.broadcast_to(fl[None], (V,) + fl.shape), homs.numpy())
    for order in (-1, 1):
        kopts(render_order=order, u8_flight=flight)
        out = torch.full((V, H, W, 3), NAN, device=dev)
        _lib.render_packed_u8(pk, homs, out=out, route_float=False)
        assert_bits(out, want, f"render_order={order}")


@pytest.mark.parametrize("V", [1, 40, 64])
@pytest.mark.parametrize("hw", MORE, ids=MORE_IDS)
def test_automatic_order(hw, V, dev, kopts):
    """Option 0 (64 views: the interleaved order; 40 views and one view: the band order) against both
    forced runs."""
    got = {}
    for order in (0, -1, 1):
        kopts(render_order=order)
        got[order] = _render(hw, V)
    assert_bits(got[0], _want(hw, V), "render_order=0")
    assert_bits(got[0], got[1 if V >= 64 else -1], "automatic vs the order it takes")
    assert_bits(got[0], got[-1 if V >= 64 else 1], "automatic vs the other order")
