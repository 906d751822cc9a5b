"""Crafted inputs shared by tools/gen_goldens_lattice.py, tests/test_lattice.py (CPU) and
tests/test_lattice_gpu.py: homographies whose sample positions are exactly representable (texel
centres and edges, the values at which the kernels' clamps, dead-tile tests and tap-reuse predicates
switch), huge / non-finite / w == 0 homographies, and texel sets that hold Inf and NaN.

A plain module: no fixtures, nothing collected by pytest.

Shapes.  The reference's swapped normalisation gives px = u * W / (H-1) - 0.5 and
py = v * H / (W-1) - 0.5 (utils.py:186-188).  With W = H-1 a power of two px = u - 0.5 exactly ("x
exact"); with H = W-1 a power of two py = v - 0.5 exactly ("y exact").  The families below are written
for the x-exact shapes and mirrored (the roles of x and y swapped) for the y-exact ones."""
from __future__ import annotations

import hashlib

import numpy as np
import torch

X_SMALL, Y_SMALL = (65, 64), (64, 65)      # one tile column / a partial wave
X_TWO, Y_TWO = (129, 128), (128, 129)      # two 64-wide tile columns / the same in y
RENDER_SHAPES = [X_SMALL, Y_SMALL, X_TWO, Y_TWO]
# Output columns / rows at which tiles start.  Every kernel's tiles are 64 columns wide.  The tile heights
# are 4 (one row per work-item), 16, 24, 32 and 36 (the rows kernels' 4R with R = 4, 6, 8, 9; the u8
# kernel's 16): 72 starts a tile of 4, 24 and 36 rows, 64 one of 4, 16 and 32.
EDGE_COLS = (64,)
EDGE_ROWS = (72, 64)
QNAN = np.uint32(0x7FC00000)


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------

def _np32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32)


def match(got, want, what=""):
    """Equal shapes, equal NaN positions, identical bits at every non-NaN position (signed zeros
    count; a NaN's payload is not part of the contract).  Short failure message."""
    got, want = _np32(got), _np32(want)
    if got.shape != want.shape:
        raise AssertionError(f"{what}: shape {got.shape} != {want.shape}")
    ng, nw = np.isnan(got), np.isnan(want)
    if not np.array_equal(ng, nw):
        d = ng != nw
        i = tuple(int(k) for k in np.argwhere(d)[0])
        raise AssertionError(f"{what}: NaN positions differ at {int(d.sum())}/{d.size} values, first at {i} "
                             f"(got {got[i]}, want {want[i]})")
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~ng
    if diff.any():
        i = tuple(int(k) for k in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())}/{diff.size} values differ, first at {i} "
                             f"(got {got[i]!r}, want {want[i]!r})")


def canon_sha(a) -> str:
    """sha256 of the float32 bits with every NaN replaced by one quiet NaN."""
    a = _np32(a)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = QNAN
    return hashlib.sha256(bits.tobytes()).hexdigest()


def sample_idx(n: int, count: int = 1024) -> np.ndarray:
    return np.random.default_rng(n).integers(0, n, size=min(count, n)).astype(np.int64)


def nan_share(a) -> float:
    return float(np.isnan(_np32(a)).mean())


# ---------------------------------------------------------------------------
# homography families
# ---------------------------------------------------------------------------

def T(sx, tx, sy, ty, h6=0.0, h7=0.0, h8=1.0):
    return [sx, 0.0, tx, 0.0, sy, ty, h6, h7, h8]


def mirror(h):
    """The same map with the roles of x and y swapped."""
    return [h[4], h[3], h[5], h[1], h[0], h[2], h[7], h[6], h[8]]


def x_exact(shape) -> bool:
    H, W = shape
    return W == H - 1


def exact_extent(shape) -> int:
    """The image extent along the exact axis (W for the x-exact shapes, H for the y-exact ones)."""
    return shape[1] if x_exact(shape) else shape[0]


LATTICE = ["int_shift", "half_shift", "scale", "rot90"]
FAMILIES = LATTICE + ["huge", "w_zero"]


def edge_starts(shape):
    return EDGE_COLS if x_exact(shape) else EDGE_ROWS


def edge_shifts(shape):
    """Shifts t of u = x + t (x exact: px = x + t - 0.5), eight per tile start b of edge_starts(shape):
    they put the first pixel of the tile column (row) starting at b at exactly N-1, N, N+0.5, N+1, and
    the last pixel of the one before it at exactly -1, -2, -2.5, -3."""
    n = exact_extent(shape)
    out = []
    for b in edge_starts(shape):
        out += [v - b + 0.5 for v in (n - 1, n, n + 0.5, n + 1)]
        out += [v - (b - 1) + 0.5 for v in (-1, -2, -2.5, -3)]
    return out


EDGE_THRESHOLDS = ["N-1", "N", "N+0.5", "N+1", "-1", "-2", "-2.5", "-3"]


def family(name: str, shape) -> np.ndarray:
    """[P, 9] float32 planes of one family for a render shape (H, W)."""
    H, W = shape
    n = exact_extent(shape)
    other = H if x_exact(shape) else W
    if name == "int_shift":
        hs = [T(1, .5, 1, .5), T(1, 1.5, 1, 3.5), T(1, -.5, 1, -1.5), T(1, -2.5, 1, 70)]
    elif name == "half_shift":
        hs = [T(1, 0, 1, 0), T(1, 1, 1, 1), T(1, -1, 1, -1), T(1, n - 1, 1, n)]
    elif name == "scale":
        hs = [T(2, .5, 2, .5), T(.5, .5, .5, .5), T(4, .5 - n + 1, 1, 0), T(.25, .5, .25, 16)]
    elif name == "rot90":
        # u = y + .5 and its inverse turn u = other - .5 - y: exact, and not column separable
        a = [0, 1, .5, -1, 0, other - .5, 0, 0, 1]
        b = [0, -1, other - .5, 1, 0, .5, 0, 0, 1]
        hs = [a, b, a, b]
    elif name == "edge":
        hs = [T(1, t, 1, 0) for t in edge_shifts(shape)]
    elif name == "huge":
        hs = [T(1, 1e9, 1, 0), T(1, -1e20, 1, 0), T(1, .5, 1, 3e38), T(1e30, .5, 1e30, 0)]
    elif name == "w_zero":
        hs = [T(1, .5, 1, 0, 1, 0, -10), T(1, .5, 1, 0, 0, 1, -20), [0.0] * 9, T(1, .5, 1, 0, 1e-30, 0, 1e-38)]
    else:
        raise KeyError(name)
    if not x_exact(shape):
        hs = [mirror(h) for h in hs]
    return np.asarray(hs, np.float64).astype(np.float32)


# `edge` views in this order of thresholds (per tile start): the dead ones and their live neighbours first
EDGE_ORDER = [3, 2, 6, 5, 0, 1, 4, 7]


def views(name: str, shape, V: int, P: int) -> np.ndarray:
    """[V, P, 9]: the family's planes cycled across planes and views (view v starts at plane v).
    `edge`: every plane of view v is the same threshold plane (a tile is dead only when it is for all
    the planes of the range), the thresholds in EDGE_ORDER, the second tile start after the first."""
    f = family(name, shape)
    if name == "edge":
        order = [8 * b + k for b in range(len(f) // 8) for k in EDGE_ORDER]
        return np.stack([np.stack([f[order[v % len(order)]]] * P) for v in range(V)])
    return np.stack([np.stack([f[(v + p) % len(f)] for p in range(P)]) for v in range(V)])


def nonfinite_views(shape, P: int) -> np.ndarray:
    """[6, P, 9]: finite int_shift / half_shift views with three views between them that hold one
    plane with Inf in h2, NaN in h5 and NaN in h0 (mirrored with the family for the y-exact shapes:
    the entries named are those of the x-exact form)."""
    a, b = views("int_shift", shape, 6, P), views("half_shift", shape, 6, P)
    out = np.stack([a[0], b[1], a[2], b[3], a[4], b[5]])
    x = x_exact(shape)
    out[1, 1 % P, 2 if x else 5] = np.inf
    out[3, 2 % P, 5 if x else 2] = np.nan
    out[4, 0, 0 if x else 4] = np.nan
    return out


NONFINITE_BAD_VIEWS = (1, 3, 4)


# ---------------------------------------------------------------------------
# texel sets
# ---------------------------------------------------------------------------

def finite_mpi(H: int, W: int, P: int, seed: int = 0) -> torch.Tensor:
    """[H, W, P, 4]: rgb in [-1, 1), alpha in [0, 1)."""
    g = torch.Generator().manual_seed(7000 + 131 * H + 17 * W + P + seed)
    m = torch.rand((H, W, P, 4), generator=g)
    m[..., :3] = m[..., :3] * 2 - 1
    return m


def poison(m: torch.Tensor) -> torch.Tensor:
    """The non-finite pattern on [H, W, P, C >= 3] texels: +Inf in channel 0 of image column 0 (plane 0),
    -Inf in channel 1 of column W-1 (plane 1), NaN in channel 2 of row 0 (plane 2), one Inf alpha on row
    H-1 and one all-NaN interior texel (the last plane); planes taken modulo P."""
    m = m.clone()
    H, W, P, C = m.shape
    m[:, 0, 0, 0] = float("inf")
    m[:, W - 1, 1 % P, 1] = float("-inf")
    m[0, :, 2 % P, 2] = float("nan")
    m[H - 1, W // 3, P - 1, C - 1] = float("inf")
    m[H // 2, W // 2, P - 1, :] = float("nan")
    return m


def nonfinite_mpi(H: int, W: int, P: int, seed: int = 0) -> torch.Tensor:
    return poison(finite_mpi(H, W, P, seed))


def texels(kind: str, H: int, W: int, P: int) -> torch.Tensor:
    return finite_mpi(H, W, P) if kind == "finite" else nonfinite_mpi(H, W, P)


def dout_for(shape_out, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(9100 + seed + int(np.prod(shape_out)) % 1000)
    return torch.rand(tuple(shape_out), generator=g) * 2 - 1


def image(B: int, H: int, W: int, C: int, kind: str = "finite") -> torch.Tensor:
    """Sweep source images [B, H, W, C] in [0, 1); "nonfinite": Inf in channel 0 of column 0, -Inf in
    the last channel of column W-1, NaN in row 0 of channel C // 2 and one all-NaN interior texel."""
    g = torch.Generator().manual_seed(8000 + 7 * H + W + 1000 * C + B)
    img = torch.rand((B, H, W, C), generator=g)
    if kind != "finite":
        img[:, :, 0, 0] = float("inf")
        img[:, :, W - 1, C - 1] = float("-inf")
        img[:, 0, :, C // 2] = float("nan")
        img[:, H // 2, W // 2, :] = float("nan")
    return img


def net_output(B: int, H: int, W: int, P: int, kind: str = "finite"):
    """(pred [B, 2P+3, H, W], fg [B, H, W, 3]) in [-1, 1); "nonfinite": Inf in blend weight 0 of column
    0, -Inf in alpha 1 of column W-1, NaN in background channel 2 of row 0, one all-NaN pixel of pred and
    an Inf and a NaN in the reference image."""
    g = torch.Generator().manual_seed(8800 + 3 * H + W + 100 * P + B)
    pred = torch.rand((B, 2 * P + 3, H, W), generator=g) * 2 - 1
    fg = torch.rand((B, H, W, 3), generator=g) * 2 - 1
    if kind != "finite":
        pred[:, 0, :, 0] = float("inf")
        pred[:, P + 1, :, W - 1] = float("-inf")
        pred[:, 2 * P + 2, 0, :] = float("nan")
        pred[:, :, H // 2, W // 2] = float("nan")
        fg[:, H - 1, W // 3, 0] = float("inf")
        fg[:, H // 3, W - 2, 1] = float("nan")
    return pred, fg


# ---------------------------------------------------------------------------
# the sample position, restated (mpiv_common.hpp hom_sample_pos) -- vacuity checks only
# ---------------------------------------------------------------------------

def _fma(a, b, c):
    # float32 operands: the product is exact in float64; the sum is rounded to float64 and then to
    # float32, which equals the single rounding whenever the exact sum fits 53 bits (every lattice
    # family: all terms are small multiples of 2^-2)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def sample_pos(h, H: int, W: int):
    """(px, py) [H, W] float32 of one plane's homography h[9]: the five roundings of hom_sample_pos
    (u / v / w chains, the division by w, the division by H-1 / W-1, to_grid, unnormalize)."""
    h = np.asarray(h, np.float32)
    f = np.float32
    fy, fx = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
    with np.errstate(all="ignore"):
        u = _fma(h[1], fy, h[0] * fx) + h[2]
        v = _fma(h[4], fy, h[3] * fx) + h[5]
        w = _fma(h[7], fy, h[6] * fx) + h[8]
        w = np.where(w == 0, w + f(1e-8), w).astype(f)
        cx = ((u / w).astype(f) / f(H - 1)).astype(f)   # swapped: x / (H-1), utils.py:188
        cy = ((v / w).astype(f) / f(W - 1)).astype(f)
        gx = _fma(np.full_like(cx, 2), cx, np.full_like(cx, -1))
        gy = _fma(np.full_like(cy, 2), cy, np.full_like(cy, -1))
        px = _fma((gx + f(1)).astype(f), np.full_like(gx, f(W) / f(2)), np.full_like(gx, -0.5))
        py = _fma((gy + f(1)).astype(f), np.full_like(gy, f(H) / f(2)), np.full_like(gy, -0.5))
    return px, py


def exact_axis_pos(h, shape):
    px, py = sample_pos(h, *shape)
    return px if x_exact(shape) else py


# ---------------------------------------------------------------------------
# plane sweep
# ---------------------------------------------------------------------------

SWEEP_K = [[64.0, 0.0, 32.0], [0.0, 64.0, 32.0], [0.0, 0.0, 1.0]]
SWEEP_DEPTHS = [1.0, 2.0, 4.0, 0.5, 0.25, 8.0, 1.0 / 3.0, 0.0, -1.0]  # the last three inexact / degenerate
SWEEP_SRC = (64, 64)
SWEEP_TGT = [(64, 64), (48, 80)]


def sweep_poses() -> torch.Tensor:
    """[4, 4, 4]: identity rotations with translations k/64 and k/128 (at depth 1 the source position
    is the target pixel shifted by k or k/2 texels exactly)."""
    ts = [(1 / 64, -2 / 64, 0.0), (3 / 128, 1 / 128, 0.0), (-65 / 64, 63 / 128, 0.0), (0.0, 64 / 64, 1 / 64)]
    out = []
    for t in ts:
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = t
        out.append(m)
    return torch.from_numpy(np.stack(out))


def sweep_depths(D: int):
    return [SWEEP_DEPTHS[i % len(SWEEP_DEPTHS)] * (1 + i // len(SWEEP_DEPTHS)) for i in range(D)]


def degenerate_depth_map(B: int, H: int, W: int) -> torch.Tensor:
    """[B, H, W] depths 1, 2, 0.5 in bands with a 0, a negative value, an Inf and a NaN patch."""
    d = torch.ones((B, H, W))
    d[:, H // 3:] = 2.0
    d[:, 2 * H // 3:] = 0.5
    d[:, 1, 1:4] = 0.0
    d[:, 5:7, 8:11] = -1.0
    d[:, 9, 20:23] = float("inf")
    d[:, 12, 30:32] = float("nan")
    return d


# ---------------------------------------------------------------------------
# grid_sample boundary coordinates
# ---------------------------------------------------------------------------

def boundary_pixels(n: int):
    return [-1.5, -1.0, -0.5, 0.0, n - 1.0, n - 0.5, float(n), n + 0.5, 1e10, 3e38, float("inf"), float("-inf"),
            float("nan"), -0.0, 2.0, 2.5]


def boundary_coords(N: int, Hi: int, Wi: int) -> torch.Tensor:
    """[N, Ho, Wo, 2] coordinates in the wrappers' [0, 1] units whose source pixel px = c * Wi - 0.5
    lies on the boundary set in x (along Wo) and in y (along Ho); Wi and Hi are powers of two, so the
    positions are exact.  The zero of the set is given as the coordinate -0.0 itself."""
    def unit(vals, n):
        out = []
        for p in vals:
            c = (np.float64(p) + 0.5) / n
            out.append(np.float32(-0.0) if (p == 0 and np.signbit(p)) else np.float32(c))
        return np.array(out, np.float32)
    cx, cy = unit(boundary_pixels(Wi), Wi), unit(boundary_pixels(Hi), Hi)
    with np.errstate(all="ignore"):
        grid = np.stack(np.meshgrid(cx, cy, indexing="xy"), axis=-1)  # [Ho, Wo, 2] = (x, y)
    return torch.from_numpy(np.broadcast_to(grid, (N,) + grid.shape).copy())
