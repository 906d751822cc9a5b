"""Shared by tests/test_planecolor.py (CPU) and tests/test_planecolor_gpu.py: the route table of
mpiv_render_packed_alpha, the constructed float MPI the plane-colour render is defined on, and the
golden fixture (tests/golden/planecolor.npz, tools/gen_goldens_planecolor.py).

A plain module: no fixtures, nothing collected by pytest."""
from __future__ import annotations

import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ((H, W, P), views, template arguments of render_alpha_kernel<R, VS, D>): the f16 render's table --
# the dispatcher has the same thresholds.  2 plain rows (stretched, small launch); 4 rows with
# vertical reuse and 4 in flight (near-square, under 2048 blocks); 2 in flight from 2048 blocks up,
# near-square (1024 views of 1 x 2 tiles of 64 x 16) and stretched (1024 views of 1 x 2 tiles of
# 64 x 32: 2048 of them, the launch fills the chip).  Each instantiation's smallest shape.
ROUTES = [((37, 203, 7), 7, "2, false, 2"), ((64, 66, 16), 7, "4, true, 4"), ((20, 18, 3), 1024, "4, true, 2"),
          ((36, 64, 2), 1024, "4, true, 2")]
ROUTE_IDS = ["plain2", "reuse_flight4", "reuse_flight2", "reuse_flight2_stretched"]
# every instantiation mpiv_render_packed_alpha can launch (abi.hip)
INSTANTIATIONS = {"2, false, 2", "4, true, 4", "4, true, 2"}


def kernel_name(route: str) -> str:
    return f"render_alpha_kernel<{route}>"


def constructed(alpha: np.ndarray, colors: np.ndarray) -> np.ndarray:
    """[..., P] alpha + [P, 3] colours -> the float MPI [..., P, 4]: RGB = colors[p] all over plane p."""
    out = np.empty(alpha.shape + (4,), np.float32)
    out[..., :3] = colors.astype(np.float32)
    out[..., 3] = alpha
    return out


def depth_colors(depths: np.ndarray) -> np.ndarray:
    d = depths.astype(np.float32)
    return np.stack([np.float32(1.0) / d, d, np.ones_like(d)], -1)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "planecolor.npz"))


def golden_homs(name: str) -> np.ndarray:
    """The reference's homographies of case `name`, [B, P, 9]."""
    h = golden()[f"{name}_H"]  # [P, B, 3, 3]
    return np.ascontiguousarray(h.transpose(1, 0, 2, 3)).reshape(h.shape[1], h.shape[0], 9)
