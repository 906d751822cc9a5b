"""Shared by tests/test_target.py and tests/test_target_gpu.py: the golden fixture of
mpi_render_view_torch2 (tests/golden/target.npz, tools/gen_goldens_target.py) and its seeded inputs."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

from mpi_vision_amd import configs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (B, (Hs, Ws), P, (Ht, Wt))
CASES = {"ta": (2, (40, 72), 6, (80, 144)), "tb": (2, (40, 72), 6, (23, 31)), "tc": (1, (37, 53), 7, (70, 70)),
         "td": (1, (64, 66), 4, (9, 5)), "te": (2, (40, 72), 6, (40, 72)), "tg": (1, (23, 35), 5, (31, 29))}
DEGENERATE = {"d1": (1, (20, 24), 3, (1, 48)), "d2": (1, (1, 48), 3, (20, 24))}


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLD, "target.npz"))


@functools.lru_cache(maxsize=None)
def mpi(name) -> torch.Tensor:
    """The case's seeded MPI [B, Hs, Ws, P, 4] (CPU), as the generator made it."""
    g = golden()
    seed = int(g[f"{name}_seed"])
    if name in DEGENERATE:
        B, (Hs, Ws), P, _ = DEGENERATE[name]
        return torch.rand((1, Hs, Ws, P, 4), generator=torch.Generator().manual_seed(seed)) * 2 - 1
    B, (Hs, Ws), P, _ = CASES[name]
    return configs.synthetic_mpi(B, Hs, Ws, P, seed)


def cameras(name):
    """(pose, depths, k_s, k_t) of a case as CPU tensors."""
    g = golden()
    return tuple(torch.tensor(g[f"{name}_{k}"]) for k in ("pose", "depths", "Ks", "Kt"))


def golden_homs(name) -> torch.Tensor:
    """The reference's homographies [P,B,3,3] as the kernels take them: [B, P, 9]."""
    H = golden()[f"{name}_H"]
    return torch.tensor(np.ascontiguousarray(H.transpose(1, 0, 2, 3)).reshape(H.shape[1], H.shape[0], 9))
