"""An independent, exact restatement of the per-point geometry helpers and the frame codecs, in numpy.

The reference computes these with `torch.matmul` on the CPU.  ATen's CPU `bmm` runs a naive loop when
contraction * rows * cols < 400 per batch element (plain products, summed in ascending k, every product
and every partial sum rounded) and hands larger products to MKL sgemm, which on these shapes rounds as a
chain of fused multiply-adds in ascending k: fma(a2, x2, fma(a1, x1, a0 * x0)).  `chain` states both,
`aten_plain` the size rule, and the functions below the helpers on top of them: IEEE fp32 division, the
reference's `w == 0 -> w + 1e-8` and `z + 1e-10`, its codecs and torch's float -> uint8 cast.

The fused multiply-add is emulated exactly: the product of two floats is exact in a double (48 <= 53
bits), the sum with the addend is taken with its rounding error (TwoSum), rounded to odd in the double and
only then rounded to float, which is the correctly rounded result (a double carries more than 24 + 2
bits).  `float64(a) * b + c` cast to float rounds twice and is wrong on about one value in 10^4.

Nothing here is imported from mpi_vision_amd: the tests compare the kernels with it, and the recorder
(tools/gen_goldens_geometry.py) holds it to the reference for every stored shape."""
from __future__ import annotations

import numpy as np

F = np.float32
EPS_W = F(1e-8)    # divide_safe_torch, utils.py:36-38
EPS_Z = F(1e-10)   # cam2pixel_torch, utils.py:391


def fma32(a, b, c):
    """Correctly rounded a * b + c for float32 arrays (broadcast)."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c == s + err exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even    # inexact and even: the odd neighbour on err's side
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F)


def chain(A, X, plain: bool):
    """A [..., R, K] @ X [..., K, N] -> [..., R, N], summed in ascending k: plain products and sums
    (each rounded) or a chain of fused multiply-adds on the first product."""
    A, X = np.asarray(A, F), np.asarray(X, F)
    K = A.shape[-1]
    assert X.shape[-2] == K
    with np.errstate(all="ignore"):
        s = A[..., :, 0:1] * X[..., 0:1, :]
        for k in range(1, K):
            a, x = A[..., :, k:k + 1], X[..., k:k + 1, :]
            s = s + a * x if plain else fma32(a, x, s)
    return np.ascontiguousarray(s, F)


def aten_plain(K: int, rows: int, cols: int) -> bool:
    """ATen's CPU bmm: the naive loop (plain chain) below 400 multiply-adds per batch element."""
    return K * rows * cols < 400


def tp_plain(n: int, batched: bool) -> bool:
    """transform_points_torch: [M,n,3] @ [M,3,3]^T; a homography without batch dimensions is `mm` (MKL)."""
    return batched and aten_plain(3, n, 3)


def p2c_plain(n: int) -> bool:
    return aten_plain(3, 3, n)      # [B,3,3] @ [B,3,n]


def c2p_plain(n: int) -> bool:
    return aten_plain(4, 4, n)      # [B,4,4] @ [B,4,n]


def _T(H):
    return np.swapaxes(np.asarray(H, F), -1, -2)


def transform_points(pts, H, plain: bool):
    """pts [..., n, 3], H [..., 3, 3] -> pts @ H^T (utils.py:69-88)."""
    return chain(pts, _T(H), plain)


def normalize_homogeneous(pts):
    """pts [..., k+1] -> (uv / w [..., k], pts after the call): w == 0 (either sign) becomes w + 1e-8 in
    place, every other w (NaN, Inf, subnormal) is left alone (utils.py:90-101, 35-39)."""
    after = np.array(pts, F, copy=True)
    w = after[..., -1]
    with np.errstate(all="ignore"):
        w[w == 0] += EPS_W
        out = after[..., :-1] / after[..., -1:]
    return np.ascontiguousarray(out, F), after


def pixel2cam(depth, pix, ki, homogeneous: bool, plain: bool):
    """depth [B,n], pix [B,3,n], ki = inverse(K) [B,3,3] -> [B, 3 or 4, n] (utils.py:356-375)."""
    with np.errstate(all="ignore"):
        cam = chain(ki, pix, plain) * np.asarray(depth, F)[:, None, :]
    if homogeneous:
        cam = np.concatenate([cam, np.ones_like(cam[:, :1])], axis=1)
    return np.ascontiguousarray(cam, F)


def cam2pixel(cam, proj, plain: bool):
    """cam [B,4,n], proj [B,4,4] -> [B,n,2] = (proj @ cam)[:2] / ((proj @ cam)[2] + 1e-10) (utils.py:377-393)."""
    u = chain(proj, cam, plain)
    with np.errstate(all="ignore"):
        xy = u[:, 0:2] / (u[:, 2:3] + EPS_Z)
    return np.ascontiguousarray(np.swapaxes(xy, 1, 2), F)


def plane_coords(pts, H, Ht: int, Wt: int, plain: bool):
    """transform_plane_imgs_torch's sample coordinates (utils.py:178-188): pts [..., n, 3], H [..., 3, 3]
    -> [..., n, 2] = (u / w / (Ht - 1), v / w / (Wt - 1)), the reference's swapped normalisation."""
    uv, _ = normalize_homogeneous(transform_points(pts, H, plain))
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(uv / np.array([Ht - 1, Wt - 1], F), F)


def preprocess(x):
    """image * 2 - 1 (utils.py:334-342)."""
    with np.errstate(all="ignore"):
        return np.asarray(x, F) * F(2) - F(1)


def deprocess_u8(x):
    """(((image + 1) / 2) * 255) cast to uint8 as torch's CPU cast does: truncation to int32 (NaN and
    values outside int32 give INT_MIN), then the low byte (utils.py:344-352)."""
    with np.errstate(all="ignore"):
        v = ((np.asarray(x, F) + F(1)) / F(2)) * F(255)
        ok = np.abs(v) < F(2147483648.0)
        q = np.where(ok, np.trunc(np.where(ok, v, 0).astype(np.float64)), 0).astype(np.int64)
    return (q & 0xFF).astype(np.uint8)


def same(got, want):
    """None when got and want have the same NaN positions and the same bits everywhere else (a NaN's
    payload is not part of the contract), else a short description of the difference."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    ng, nw = np.isnan(got), np.isnan(want)
    if not np.array_equal(ng, nw):
        return f"NaN positions differ ({int(ng.sum())} vs {int(nw.sum())})"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~ng
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), got.shape)
        return f"{int(bad.sum())}/{bad.size} values differ, first at {i}: got {got[i]!r}, want {want[i]!r}"
    return None


def ndiff(a, b) -> int:
    """How many values differ in bits (NaN against NaN counts as equal)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())
