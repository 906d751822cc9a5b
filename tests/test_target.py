"""CPU: the ABI surface of the render into a target frame of its own size (mpiv_render_packed_tgt and its
u8 / f16 twins, their dry runs), argument validation, the golden fixture, the homography route with
separate source and target intrinsics on the host, and mpi_render_view_torch2's argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import target_cases as tc
from conftest import assert_bits
from test_abi import declared_symbols

import mpi_vision_amd
from mpi_vision_amd import _host, _lib
from mpi_vision_amd import utils as mvu

ENTRIES = ("mpiv_render_packed_tgt", "mpiv_render_packed_u8_tgt", "mpiv_render_packed_f16_tgt")


def test_entries_declared_exported_and_bound():
    """Additive: the header declares the three entries, the library exports them, _lib binds them in a
    dict of their own (tests/stream_cases.py holds one replay case per _SIGS entry), the ABI version
    stays 17."""
    import stream_cases
    L = _lib.load()
    for name in ENTRIES:
        assert name in declared_symbols() and hasattr(L, name) and name in _lib.EXPORTS, name
        assert name in _lib._SIGS_TGT and name not in _lib._SIGS, name
        assert getattr(L, name).argtypes == _lib._SIGS_TGT[name]
        assert len(_lib._SIGS_TGT[name]) == 10  # packed, Hs, Ws, P, homs, V, Ht, Wt, out, stream
    assert _lib.ABI_VERSION == 17 and L.mpiv_abi_version() == 17
    assert set(_lib._SIGS) == stream_cases.COVERED | set(stream_cases.EXCLUDED)
    assert "mpi_render_view_torch2" in mpi_vision_amd.__all__ and mpi_vision_amd.mpi_render_view_torch2 is mvu.mpi_render_view_torch2


def _err(L):
    return L.mpiv_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_render_arguments_rejected(name):
    L = _lib.load()
    p = ctypes.c_void_p(256)
    render = getattr(L, name)
    for k in (0, 4, 8):  # packed, homs, out
        args = [p, 8, 8, 2, p, 1, 6, 6, p, None]
        args[k] = None
        assert render(*args) == -1 and f"{name}: null pointer" in _err(L), k
    for Hs, Ws, P, V, Ht, Wt in ((0, 8, 2, 1, 6, 6), (8, 0, 2, 1, 6, 6), (8, 8, 0, 1, 6, 6), (8, 8, 2, 0, 6, 6),
                                 (8, 8, 2, 1, 0, 6), (8, 8, 2, 1, 6, -1)):
        assert render(p, Hs, Ws, P, p, V, Ht, Wt, p, None) == -1 and "bad shape" in _err(L), (Hs, Ws, P, V, Ht, Wt)
    # the 2 GiB limit is the SOURCE plane's; a side of 2^22 is refused on either
    big = 23171 if name != "mpiv_render_packed_tgt" else 11584
    assert render(p, big, big, 2, p, 1, 6, 6, p, None) == -1 and "padded plane larger than 2 GiB" in _err(L)
    assert render(p, 8, 8, 2, p, 1, 2, 1 << 22, p, None) == -1 and "a side >= 2^22" in _err(L)
    if name != "mpiv_render_packed_tgt":  # the narrow formats have the fast recipe only
        for Hs, Ws, Ht, Wt in ((1, 8, 6, 6), (8, 8, 1, 6), (8, 8, 6, 1)):
            assert render(p, Hs, Ws, 2, p, 1, Ht, Wt, p, None) == -1 and "bad shape (H, W >= 2)" in _err(L)


def test_routes():
    """The dry runs: the target kernels' names and grids (tile counts from the TARGET), the flavour policy
    on the sample's advance Ws/(Ht-1), Hs/(Wt-1), the generic recipe below 2 on any of the four
    dimensions, and the same-size kernel itself where the sizes agree."""
    r = _lib.route
    # both advances ~1: the tap-reuse rows kernel, (R, D) by view count; grid from the 150 x 160 target
    rows = "render_rows_tgt_kernel<false, %d, true, false, %d, false, false>"
    assert r("render_packed_tgt", 160, 150, 8, 1, 150, 160) == (rows % (4, 4), 3 * 10 * 1 * 256)
    assert r("render_packed_tgt", 160, 150, 8, 3, 150, 160) == (rows % (8, 4), 3 * 5 * 3 * 256)
    assert r("render_packed_tgt", 160, 150, 8, 40, 150, 160) == (rows % (6, 3), 3 * 7 * 40 * 256)
    # advances far from 1 on a launch that does not fill the chip: the one-row kernel
    for Hs, Ws, Ht, Wt in ((75, 80, 150, 160), (150, 160, 75, 80), (37, 203, 150, 70)):
        name, grid = r("render_packed_tgt", Hs, Ws, 8, 3, Ht, Wt)
        assert name == "render_packed_tgt_kernel<false, true>" and grid == -(-Wt // 64) * -(-Ht // 4) * 3 * 256
    # ... and same-row reuse once it does (advance 0.47 rows per output row)
    assert r("render_packed_tgt", 75, 80, 8, 140, 150, 160)[0] == rows.replace("false, false>", "true, false>") % (6, 3)
    # config 4's MPI into 2048^2 (advance 0.5), 512^2 (advance 2) and a 1024^2 frame (the same-size kernel)
    assert r("render_packed_tgt", 1024, 1024, 128, 1, 2048, 2048)[0] == \
        "render_rows_tgt_kernel<false, 6, true, false, 3, true, true>"
    assert r("render_packed_tgt", 1024, 1024, 128, 8, 512, 512)[0] == "render_packed_tgt_kernel<false, true>"
    assert r("render_packed_tgt", 1024, 1024, 128, 125, 1024, 1024) == r("render_packed", 1024, 1024, 128, 125)
    # the generic recipe when any of the four dimensions is below 2
    for Hs, Ws, Ht, Wt in ((1, 48, 20, 24), (48, 1, 20, 24), (20, 24, 1, 48), (20, 24, 48, 1)):
        assert r("render_packed_tgt", Hs, Ws, 3, 1, Ht, Wt)[0] == "render_packed_tgt_kernel<false, false>"
    assert r("render_packed_u8_tgt", 160, 150, 8, 3, 150, 160) == ("render_u8_tgt_kernel<4, true, 4>", 3 * 10 * 3 * 256)
    assert r("render_packed_f16_tgt", 160, 150, 8, 72, 150, 160)[0] == "render_f16_tgt_kernel<4, true, 2>"
    assert r("render_packed_u8_tgt", 37, 203, 7, 3, 150, 70)[0] == "render_u8_tgt_kernel<2, false, 2>"
    assert r("render_packed_f16_tgt", 64, 64, 4, 2, 64, 64) == r("render_packed_f16", 64, 64, 4, 2)
    with pytest.raises(RuntimeError, match="wrong argument count"):
        r("render_packed_tgt", 64, 64, 2, 1)


@pytest.mark.parametrize("name", list(tc.CASES) + list(tc.DEGENERATE))
def test_golden_shapes(name):
    g = tc.golden()
    B, (Hs, Ws), P, (Ht, Wt) = {**tc.CASES, **tc.DEGENERATE}[name]
    assert tuple(g[f"{name}_src"]) == (Hs, Ws, P) and tuple(g[f"{name}_tgt"]) == (Ht, Wt)
    assert g[f"{name}_out"].shape == (B, Ht, Wt, 3) and g[f"{name}_H"].shape == (P, B, 3, 3)
    assert g[f"{name}_pose"].shape == (B, 4, 4) and g[f"{name}_Ks"].shape == g[f"{name}_Kt"].shape == (B, 3, 3)
    assert tuple(tc.mpi(name).shape) == (B, Hs, Ws, P, 4)
    same_k = np.array_equal(g[f"{name}_Ks"], g[f"{name}_Kt"])
    assert same_k == (name in ("ta", "te", "d1", "d2"))
    if name in tc.CASES:
        out = g[f"{name}_out"]
        assert np.isfinite(out).all() and (np.abs(out).sum(-1) > 0).mean() > 0.4
    else:
        assert g[f"{name}_out"].dtype == np.float32
    if name == "tg":
        assert g["tg_grad"].shape == (1, 23, 35, 5, 4) and g["tg_dout"].shape == (1, 31, 29, 3)
        assert np.isfinite(g["tg_grad"]).all() and np.abs(g["tg_grad"]).max() > 0


@pytest.mark.parametrize("name", list(tc.CASES) + list(tc.DEGENERATE))
def test_homographies_host(name):
    """mpiv_render_homographies with K = k_s and Kinv = inverse(k_t) (the memoised torch.inverse of the
    contiguous batch) gives the reference's H bits; with tgt_intrinsics left out it is today's route."""
    pose, depths, ks, kt = tc.cameras(name)
    B = pose.shape[0]
    got = _host.render_homographies(pose, depths, ks, B, tgt_intrinsics=kt)
    assert_bits(got, tc.golden_homs(name).numpy(), f"{name}: H with separate k_s, k_t")
    same = _host.render_homographies(pose, depths, ks, B)
    assert_bits(_host.render_homographies(pose, depths, ks, B, tgt_intrinsics=ks), same.numpy(), "k_t = k_s")
    if not torch.equal(ks, kt):
        assert not torch.equal(got, same)


def test_same_size_homographies_are_the_render(small):
    """te: with k_s = k_t the definition's H are mpi_render_view_torch's."""
    pose, depths, ks, kt = tc.cameras("te")
    assert torch.equal(ks, kt)
    assert_bits(_host.render_homographies(pose, depths, ks, 2), tc.golden_homs("te").numpy())


def test_wrapper_raises():
    """`planes` must be a tensor (the reference's AttributeError); batch and plane counts must agree; float32,
    uint8 and float16 MPIs only; no CPU path."""
    mpi = torch.rand((1, 8, 8, 3, 4))
    pose, K, planes = torch.eye(4)[None], torch.eye(3)[None], torch.tensor([4.0, 2.0, 1.0])

    def call(m, pl=planes, p=pose, size=(6, 7)):
        return mvu.mpi_render_view_torch2(m, p, pl, K, K, *size)

    with pytest.raises(AttributeError):
        call(mpi, [4.0, 2.0, 1.0])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        call(mpi, planes[:2])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        call(mpi, p=pose.repeat(2, 1, 1))
    for bad in (mpi.double(), mpi.to(torch.bfloat16), (mpi * 255).to(torch.int32)):
        with pytest.raises(RuntimeError, match="expects a float32, uint8 or float16 MPI"):
            call(bad)
    with pytest.raises(RuntimeError, match=r"\[B,H,W,P,4\]"):
        call(mpi[..., :3])
    with pytest.raises(RuntimeError, match="size must be"):
        call(mpi, size=(0, 7))
    for ok in (mpi, (mpi * 255).to(torch.uint8), mpi.half()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(ok)
