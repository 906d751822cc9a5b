"""CPU tests of the plane sweep's differentiable route: the ABI surface of its entry
(mpiv_plane_sweep_backward and its two workspace sizes), its refusals -- all raised before the first HIP
call, so they need no GPU -- and the golden fixtures' own assertions (tests/golden/psvgrad.npz,
tools/gen_goldens_psvgrad.py)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLD, REPO

from mpi_vision_amd import _lib

CASES = ["psv", "psv1", "psv33", "one2"]
U = 2.0 ** -24
NAMES = ("mpiv_plane_sweep_backward", "mpiv_plane_sweep_backward_workspace_size",
         "mpiv_plane_sweep_backward_workspace_size_min")


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "psvgrad.npz")))


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "mpiv.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(", header), n
        assert n in _lib.EXPORTS
    assert "mpiv_plane_sweep_backward" in _lib._SIGS_PSV and "mpiv_plane_sweep_backward" not in _lib._SIGS
    assert len(_lib._SIGS_PSV["mpiv_plane_sweep_backward"]) == 21
    L = _lib.load_main()
    assert L.mpiv_abi_version() == 17 == _lib.ABI_VERSION
    assert L.mpiv_plane_sweep_backward.argtypes == _lib._SIGS_PSV["mpiv_plane_sweep_backward"]
    for n in NAMES[1:]:
        assert getattr(L, n).argtypes == [_lib.ctypes.c_int] * 7 and getattr(L, n).restype == _lib.ctypes.c_size_t
    with open(os.path.join(REPO, "mpi_vision_amd", "csrc", "SOURCES")) as f:
        assert "psv_bwd.hip" in f.read().split()
    assert hasattr(_lib, "PlaneSweepFunction") and hasattr(_lib, "plane_sweep_backward")


def test_workspace_sizes():
    L = _lib.load_main()
    full, least = L.mpiv_plane_sweep_backward_workspace_size, L.mpiv_plane_sweep_backward_workspace_size_min
    prev = (0, 0)
    for D in (1, 2, 3, 6, 33, 64):
        f, m = full(2, 30, 44, 3, 30, 44, D), least(2, 30, 44, 3, 30, 44, D)
        assert 0 < m <= f and (D > 1 or m == f), D
        assert f > prev[0] and m > prev[1], "monotone in D"
        # per pair: positions, two key and two id arrays (24 B a pixel) and the bounds table (8 B a bucket)
        assert f >= 2 * D * (30 * 44 * 24 + 31 * 45 * 8) and m >= 2 * (30 * 44 * 24 + 31 * 45 * 8)
        prev = (f, m)
    # the config-3 shape ungrouped is over a gigabyte; one plane per group is a small fraction of it
    assert full(1, 768, 1024, 3, 768, 1024, 64) > (1 << 30) > 16 * least(1, 768, 1024, 3, 768, 1024, 64)
    # B*G stays within the grid's y limit: the full size stops growing with D there
    assert full(40000, 2, 2, 1, 2, 2, 3) == least(40000, 2, 2, 1, 2, 2, 3)


def test_size_functions_return_0_for_what_cannot_be_indexed():
    L = _lib.load_main()
    for fn in (L.mpiv_plane_sweep_backward_workspace_size, L.mpiv_plane_sweep_backward_workspace_size_min):
        assert fn(1, 4, 4, 3, 1 << 16, 1 << 15, 2) == 0        # Ht*Wt = 2^31
        assert fn(1, (1 << 16) - 1, 1 << 15, 1, 4, 4, 2) == 0  # (Hs+1)*(Ws+1) = 2^31 + 2^15
        assert fn(1, 4, 4, 1 << 16, 4, 4, 1 << 15) == 0        # D*C = 2^31
        assert fn(1 << 16, 4, 4, 1, 4, 4, 2) == 0              # B beyond the grid's y limit
        assert fn(1 << 15, 4, 4, 1, 4, 4, 1 << 16) == 0        # B*D partial records = 2^31
        for bad in ((0, 4, 4, 3, 4, 4, 2), (1, 4, 4, 3, 0, 4, 2), (1, 4, 4, 3, 4, 4, 0), (1, 4, 4, 3, 4, 4, -1)):
            assert fn(*bad) == 0
        assert fn(1, 4, 4, 3, 4, 4, 2) > 0


def test_entry_refuses_before_any_hip_call():
    """Fake pointers: every refusal returns -1 with its message; nothing is dereferenced or launched
    (there is no device here to launch on)."""
    L = _lib.load_main()
    st = (_lib.ctypes.c_int64 * 4)(1, 1, 1, 1)
    ok = dict(img=8, st=st, B=1, Hs=4, Ws=4, C=3, ki=8, proj=8, depths=8, D=2, Ht=4, Wt=4, dout=8, dst=st, dimg=8,
              ddepths=None, dki=None, dproj=None, ws=16, nbytes=1 << 20, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.mpiv_plane_sweep_backward(*a.values())
        return rc, L.mpiv_last_error()

    for k in ("img", "st", "ki", "proj", "depths", "dout", "dst", "ws"):
        rc, msg = call(**{k: None})
        assert rc == -1 and b"null pointer" in msg, k
    rc, msg = call(dimg=None)
    assert rc == -1 and b"no gradient" in msg
    for k in ("B", "Hs", "Ws", "C", "Ht", "Wt"):
        rc, msg = call(**{k: 0})
        assert rc == -1 and b"bad shape" in msg, k
    for d in (0, -3):
        rc, msg = call(D=d)
        assert rc == -1 and b"D must be positive" in msg
    rc, msg = call(Ht=1 << 16, Wt=1 << 15)
    assert rc == -1 and b"limited to" in msg
    rc, msg = call(B=1 << 16)
    assert rc == -1 and b"limited to" in msg
    need = L.mpiv_plane_sweep_backward_workspace_size_min(1, 4, 4, 3, 4, 4, 2)
    rc, msg = call(nbytes=need - 1)
    assert rc == -1 and b"workspace" in msg and str(need).encode() in msg
    rc, msg = call(ws=24)
    assert rc == -1 and b"16-byte aligned" in msg
    for k in ("ddepths", "dki", "dproj"):  # each output alone is a request
        rc, msg = call(dimg=None, nbytes=need - 1, **{k: 8})
        assert rc == -1 and b"workspace" in msg, k


def fold(parts, descending):
    order = parts[::-1] if descending else parts
    acc = order[0]
    for p in order[1:]:
        acc = acc + p
    return acc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_source(name, g, dimg, D, B, N, ddepths=None):
    dimg_d = g["dimg_d"]
    assert dimg_d.shape == (D,) + dimg.shape and g["ddepth_d"].shape[:2] == (D, B)
    assert same_bits(fold(list(dimg_d), True), dimg), f"{name}: the descending fold is not dimg"
    if D > 1:
        asc = np.ascontiguousarray(fold(list(dimg_d), False)).view(np.uint32)
        diff = (asc != np.ascontiguousarray(dimg).view(np.uint32)).mean()
        assert diff >= 0.01, f"{name}: the ascending fold differs in only {100 * diff:.2f} % of the elements"
    assert (np.abs(dimg).sum(-1) != 0).mean() >= 0.5, f"{name}: too few live texels"
    for what, n in (("dki", 9), ("dproj", 16)):
        got, S64, A = (g[what + s] for s in ("", "_S64", "_A"))
        assert got.shape == S64.shape == A.shape == (B, n) and S64.dtype == np.float64
        assert (np.abs(got - S64) <= gamma(D * N) * A).all(), f"{name}: the reference's {what} is outside gamma_N * A"
    assert not g["dproj"][:, 12:].any()
    S64, A = g["ddepths_S64"], g["ddepths_A"]
    assert S64.shape == A.shape == (D,)
    assert np.allclose(S64, g["ddepth_d"].astype(np.float64).sum((1, 2, 3)), rtol=1e-12, atol=0)
    if ddepths is not None:
        assert (np.abs(ddepths - S64) <= gamma(B * N) * A).all(), f"{name}: the reference's ddepths"


@pytest.mark.parametrize("name", CASES)
def test_goldens_own_assertions(name, gold):
    g = {k[len(name) + 1:]: v for k, v in gold.items() if k.startswith(name + "_")}
    dimg = g["dimg"] if g["dimg"].ndim == 4 else g["dimg"][None]
    D = len(g["ddepths"])
    B = dimg.shape[0]
    N = g["ddepth_d"].shape[2] * g["ddepth_d"].shape[3]
    assert D == {"psv": 6, "psv1": 1, "psv33": 33, "one2": 3}[name]
    check_source(name, g, dimg, D, B, N, g["ddepths"])
    for k in (("dKs", "dKt") if name == "one2" else ("dK",)) + ("dpose",):
        assert np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0
    if name == "psv":
        d = gold["psv_depths"]
        assert len(set(d.tolist())) == D - 1, "one depth value is repeated"
    # exact-inverse cameras: power-of-two focal lengths, dyadic principal points
    for k in (("Ks", "Kt") if name == "one2" else ("K",)):
        K = gold[f"{'psv' if name == 'psv1' else name}_{k}"].reshape(-1, 3, 3)
        assert (np.log2(K[:, 0, 0]) % 1 == 0).all() and (np.log2(K[:, 1, 1]) % 1 == 0).all()
        assert (K[:, :2, 2] * 2 % 1 == 0).all()


def test_network_input_goldens_own_assertions(gold):
    g = {k[4:]: v for k, v in gold.items() if k.startswith("fni_")}
    B, H, W, _ = g["ref"].shape
    S, D = g["src_poses"].shape[1], len(g["depths"])
    assert (S, D) == (2, 4) and g["dout"].shape == (B, H, W, 3 + S * D * 3)
    assert same_bits(g["dref"], g["dout"][..., :3])
    for i in range(S):
        per = {k: g[k][i] for k in ("dimg_d", "ddepth_d", "dki", "dki_S64", "dki_A", "dproj", "dproj_S64", "dproj_A",
                                    "ddepths_S64", "ddepths_A")}
        check_source(f"fni[{i}]", per, g["dsrc"][..., 3 * i:3 * i + 3], D, B, H * W)
    err = np.abs(g["ddepths"] - g["ddepths_S64"].sum(0))
    assert (err <= gamma(S * B * H * W) * g["ddepths_A"].sum(0)).all()
    for k in ("dref_pose", "dsrc_poses", "dK"):
        assert np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0
