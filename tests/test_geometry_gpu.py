"""GPU: the per-point geometry helpers and the frame codecs against the reference's goldens
(tests/golden/geometry.npz) and the exact restatement (tests/geometry_cases.py), bit for bit, on both sides
of ATen's small-matmul threshold (plain products below 400 multiply-adds per batch element, MKL's FMA chain
from there on), on both sides of a 256-thread block, for k = 1..3, zero denominators and non-finite values.

The *_dropin tests go through the Python drop-ins, which pick the chain from the shape.  The *_entries
tests call the raw _chain entries with both flag values (so the plain form is seen to stay unfused and the
FMA form fused at every size) and the entries without a flag, which stay the FMA chain at every n.  NaN
positions are compared as sets (a NaN's payload is not part of the contract).  Every test is a handful of
launches on at most 6 000 points."""
import numpy as np
import pytest
import torch

import geometry_cases as gc
import mpi_vision_amd as mv
from mpi_vision_amd import _lib
from test_geometry import gen, gold, host_agrees, ok, tp_want  # noqa: F401  (gold: the module's fixture)

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _raw(name, dev, out_shape, *args):
    """One raw entry call on the current stream: args up to the output, then (out, stream) appended."""
    out = torch.empty(out_shape, device=dev, dtype=torch.float32)
    _lib._call(name, *args, out, _lib._stream(dev))
    return _np(out)


# ---------------------------------------------------------------------------
# transform_points_torch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,n", gen.TP)
def test_transform_points_dropin(M, n, gold, dev):
    want, mine = tp_want(gold, M, n)
    pts, H = gen.tp_inputs(M, n)
    got = _np(mv.transform_points_torch(pts.to(dev), H.to(dev)))
    ok(got, want, f"transform_points_torch M={M} n={n} against the reference")
    ok(got, mine, f"transform_points_torch M={M} n={n} against the restatement")


@pytest.mark.parametrize("M,n", gen.TP)
def test_transform_points_entries(M, n, gold, dev):
    pts, H = gen.tp_inputs(M, n)
    m = max(M, 1)
    p, h = pts.reshape(m, n, 3).contiguous().to(dev), H.reshape(m, 9).contiguous().to(dev)
    reference, _ = tp_want(gold, M, n)
    for plain in (False, True):
        want = gc.transform_points(pts.reshape(m, n, 3).numpy(), H.reshape(m, 3, 3).numpy(), plain)
        got = _raw("mpiv_transform_points_chain", dev, (m, n, 3), p, m, n, h, int(plain))
        ok(got, want, f"mpiv_transform_points_chain M={M} n={n} plain={plain}")
        if plain == gc.tp_plain(n, M > 0):
            ok(got.reshape(reference.shape), reference, f"mpiv_transform_points_chain M={M} n={n} against the reference")
        if not plain:  # the entry without a flag: the MKL regime at every n, as before
            ok(_raw("mpiv_transform_points", dev, (m, n, 3), p, m, n, h), want, f"mpiv_transform_points M={M} n={n}")


# ---------------------------------------------------------------------------
# pixel2cam_torch / cam2pixel_torch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("homogeneous", [True, False])
@pytest.mark.parametrize("B,n", gen.P2C)
def test_pixel2cam_dropin(B, n, homogeneous, gold, dev):
    depth, pix, K = gen.p2c_inputs(B, n)
    want = gold[f"p2c_{B}_{n}"]
    if not homogeneous:  # recorded as a digest of the reference's own [B,3,H,W] result
        want = np.ascontiguousarray(want[:, :3])
        assert gen.sha(want) == gold["shas"][f"p2c_{B}_{n}_h0"]
    got = _np(mv.pixel2cam_torch(depth.to(dev), pix.to(dev), K.to(dev), is_homogeneous=homogeneous))
    ki = torch.inverse(K)  # as the reference and the drop-in compute it, on this host
    mine = gc.pixel2cam(depth.reshape(B, n).numpy(), pix.reshape(B, 3, n).numpy(), ki.numpy(), homogeneous,
                        gc.p2c_plain(n))
    ok(got, mine.reshape(got.shape), f"pixel2cam_torch B={B} n={n} against the restatement")
    if host_agrees(ki, gold[f"p2c_{B}_{n}_ki"]):  # (test_pixel2cam_entries holds the kernel to it on any host)
        ok(got, want, f"pixel2cam_torch B={B} n={n} homogeneous={homogeneous} against the reference")


@pytest.mark.parametrize("B,n", gen.P2C)
def test_pixel2cam_entries(B, n, gold, dev):
    depth, pix, K = gen.p2c_inputs(B, n)
    ki = torch.tensor(gold[f"p2c_{B}_{n}_ki"])  # the reference's K^-1 bits: the goldens on any host
    d, p, k = (t.contiguous().to(dev) for t in (depth.reshape(B, n), pix.reshape(B, 3, n), ki.reshape(B, 9)))
    for homogeneous in (1, 0):
        for plain in (False, True):
            want = gc.pixel2cam(depth.reshape(B, n).numpy(), pix.reshape(B, 3, n).numpy(), ki.numpy(),
                                bool(homogeneous), plain)
            got = _raw("mpiv_pixel2cam_chain", dev, want.shape, d, p, k, B, n, homogeneous, int(plain))
            ok(got, want, f"mpiv_pixel2cam_chain B={B} n={n} homogeneous={homogeneous} plain={plain}")
            if plain == gc.p2c_plain(n):
                reference = gold[f"p2c_{B}_{n}"].reshape(B, 4, n)[:, :want.shape[1]]
                ok(got, reference, f"mpiv_pixel2cam_chain B={B} n={n} homogeneous={homogeneous} against the reference")
            if not plain:
                ok(_raw("mpiv_pixel2cam", dev, want.shape, d, p, k, B, n, homogeneous), want,
                   f"mpiv_pixel2cam B={B} n={n} homogeneous={homogeneous}")


@pytest.mark.parametrize("B,n", gen.C2P)
def test_cam2pixel_dropin(B, n, gold, dev):
    cam, proj = gen.c2p_inputs(B, n)
    got = _np(mv.cam2pixel_torch(cam.to(dev), proj.to(dev)))
    ok(got, gold[f"c2p_{B}_{n}"], f"cam2pixel_torch B={B} n={n} against the reference")
    mine = gc.cam2pixel(cam.reshape(B, 4, n).numpy(), proj.numpy(), gc.c2p_plain(n))
    ok(got, mine.reshape(got.shape), f"cam2pixel_torch B={B} n={n} against the restatement")


@pytest.mark.parametrize("B,n", gen.C2P)
def test_cam2pixel_entries(B, n, gold, dev):
    cam, proj = gen.c2p_inputs(B, n)
    c, p = cam.reshape(B, 4, n).contiguous().to(dev), proj.reshape(B, 16).contiguous().to(dev)
    for plain in (False, True):
        want = gc.cam2pixel(cam.reshape(B, 4, n).numpy(), proj.numpy(), plain)
        got = _raw("mpiv_cam2pixel_chain", dev, (B, n, 2), c, p, B, n, int(plain))
        ok(got, want, f"mpiv_cam2pixel_chain B={B} n={n} plain={plain}")
        if plain == gc.c2p_plain(n):
            ok(got, gold[f"c2p_{B}_{n}"].reshape(B, n, 2), f"mpiv_cam2pixel_chain B={B} n={n} against the reference")
        if not plain:
            ok(_raw("mpiv_cam2pixel", dev, (B, n, 2), c, p, B, n), want, f"mpiv_cam2pixel B={B} n={n}")


# ---------------------------------------------------------------------------
# transform_plane_imgs_torch: its sample coordinates and the sampled planes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("Ht,Wt", gen.PC)
def test_plane_imgs_dropin(Ht, Wt, gold, dev):
    tag = f"pc_{Ht}x{Wt}"
    imgs, pts = gen.pc_inputs(Ht, Wt, gold[tag + "_hom"])
    cams = [t.to(dev) for t in gen.pc_cameras(Ht, Wt)]
    hom = torch.tensor(gold[tag + "_hom"])  # the reference's (torch.inverse(k_t) inside: host-dependent bits)
    ok(_np(_lib.warp_planes(imgs.to(dev), pts.to(dev), hom.to(dev))), gold[tag + "_out"],
       f"transform_plane_imgs_torch {Ht}x{Wt} with the reference's homographies")
    mine = mv.inv_homography_torch(*cams)
    got = mv.transform_plane_imgs_torch(imgs.to(dev), pts.to(dev), *cams)
    ok(_np(got), _np(_lib.warp_planes(imgs.to(dev), pts.to(dev), mine)), f"transform_plane_imgs_torch {Ht}x{Wt}")
    if host_agrees(mine, gold[tag + "_hom"]):
        ok(_np(got), gold[tag + "_out"], f"transform_plane_imgs_torch {Ht}x{Wt} against the reference")


@pytest.mark.parametrize("Ht,Wt", gen.PC)
def test_plane_coords_entries(Ht, Wt, gold, dev):
    tag, n = f"pc_{Ht}x{Wt}", Ht * Wt
    hom = gold[tag + "_hom"]
    _, pts = gen.pc_inputs(Ht, Wt, hom)
    flat = pts.reshape(4, n, 3).contiguous()
    p, h = flat.to(dev), torch.tensor(hom).reshape(4, 9).to(dev)
    rule = gc.tp_plain(n, True)
    for plain in (False, True):
        want = gc.plane_coords(flat.numpy(), hom.reshape(4, 3, 3), Ht, Wt, plain)
        got = _raw("mpiv_plane_coords_chain", dev, (4, n, 2), p, 4, n, h, Ht, Wt, int(plain))
        ok(got, want, f"mpiv_plane_coords_chain {Ht}x{Wt} plain={plain}")
        if plain == rule:
            ok(got.reshape(2, 2, Ht, Wt, 2), gold[tag + "_coords"], f"plane coordinates {Ht}x{Wt} against the reference")
        if not plain:
            ok(_raw("mpiv_plane_coords", dev, (4, n, 2), p, 4, n, h, Ht, Wt), want, f"mpiv_plane_coords {Ht}x{Wt}")


# ---------------------------------------------------------------------------
# normalize_homogeneous_torch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k,n", gen.NH)
def test_normalize_homogeneous_dropin(k, n, gold, dev):
    tag = f"nh_{k}_{n}"
    pts = gen.nh_inputs(k, n)
    _, after = gc.normalize_homogeneous(pts.numpy())
    assert gen.sha(after) == gold["shas"][tag + "_after"]  # the reference's input after its call
    work = pts.to(dev)
    out = mv.normalize_homogeneous_torch(work)
    ok(_np(out), gold[tag + "_out"], tag)
    ok(_np(work), after, tag + ": the input after the call")
    ok(_np(work)[:, k], gold[tag + "_w"], tag + ": w after the call")


@pytest.mark.parametrize("k,n", gen.NH)
def test_normalize_homogeneous_through_a_view(k, n, gold, dev):
    """A non-contiguous input: the kernel runs on a dense copy, and the rewritten w column is copied back
    into the caller's view -- and nowhere else."""
    tag = f"nh_{k}_{n}"
    pts = gen.nh_inputs(k, n)
    _, after = gc.normalize_homogeneous(pts.numpy())
    base = torch.full((n, k + 4), 7.0, device=dev)
    view = base[:, 1:k + 2]
    view.copy_(pts.to(dev))
    assert not view.is_contiguous() or n == 1
    out = mv.normalize_homogeneous_torch(view)
    ok(_np(out), gold[tag + "_out"], tag + " through a view")
    ok(_np(view), after, tag + ": the view after the call")
    assert bool((base[:, 0] == 7).all()) and bool((base[:, k + 2:] == 7).all()), "written outside the view"


# ---------------------------------------------------------------------------
# the frame codecs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", gen.CODEC_N)
def test_codecs(n, gold, dev):
    pre, dep = gen.codec_inputs(n)
    ok(_np(mv.preprocess_image_torch(pre.to(dev))), gold[f"pre_{n}"], f"preprocess_image_torch n={n}")
    got = mv.deprocess_image_torch(dep.to(dev))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n,)
    bad = np.flatnonzero(_np(got) != gold[f"dep_{n}"])
    assert bad.size == 0, (f"deprocess_image_torch n={n}: {bad.size} bytes differ, first at {bad[0]}: input "
                           f"{float(dep[bad[0]])!r}, got {int(got[bad[0]])}, want {int(gold[f'dep_{n}'][bad[0]])}")
    assert np.array_equal(_np(got), gc.deprocess_u8(dep.numpy()))


# ---------------------------------------------------------------------------
# the fused kernels at the smallest frame inside their contract (5x9 = 45 pixels)
# ---------------------------------------------------------------------------

def test_fused_kernels_at_the_smallest_in_contract_frame(gold, dev):
    """The kernels fed the reference's homographies and K^-1 reproduce its frames on any host; the drop-ins,
    which invert K on this host, equal the oracle fed with this host's matrices, and the goldens wherever
    this host's LAPACK agrees with the golden host's."""
    from mpi_vision_amd import _host
    from oracle import oracle
    cpu = gen.boundary_inputs()
    b = {k: v.to(dev) for k, v in cpu.items()}
    homs = torch.tensor(np.ascontiguousarray(gold["bd_homs"].transpose(1, 0, 2, 3))).reshape(1, 5, 9)
    ok(_np(_lib.render(b["mpi"], homs.to(dev))), gold["bd_render"], "render 5x9x5, the reference's homographies")
    mine_h = _host.render_homographies(cpu["pose"], cpu["planes"], cpu["K"], 1)
    got = _np(mv.mpi_render_view_torch(b["mpi"], b["pose"], b["planes"], b["K"]))
    ok(got, oracle.render(cpu["mpi"].numpy(), mine_h.numpy()), "mpi_render_view_torch 5x9x5 against the oracle")
    if host_agrees(mine_h, _np(homs)):
        ok(got, gold["bd_render"], "mpi_render_view_torch 5x9x5 against the reference")

    mine_ki, proj = _host.psv_matrices(cpu["K2"], cpu["K2"], cpu["pose2"])
    ki = torch.tensor(gold["bd_ki"]).reshape(2, 9)
    ok(_np(_lib.inverse_warp_depthmap(b["img"], b["depth"], ki, proj, 5, 9)), gold["bd_warp"],
       "inverse warp 5x9, the reference's K^-1")
    ok(_np(_lib.plane_sweep(b["img"], gen.SWEEP_DEPTHS, ki, proj, 5, 9)), gold["bd_sweep"],
       "plane sweep 5x9, D = 3, the reference's K^-1")
    warp = _np(mv.projective_inverse_warp_torch(b["img"], b["depth"], b["pose2"], b["K2"]))
    sweep = _np(mv.plane_sweep_torch(b["img"], gen.SWEEP_DEPTHS, b["pose2"], b["K2"]))
    img = cpu["img"].numpy()
    ok(warp, oracle.inverse_warp(img, mine_ki.numpy(), proj.numpy(), cpu["depth"].numpy()),
       "projective_inverse_warp_torch 5x9 against the oracle")
    ok(sweep, oracle.plane_sweep(img, mine_ki.numpy(), proj.numpy(), gen.SWEEP_DEPTHS, 5, 9),
       "plane_sweep_torch 5x9 against the oracle")
    if host_agrees(mine_ki, gold["bd_ki"]):
        ok(warp, gold["bd_warp"], "projective_inverse_warp_torch 5x9 against the reference")
        ok(sweep, gold["bd_sweep"], "plane_sweep_torch 5x9, D = 3 against the reference")
