"""Side streams, HIP-graph capture and replay with new data, two streams and two threads.

A. Every stream-ordered entry point of include/mpiv.h (tests/stream_cases.py): eager on a side stream,
   captured there, replayed with other data -- bit for bit against the CPU oracle.
B. The Python layer's per-stream memos (K^-1, the float copy of a u8 / f16 MPI, the proj scratch, the
   uploaded depth list) under capture: nothing a replay reads or writes may belong to a memo that a
   later eager call frees, and a memo hit must not skip work whose input changes between replays.  The
   lifetime tests free the memo's block, take the same block again (the pointer is asserted) and fill
   it, so a graph that still used it would render garbage or overwrite the filler -- never a fault: the
   block stays allocated to this process throughout.
C. Eager ordering (a call enqueued before its input exists), two streams that share every memo key,
   two threads.

No test provokes a fault: every failure is a Python exception raised before a launch or a bit
comparison after a synchronisation."""
import threading

import numpy as np
import pytest
import torch

import lattice_cases as lc
import stream_cases as sc
from lattice_cases import match
from test_f16_gpu import _half_mpi
from test_lattice_gpu import SENT

pytestmark = pytest.mark.gpu

import mpi_vision_amd as mv  # noqa: E402
from mpi_vision_amd import _host, _lib, configs  # noqa: E402
from oracle import oracle  # noqa: E402

F32 = torch.float32


# ---------------------------------------------------------------------------
# A. every entry point
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_replay_follows_new_data(case, dev, kopts):
    if case.opts:
        kopts(**case.opts)
    sc.replay_case(case, dev)


# ---------------------------------------------------------------------------
# B. the memos under capture
# ---------------------------------------------------------------------------

RECLAIM_CAP = 4096


def reclaim(ptr, numel, dev, stream, fill):
    """Allocate float tensors of `numel` elements on `stream`, filled with `fill`, until one sits at
    `ptr` (a block freed on that stream goes back to that stream's free list).  Returns (all of them --
    keep them alive --, the one at ptr).  Not finding the block is a failure: the test would be vacuous."""
    keep = []
    with torch.cuda.stream(stream):
        for _ in range(RECLAIM_CAP):
            t = torch.full((numel,), fill, dtype=F32, device=dev)
            keep.append(t)
            if t.data_ptr() == ptr:
                return keep, t
    pytest.fail(f"the freed block at {ptr:#x} was not handed out again in {RECLAIM_CAP} allocations")


def cams(k, B, W=70, H=37):
    """(pose [B,4,4], K [B,3,3]) of data set k, CPU."""
    f = configs.focal_from_fov(W) * (1 + 0.1 * k)
    K = configs.f32([configs.intrinsics_matrix(f + b, 1.1 * f, W / 2.0, H / 2.0 + k) for b in range(B)])
    pose = configs.f32([configs.pose_from(configs.rot_y((1 - 2 * k) * 2.0 * (b + 1)),
                                          (0.03 * (b + 1), -0.02 * k, 0.01 * b)) for b in range(B)])
    return pose, K


def want_render(mpi, pose, planes, K):
    """The oracle's frames through the reference's own homography chain (op by op, torch CPU)."""
    B = pose.shape[0]
    homs = _host.render_homographies_torch(pose, planes, K, B)
    return oracle.render(mpi.numpy(), homs.numpy())


def want_psv(img, pose, K, depths):
    ki, proj = _host.psv_matrices(K, K, pose)
    return oracle.plane_sweep(img.numpy(), ki.numpy(), proj.numpy(), [float(d) for d in depths], img.shape[1],
                              img.shape[2])


def test_captured_render_does_not_read_the_kinv_memo(dev):
    """An eager call on another stream replaces the memoised inverse(K); its block is taken again and
    filled with NaN; the replay still renders with the captured K -- also after K is updated in place
    (the intrinsics are a constant of the captured graph: INTEGRATION.md)."""
    B, H, W, P = 2, 37, 70, 11
    A, S, T = (torch.cuda.Stream(dev) for _ in range(3))
    planes = configs.f32(configs.inv_depths(1, 100, P))
    mpis = [torch.stack([lc.finite_mpi(H, W, P, seed=10 * k + b) for b in range(B)]) for k in range(3)]
    poses = [cams(k, B)[0] for k in range(2)] + [cams(0, B)[0].flip(0).contiguous()]
    Kc = cams(0, B)[1]
    K, planes_d = Kc.to(dev), planes.to(dev)
    mpi_s, pose_s = mpis[0].to(dev), poses[0].to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        mv.mpi_render_view_torch(mpi_s, pose_s, planes_d, K)  # the warm-up: inverse(K) memoised on stream A
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        out = mv.mpi_render_view_torch(mpi_s, pose_s, planes_d, K)
    old = _host._KINV_DEV[(id(K), False)][3]
    ptr, numel = old.data_ptr(), old.numel()
    del old
    with torch.cuda.stream(T):
        mv.mpi_render_view_torch(mpi_s, pose_s, planes_d, K)  # another stream: the entry is replaced
    torch.cuda.synchronize()
    assert _host._KINV_DEV[(id(K), False)][3].data_ptr() != ptr
    keep, hit = reclaim(ptr, numel, dev, A, float("nan"))
    torch.cuda.synchronize()
    assert hit.data_ptr() == ptr
    for k in (1, 2):
        if k == 2:
            K.mul_(1.5)  # in place: the graph keeps the K it was captured with
        mpi_s.copy_(mpis[k])
        pose_s.copy_(poses[k])
        out.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        match(out, want_render(mpis[k], poses[k], planes, Kc), f"replay {k}")
        assert bool(torch.isnan(hit).all()), "the replay wrote into the block the memo had freed"
    del g, keep


@pytest.mark.parametrize("warm", ["same_stream", "other_stream"])
@pytest.mark.parametrize("fmt", ["u8", "f16"])
def test_captured_float_route_converts_on_every_replay(fmt, warm, dev):
    """render_packed_u8 / _f16 at 40 views (the float-copy route): after the packed buffer is refilled
    with another MPI the replay renders that MPI, whether the warm-up filled the memo on the capture
    stream or on another one."""
    H, W, P, V = 37, 70, 5, 40
    assert V >= _lib.U8_FLOAT_MIN_VIEWS and V >= _lib.F16_FLOAT_MIN_VIEWS
    if fmt == "u8":
        hosts = [sc._u8_mpi(k, H, W, P) for k in range(2)]
        floats = [sc._u8_float(k, H, W, P) for k in range(2)]
        pack, render = _lib.pack_planes_u8, _lib.render_packed_u8
    else:
        hosts = [torch.from_numpy(_half_mpi(H, W, P, 70 + k)) for k in range(2)]
        floats = [h.numpy().astype(np.float32) for h in hosts]
        pack, render = _lib.pack_planes_f16, _lib.render_packed_f16
    homs = sc.cam_homs(0, V, P, H, W)
    S, O = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    pk, homs_d = pack(hosts[0].to(dev)), homs.to(dev)
    out = torch.full((V, H, W, 3), SENT, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(S if warm == "same_stream" else O):
        render(pk, homs_d, out=out)
    torch.cuda.synchronize()
    match(out, oracle.render(sc._bcast(floats[0], V), homs.numpy()), "warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        render(pk, homs_d, out=out)
    for k in (1, 0, 1):
        pack(hosts[k].to(dev), out=pk)
        out.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        match(out, oracle.render(sc._bcast(floats[k], V), homs.numpy()), f"replay with MPI {k + 1}")
    del g
    _lib.clear_float_copies()


def _sweep_inputs(k, B, H=24, W=32, C=3):
    g = torch.Generator().manual_seed(300 + k)
    img = torch.rand((B, H, W, C), generator=g)
    pose, K = cams(k, B, W, H)
    return img, pose, K


def test_captured_sweep_does_not_write_the_proj_scratch_memo(dev):
    """An eager call with a larger batch replaces (frees) the per-stream proj scratch; its block is
    taken again by sentinel tensors; the replay leaves them alone and sweeps the new image."""
    B, D = 2, 4
    S = torch.cuda.Stream(dev)
    depths = configs.f32(configs.inv_depths(1, 50, D))
    data = [_sweep_inputs(k, B) for k in range(2)]
    Kc = data[0][2]
    img_s, pose_s, K, depths_d = data[0][0].to(dev), data[0][1].to(dev), Kc.to(dev), depths.to(dev)
    big = [t.to(dev) for t in _sweep_inputs(0, 16)]
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        mv.plane_sweep_torch(img_s, depths_d, pose_s, K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        out = mv.plane_sweep_torch(img_s, depths_d, pose_s, K)
    old = _lib._PROJ_SCRATCH[(dev.index, S.cuda_stream)]
    ptr, numel = old.data_ptr(), old.numel()
    del old
    with torch.cuda.stream(S):
        mv.plane_sweep_torch(big[0], depths_d, big[1], big[2])  # 16 poses: a larger scratch replaces the old one
    torch.cuda.synchronize()
    assert _lib._PROJ_SCRATCH[(dev.index, S.cuda_stream)].data_ptr() != ptr
    keep, hit = reclaim(ptr, numel, dev, S, SENT)
    torch.cuda.synchronize()
    assert hit.data_ptr() == ptr
    img_s.copy_(data[1][0])
    pose_s.copy_(data[1][1])
    out.fill_(SENT)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    match(out, want_psv(data[1][0], data[1][1], Kc, depths), "replay")
    assert all(bool((t == SENT).all()) for t in keep), "the replay wrote into the block the scratch memo had freed"
    del g, keep


@pytest.mark.parametrize("warm", ["same_stream", "other_stream"])
def test_captured_sweep_does_not_read_the_depth_list_memo(warm, dev):
    """plane_sweep_torch with a Python list of depths: 64 other lists evict (free) the uploaded copy;
    its block is taken again and filled with NaN; the replay still sweeps at the captured depths."""
    B = 2
    depths = [1.0 + 0.37 * i for i in range(5)] + [12.5 if warm == "same_stream" else 13.5]
    S, O = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    W_ = S if warm == "same_stream" else O
    data = [_sweep_inputs(k, B) for k in range(2)]
    Kc = data[0][2]
    img_s, pose_s, K = data[0][0].to(dev), data[0][1].to(dev), Kc.to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(W_):
        mv.plane_sweep_torch(img_s, depths, pose_s, K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        out = mv.plane_sweep_torch(img_s, depths, pose_s, K)
    key = (tuple(depths), dev.index, W_.cuda_stream)
    old = _lib._DEPTHS_DEV[key]
    ptr, numel = old.data_ptr(), old.numel()
    del old
    # (on the default stream: the 64 uploads come from that stream's blocks, so none of them takes the
    # block the eviction hands back to the warm-up stream)
    for i in range(64):
        _lib._depths_on([100.0 + i, 200.0 + i, 3.0, 4.0, 5.0, 6.0], dev)
    torch.cuda.synchronize()
    assert key not in _lib._DEPTHS_DEV, "the eviction did not run"
    keep, hit = reclaim(ptr, numel, dev, W_, float("nan"))
    torch.cuda.synchronize()
    assert hit.data_ptr() == ptr
    img_s.copy_(data[1][0])
    pose_s.copy_(data[1][1])
    out.fill_(SENT)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    match(out, want_psv(data[1][0], data[1][1], Kc, depths), "replay")
    assert bool(torch.isnan(hit).all())
    del g, keep


def _no_launch(monkeypatch):
    def refuse(name, *a):
        raise AssertionError(f"{name} was called: the error must be raised before any launch")
    monkeypatch.setattr(_lib, "_call", refuse)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)


def test_depth_list_without_warm_up_raises_under_capture(dev, monkeypatch):
    """Under capture, a depth list that no warm-up uploaded raises -- before any HIP call -- and tells
    the caller to warm up or to pass a device tensor; so does the whole drop-in without a warm-up."""
    img, pose, K = (t.to(dev) for t in _sweep_inputs(0, 2))
    torch.cuda.synchronize()
    _no_launch(monkeypatch)
    with pytest.raises(RuntimeError, match="warm-up.*device tensor"):
        _lib._depths_on([0.123, 4.5, 67.0], dev)
    with pytest.raises(RuntimeError, match="warm-up"):
        mv.plane_sweep_torch(img, [0.123, 4.5, 67.0], pose, K)


def test_host_matrices_raise_under_capture(dev, monkeypatch):
    """CPU poses / homographies cannot be part of a captured graph (their upload would read a temporary
    host buffer on every replay): a RuntimeError that names the argument, nothing launched, `out`
    untouched."""
    B, H, W, P = 2, 37, 70, 11
    mpi = torch.stack([lc.finite_mpi(H, W, P, seed=b) for b in range(B)]).to(dev)
    pose, K = cams(0, B)
    planes = configs.f32(configs.inv_depths(1, 100, P))
    packed = sc.pack_host(lc.finite_mpi(H, W, P)).to(dev)
    homs = sc.cam_homs(0, B, P, H, W)
    out = torch.full((B, H, W, 3), SENT, device=dev)
    torch.cuda.synchronize()
    _no_launch(monkeypatch)
    with pytest.raises(RuntimeError, match="tgt_pose"):
        mv.mpi_render_view_torch(mpi, pose, planes, K)
    for h in (homs, homs.pin_memory()):
        with pytest.raises(RuntimeError, match="homs"):
            _lib.render_packed(packed, h, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_fused_training_step_graphed_with_new_data_each_replay(dev):
    """mpi_render_net_output_torch under torch.cuda.make_graphed_callables: three steps with three
    different predictions / reference images; frames, d mpi_pred and d ref_img equal the oracle's
    assembly -> render / render backward -> assembly backward each time."""
    B, H, W, P = 1, 33, 47, 17
    pose, Kc = cams(0, B, W, H)
    planes = configs.f32(configs.inv_depths(1, 100, P))
    pose_d, K, planes_d = pose.to(dev), Kc.to(dev), planes.to(dev)
    homs = _host.render_homographies_torch(pose, planes, Kc, B).numpy()

    def data(k):
        g = torch.Generator().manual_seed(900 + k)
        return (torch.rand((B, 2 * P + 3, H, W), generator=g) * 2 - 1, torch.rand((B, H, W, 3), generator=g) * 2 - 1,
                torch.rand((B, H, W, 3), generator=g) * 2 - 1)

    def step(pred, ref):
        return mv.mpi_render_net_output_torch(pred, ref, pose_d, planes_d, K)
    sample = tuple(t.to(dev).requires_grad_(True) for t in data(0)[:2])
    graphed = torch.cuda.make_graphed_callables(step, sample)
    for k in (1, 2, 3):
        pred, ref, dout = data(k)
        pd, rd = pred.to(dev).requires_grad_(True), ref.to(dev).requires_grad_(True)
        out = graphed(pd, rd)
        out.backward(dout.to(dev))
        torch.cuda.synchronize()
        rgba = oracle.assemble_mpi(pred.numpy(), ref.numpy(), P)
        drgba = oracle.render_backward(rgba, homs, dout.numpy())
        match(out.detach(), oracle.render(rgba, homs), f"step {k}: frames")
        match(pd.grad, oracle.assemble_mpi_backward(drgba, pred.numpy(), ref.numpy(), P), f"step {k}: d mpi_pred")
        match(rd.grad, oracle.assemble_mpi_backward_fg(drgba, pred.numpy(), P), f"step {k}: d ref_img")


# ---------------------------------------------------------------------------
# C. eager ordering and re-entrancy
# ---------------------------------------------------------------------------

def _case(prefix):
    return next(c for c in sc.CASES if c.name.startswith(prefix))


STALE = {
    "render_packed": ("render_packed-64x66x16", "out", lambda b: _lib.render_packed(b["packed"], b["homs"])),
    "render_backward": ("render_backward-folded", "grad_null",
                        lambda b: _lib.render_backward(b["mpi"], b["homs"], b["dout"])),
    "plane_sweep": ("plane_sweep-C3-D10", "out",
                    lambda b: _lib.plane_sweep(b["img"], b["depths"], b["ki"], b["proj"], sc.SHT, sc.SWT)),
    "plane_sweep_pose": ("plane_sweep_pose-C3-D10", "out",
                         lambda b: _lib.plane_sweep_pose(b["img"], b["depths"], b["ki"], b["Ks"], b["pose"], sc.SHT,
                                                         sc.SWT)),
    "render_net_output": ("render_net_output-", "out",
                          lambda b: _lib.render_net_output(b["pred"], b["fg"], sc.AP, b["homs"])),
    "render_packed_f16": ("render_packed_f16-64x66x16", "out",
                          lambda b: _lib.render_packed_f16(b["packed"], b["homs"])),
}
_SLEEP = {}


def sleep_cycles(dev, ms=50.0):
    """torch.cuda._sleep cycles for about `ms` milliseconds, from one timed _sleep(10**7)."""
    if "c" not in _SLEEP:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(10 ** 7)
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        _SLEEP["c"] = int(10 ** 7 * ms / max(t, 1e-3))
        print(f"_sleep(1e7) took {t:.3f} ms -> {_SLEEP['c']} cycles for ~{ms} ms")
    return _SLEEP["c"]


@pytest.mark.parametrize("name", list(STALE))
def test_call_enqueued_before_its_input_exists(name, dev):
    """The wrapper is enqueued on stream s behind a copy that waits for a ~50 ms sleep on stream t: it
    returns while the sleep still runs (asserted -- else the test proves nothing) and, once everything has
    run, its result is that of the data copied in, not of the data the buffers held at the call."""
    prefix, key, fn = STALE[name]
    case = _case(prefix)
    c = sleep_cycles(dev)
    s, t = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    b = {n: x.to(dev) for n, x in case.inputs(0).items()}
    new = {n: x.to(dev) for n, x in case.inputs(1).items()}
    want = case.want(1)[key]
    with torch.cuda.stream(s):
        fn(b)  # the per-device lazy state, module loading: not part of the timed window
    torch.cuda.synchronize()
    e = torch.cuda.Event()
    with torch.cuda.stream(t):
        torch.cuda._sleep(c)
        e.record()
    with torch.cuda.stream(s):
        s.wait_event(e)
        for n in b:
            b[n].copy_(new[n], non_blocking=True)
        got = fn(b)
    pending = not e.query()
    torch.cuda.synchronize()
    assert pending, "the sleep had ended before the call returned: the call was not shown to run ahead of its input"
    match(got, want, name)


def test_two_streams_share_every_memo_key(dev):
    """Streams s1 and s2 alternate for eight rounds without synchronising: the same intrinsics tensor,
    the same depth list and the same packed f16 MPI (40 views: the float-copy route), different poses
    and outputs.  Every memo entry is replaced on every call; every output equals the oracle's."""
    B, V, H, W, P = 2, 40, 37, 70, 5
    depths = [1.0, 1.7, 2.9, 5.1, 9.3, 17.0, 33.0]
    half = _half_mpi(H, W, P, 81)
    pk = _lib.pack_planes_f16(torch.from_numpy(half).to(dev))
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    Kc = cams(0, B, 32, 24)[1]
    K = Kc.to(dev)
    img = _sweep_inputs(0, B)[0]
    img_d = img.to(dev)
    poses = [cams(k, B, 32, 24)[0] for k in range(2)]
    homs = [sc.cam_homs(k, V, P, H, W) for k in range(2)]
    poses_d, homs_d = [p.to(dev) for p in poses], [h.to(dev) for h in homs]
    torch.cuda.synchronize()
    outs = [[], []]
    for _ in range(8):
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                outs[i].append((mv.plane_sweep_torch(img_d, depths, poses_d[i], K),
                                _lib.render_packed_f16(pk, homs_d[i])))
    torch.cuda.synchronize()
    for i in range(2):
        psv = want_psv(img, poses[i], Kc, depths)
        frames = oracle.render(sc._bcast(half.astype(np.float32), V), homs[i].numpy())
        for r, (a, b) in enumerate(outs[i]):
            match(a, psv, f"stream {i + 1}, round {r}: plane sweep")
            match(b, frames, f"stream {i + 1}, round {r}: f16 render")
    _lib.clear_float_copies()


def test_two_threads_two_streams(dev, kopts):
    """Two Python threads, each with its own stream and problem (render_backward through the bucket
    fallback, plane_sweep at 10 depths), four calls each; then a failing call in one thread leaves the
    other thread's mpiv_last_error() as it was."""
    kopts(bwd_fallback=1)
    bc, pc = _case("render_backward-fallback"), _case("plane_sweep-C3-D10")
    bi = {n: x.to(dev) for n, x in bc.inputs(0).items()}
    pi = {n: x.to(dev) for n, x in pc.inputs(1).items()}
    _lib.render_backward(bi["mpi"], bi["homs"], bi["dout"])  # lazy per-device state, before the threads start
    torch.cuda.synchronize()
    res, errs = {"bwd": [], "psv": []}, []

    def run(key, fn):
        try:
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                for _ in range(4):
                    res[key].append(fn())
            s.synchronize()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((key, e))
    ths = [threading.Thread(target=run, args=("bwd", lambda: _lib.render_backward(bi["mpi"], bi["homs"], bi["dout"]))),
           threading.Thread(target=run, args=("psv", lambda: _lib.plane_sweep(pi["img"], pi["depths"], pi["ki"],
                                                                              pi["proj"], sc.SHT, sc.SWT)))]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths), "a thread did not finish"
    assert not errs, errs
    torch.cuda.synchronize()
    for got in res["bwd"]:
        match(got, bc.want(0)["grad_null"], "render_backward in a thread")
    for got in res["psv"]:
        match(got, pc.want(1)["out"], "plane_sweep in a thread")
    _lib.render_backward_raise_pending(dev)

    # mpiv_last_error() is per thread
    L = _lib.load()
    seen, failed, go, done = [], [], threading.Event(), threading.Event()

    def reader():
        seen.append(L.mpiv_last_error())
        go.set()
        if done.wait(timeout=60):
            seen.append(L.mpiv_last_error())

    def failing():
        if go.wait(timeout=60):
            try:
                _lib._call("mpiv_combine_ct", bi["dout"], 0, 0, bi["dout"], _lib._stream(dev))  # G = 0: refused
            except RuntimeError as e:
                failed.append(str(e))
        done.set()
    ths = [threading.Thread(target=reader), threading.Thread(target=failing)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ths)
    assert failed and "bad shape" in failed[0]
    assert len(seen) == 2 and seen[0] == seen[1], f"another thread's failure changed mpiv_last_error(): {seen}"
