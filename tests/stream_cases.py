"""Every stream-ordered entry point of include/mpiv.h on a side stream and in a captured HIP graph that
is replayed with other data (tests/test_streams_gpu.py; the table itself is checked on the CPU by
tests/test_stream_cases.py).

A plain module: no fixtures, nothing collected by pytest.

A Case holds two input data sets of one shape (different seeds: texels, every matrix, depth list and
incoming gradient differ), the static device buffers, the raw `_lib._call(...)` closure on those buffers
and the expected outputs of each data set -- from the CPU oracle where it has the operation, else from
the reference's golden outputs (tests/golden/small.npz) or plain torch-CPU ops; never from the code under
test.  replay_case() runs the closure eagerly on a side stream, captures it there, and replays the graph
with data sets 2, 1, 2 copied into the static inputs."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

import lattice_cases as lc
from lattice_cases import match
from mpi_vision_amd import _host, _lib, configs
from oracle import oracle
from test_f16_gpu import _half_mpi
from test_lattice_gpu import SENT

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = torch.float32
BYTE = 0x5A  # the prefill of outputs that are not float32 (int32 0x5A5A5A5A, half 203.25, uint8 90)

EXCLUDED = {
    "mpiv_render_backward_status": "synchronises by contract",
    "mpiv_route": "host-only, no stream",
    "mpiv_tile_order": "host-only, no stream",
    "mpiv_render_homographies": "host-only, no stream",
    "mpiv_psv_proj": "host-only, no stream",
    "mpiv_mark": "diagnostics",
    "mpiv_probe_gather": "diagnostics",
    "mpiv_selftest_div_const": "diagnostics",
    "mpiv_selftest_tickets": "diagnostics",
    "mpiv_render_packed_lds": "A/B library only",
}
COVERED = set(_lib._SIGS) - set(EXCLUDED)

CASES: list = []


class Case:
    """name: the test id; entries: the ABI names the closure calls; inputs(k) -> {name: CPU tensor} of
    data set k (0 or 1); outputs: {name: (shape, dtype[, prefill])}; state: {name: bytes or callable ->
    bytes} zeroed uint8 buffers that are never refilled (workspaces, counters); call(b, dev): the closure
    on the buffer dict b; want(k) -> {output name: expected array, or a function (got tensor, b) that
    asserts}; prepare(b, dev): device-side setup before the first call (pointer tables); opts: debug
    options of the production library the case runs under; after(b): a check after every call."""

    def __init__(self, name, entries, inputs, outputs, call, want, state=None, prepare=None, opts=None, after=None):
        self.name, self.entries = name, tuple(entries)
        self.inputs, self.want = functools.lru_cache(maxsize=None)(inputs), functools.lru_cache(maxsize=None)(want)
        self.outputs, self.call, self.state = outputs, call, state or {}
        self.prepare, self.opts, self.after = prepare, opts or {}, after
        CASES.append(self)


def _prefill(t, fill=None):
    if fill is not None:
        t.fill_(fill)
    elif t.dtype == F32:
        t.fill_(SENT)
    else:
        t.view(torch.uint8).fill_(BYTE)


def _compare(case, b, k, what):
    for name, want in case.want(k).items():
        got = b[name]
        label = f"{case.name}: {name}, {what}"
        if callable(want):
            want(got, b, label)
        elif got.dtype == F32:
            match(got, want, label)
        else:
            g = got.detach().cpu().contiguous().numpy()
            assert g.shape == want.shape and g.tobytes() == np.ascontiguousarray(want).tobytes(), label
    if case.after is not None:
        case.after(b)


def replay_case(case, dev):
    """Side-stream eager call, capture on that stream, three replays with data sets 2, 1, 2.  The
    debug options of case.opts must be set by the caller (the kopts fixture).  No retry: any exception
    ends the test."""
    side = torch.cuda.Stream(dev)
    data = [case.inputs(0), case.inputs(1)]
    b = {n: t.to(dev) for n, t in data[0].items()}
    for n, spec in case.outputs.items():
        b[n] = torch.empty(spec[0], dtype=spec[1], device=dev)
    for n, nbytes in case.state.items():
        b[n] = torch.zeros(nbytes() if callable(nbytes) else nbytes, dtype=torch.uint8, device=dev)
    if case.prepare is not None:
        case.prepare(b, dev)

    def refill():
        for n, spec in case.outputs.items():
            _prefill(b[n], spec[2] if len(spec) > 2 else None)
        torch.cuda.synchronize()

    refill()
    with torch.cuda.stream(side):
        case.call(b, dev)  # the warm-up of the per-device lazy state, and the side-stream eager check
    torch.cuda.synchronize()
    _compare(case, b, 0, "eager on a side stream")
    refill()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        case.call(b, dev)
    for k in (1, 0, 1):
        for n, t in data[k].items():
            b[n].copy_(t)
        refill()
        g.replay()
        torch.cuda.synchronize()
        _compare(case, b, k, f"replay with data set {k + 1}")
    torch.cuda.synchronize()  # every static buffer (b) is still referenced here
    del g


# ---------------------------------------------------------------------------
# shared data
# ---------------------------------------------------------------------------

def S(dev):
    return _lib._stream(dev)


def _st(t, dims=None):
    return _lib._strides(t, dims)


def pack_host(m):
    """[H, W, P, C] -> the packed layout [P, H+4, W+4, C] with its zero border (include/mpiv.h)."""
    m = torch.as_tensor(m)
    H, W, P, C = m.shape
    out = torch.zeros((P, H + 4, W + 4, C), dtype=m.dtype)
    out[:, 2:2 + H, 2:2 + W] = m.permute(2, 0, 1, 3)
    return out


@functools.lru_cache(maxsize=None)
def cam_homs(k, V, P, H, W):
    """[V, P, 9] homographies of a small camera sweep, from the host chain (the reference's ops):
    the two data sets differ in the poses, the intrinsics and the plane depths."""
    f = configs.focal_from_fov(W) * (1.0 + 0.07 * k)
    K = configs.f32([configs.intrinsics_matrix(f, 1.1 * f, W / 2.0 + k, H / 2.0 - k)])
    sign = 1.0 if k == 0 else -0.8
    poses = configs.f32([configs.pose_from(configs.rot_y(sign * 1.5 * (v + 1)),
                                           (sign * 0.03 * (v + 1), 0.01 * v - 0.02 * k, 0.02 * k * v))
                         for v in range(V)])
    depths = configs.f32(configs.inv_depths(1.0 + 0.5 * k, 100.0 - 30.0 * k, P))
    return _host.render_homographies(poses, depths, K, V).clone()


def _bcast(m, V):
    m = m.numpy() if isinstance(m, torch.Tensor) else m
    return np.broadcast_to(m[None], (V,) + m.shape)


PACKED_SHAPES = [(64, 66, 16), (37, 203, 7)]
VP = 7


def _route(entry, *args):
    try:
        return _lib.route(entry, *args)[0].split("(")[0].split("<")[0].replace("void ", "").strip()
    except (RuntimeError, OSError):
        return "?"


# ---------------------------------------------------------------------------
# packed float render, (C, T) partials, row bands, combine, pack
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pk_mpi(k, H, W, P):
    return lc.finite_mpi(H, W, P, seed=k)


@functools.lru_cache(maxsize=None)
def _pk_ct(k, H, W, P, a, b_):
    return oracle.render_ct(_bcast(_pk_mpi(k, H, W, P), VP), cam_homs(k, VP, P, H, W).numpy(), a, b_, back=(a == 0))


def _rows_check(want, y0, y1):
    def check(got, b, label):
        match(got[:, y0:y1], want[:, y0:y1], label)
        assert bool((got[:, :y0] == SENT).all()) and bool((got[:, y1:] == SENT).all()), label + ": other rows touched"
    return check


def _packed_cases(H, W, P):
    V, tag = VP, f"{H}x{W}x{P}"
    ranges = ((0, P // 3), (P // 3, P), (1, P))

    def inputs(k):
        m = _pk_mpi(k, H, W, P)
        return {"packed": pack_host(m), "homs": cam_homs(k, V, P, H, W)}

    def frames(k):
        return oracle.render(_bcast(_pk_mpi(k, H, W, P), V), cam_homs(k, V, P, H, W).numpy())

    Case(f"pack_planes-{tag}", ["mpiv_pack_planes"], lambda k: {"mpi": _pk_mpi(k, H, W, P)},
         {"out": ((P, H + 4, W + 4, 4), F32)},
         lambda b, d: _lib._call("mpiv_pack_planes", b["mpi"], _st(b["mpi"]), H, W, P, b["out"], S(d)),
         lambda k: {"out": pack_host(_pk_mpi(k, H, W, P)).numpy()})
    Case(f"render_packed-{tag}-{_route('render_packed', H, W, P, V)}", ["mpiv_render_packed"], inputs,
         {"out": ((V, H, W, 3), F32)},
         lambda b, d: _lib._call("mpiv_render_packed", b["packed"], H, W, P, b["homs"], V, b["out"], S(d)),
         lambda k: {"out": frames(k)})
    if "render_rows" in _route("render_packed", H, W, P, V):  # (the counting build exists for the rows kernel only)
        Case(f"render_packed_census-{tag}", ["mpiv_render_packed_census"], inputs, {"out": ((V, H, W, 3), F32)},
             lambda b, d: _lib._call("mpiv_render_packed_census", b["packed"], H, W, P, b["homs"], V, b["out"],
                                     b["n"], S(d)),
             lambda k: {"out": frames(k)}, state={"n": 8})

    def call_ct(b, d):
        for i, (p0, p1) in enumerate(ranges):
            _lib._call("mpiv_render_packed_ct", b["packed"], H, W, P, p0, p1, int(p0 == 0), b["homs"], V, b[f"ct{i}"],
                       S(d))
    Case(f"render_packed_ct-{tag}-{_route('render_packed_ct', H, W, P, V)}", ["mpiv_render_packed_ct"], inputs,
         {f"ct{i}": ((V, H, W, 4), F32) for i in range(3)}, call_ct,
         lambda k: {f"ct{i}": _pk_ct(k, H, W, P, a, b_) for i, (a, b_) in enumerate(ranges)})
    Case(f"render_packed_ct_rows-{tag}-{_route('render_packed_ct_rows', H, W, P, V, 5, H - 7)}",
         ["mpiv_render_packed_ct_rows"], inputs, {"band": ((V, H, W, 4), F32)},
         lambda b, d: _lib._call("mpiv_render_packed_ct_rows", b["packed"], H, W, P, P // 3, P, 0, b["homs"], V, 5,
                                 H - 7, b["band"], S(d)),
         lambda k: {"band": _rows_check(_pk_ct(k, H, W, P, P // 3, P), 5, H - 7)})

    def parts(k):
        return np.stack([_pk_ct(k, H, W, P, 0, P // 3), _pk_ct(k, H, W, P, P // 3, P)])
    Case(f"combine_ct-{tag}", ["mpiv_combine_ct"], lambda k: {"parts": torch.from_numpy(parts(k))},
         {"out": ((V, H, W, 3), F32)},
         lambda b, d: _lib._call("mpiv_combine_ct", b["parts"], 2, V * H * W, b["out"], S(d)),
         lambda k: {"out": oracle.combine_ct(parts(k))})


for _s in PACKED_SHAPES:
    _packed_cases(*_s)


# ---------------------------------------------------------------------------
# in-place layout: render, render_train, render_backward[_watched]
# ---------------------------------------------------------------------------

NB, NH, NW = 2, 37, 70


@functools.lru_cache(maxsize=None)
def _nat_mpi(k, P):
    return torch.stack([lc.finite_mpi(NH, NW, P, seed=10 * k + v) for v in range(NB)])


@functools.lru_cache(maxsize=None)
def _nat_frames(k, P, p_end=None):
    h, m = cam_homs(k, NB, P, NH, NW).numpy(), _nat_mpi(k, P).numpy()
    if p_end is not None:
        h, m = np.ascontiguousarray(h[:, :p_end]), m[:, :, :, :p_end]
    return oracle.render(m, h)


def _ckpt_check(k, P):
    def check(got, b, label):
        for c in range(1, (P + 7) // 8):
            match(got[:, c, :, :, :3], _nat_frames(k, P, 8 * c), f"{label}, slot {c}")
            assert bool((got[:, c, :, :, 3].view(torch.int32) == 0).all()), label + ": checkpoint channel 3 is +0"
    return check


def _native_cases():
    P = 11

    def call_render(b, d):
        _lib._call("mpiv_render", b["mpi"], _st(b["mpi"]), NB, NH, NW, P, b["homs"], b["out"], S(d))
    Case(f"render-contiguous-{_route('render', NB, NH, NW, P)}", ["mpiv_render"],
         lambda k: {"mpi": _nat_mpi(k, P), "homs": cam_homs(k, NB, P, NH, NW)}, {"out": ((NB, NH, NW, 3), F32)},
         call_render, lambda k: {"out": _nat_frames(k, P)})

    def permuted(k):  # planes not contiguous per pixel (strides[3] == 1, strides[4] == P): the gather kernel
        m = _nat_mpi(k, P).permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)
        assert m.stride(3) != 4
        return {"mpi": m, "homs": cam_homs(k, NB, P, NH, NW)}
    Case("render-permuted-gather", ["mpiv_render"], permuted, {"out": ((NB, NH, NW, 3), F32)}, call_render,
         lambda k: {"out": _nat_frames(k, P)})
    for P2 in (11, 19):
        Case(f"render_train-P{P2}", ["mpiv_render_train"],
             lambda k, P2=P2: {"mpi": _nat_mpi(k, P2), "homs": cam_homs(k, NB, P2, NH, NW)},
             {"out": ((NB, NH, NW, 3), F32), "ckpt": ((NB, (P2 + 7) // 8, NH, NW, 4), F32)},
             lambda b, d, P2=P2: _lib._call("mpiv_render_train", b["mpi"], _st(b["mpi"]), NB, NH, NW, P2, b["homs"],
                                            b["out"], b["ckpt"], S(d)),
             lambda k, P2=P2: {"out": _nat_frames(k, P2), "ckpt": _ckpt_check(k, P2)})


_native_cases()

BP = 19
BWD_MODES = {"folded": {}, "fallback": {"bwd_fallback": 1}, "miss": {"bwd_margin": -96}, "group8": {"bwd_group": 8}}


def _ws_bytes(H, W, P):
    return lambda: _lib.load().mpiv_render_backward_workspace_size(H, W, P)


def _no_abort(H, W, P, names=("ws",)):
    def after(b):
        off = _lib.bwd_flag_offset(H, W, P)
        for n in names:
            words = b[n][off:off + 20].view(torch.int32).tolist()
            assert words[3] == 0 and words[4] == 0, f"abort words of {n}: {words}"
    return after


@functools.lru_cache(maxsize=None)
def _bwd_want(k):
    return oracle.render_backward(_nat_mpi(k, BP).numpy(), cam_homs(k, NB, BP, NH, NW).numpy(),
                                  lc.dout_for((NB, NH, NW, 3), seed=k).numpy())


def _backward_cases():
    for entry in ("mpiv_render_backward", "mpiv_render_backward_watched"):
        for mode, opts in BWD_MODES.items():
            def call(b, d, entry=entry):
                # the forward's checkpoints, the backward that takes them, and the one that recomputes
                # (ckpt = NULL), one after the other on the same workspace
                _lib._call("mpiv_render_train", b["mpi"], _st(b["mpi"]), NB, NH, NW, BP, b["homs"], b["out"],
                           b["ckpt"], S(d))
                _lib._call(entry, b["mpi"], _st(b["mpi"]), NB, NH, NW, BP, b["homs"], b["dout"], b["ckpt"],
                           b["grad_ckpt"], b["ws"], b["ws"].numel(), S(d))
                _lib._call(entry, b["mpi"], _st(b["mpi"]), NB, NH, NW, BP, b["homs"], b["dout"], None,
                           b["grad_null"], b["ws"], b["ws"].numel(), S(d))
            Case(f"{entry[5:]}-{mode}", [entry, "mpiv_render_train"],
                 lambda k: {"mpi": _nat_mpi(k, BP), "homs": cam_homs(k, NB, BP, NH, NW),
                            "dout": lc.dout_for((NB, NH, NW, 3), seed=k)},
                 {"out": ((NB, NH, NW, 3), F32), "ckpt": ((NB, (BP + 7) // 8, NH, NW, 4), F32),
                  "grad_ckpt": ((NB, NH, NW, BP, 4), F32), "grad_null": ((NB, NH, NW, BP, 4), F32)},
                 call, lambda k: {"out": _nat_frames(k, BP), "grad_ckpt": _bwd_want(k), "grad_null": _bwd_want(k)},
                 state={"ws": _ws_bytes(NH, NW, BP)}, opts=opts, after=_no_abort(NH, NW, BP))


_backward_cases()


# ---------------------------------------------------------------------------
# assembly from the network output, fused net-output render
# ---------------------------------------------------------------------------

AP = 11


@functools.lru_cache(maxsize=None)
def _net(k):
    g = torch.Generator().manual_seed(4400 + k)
    pred = torch.rand((NB, 2 * AP + 3, NH, NW), generator=g) * 2 - 1
    fg = torch.rand((NB, NH, NW, 3), generator=g) * 2 - 1
    drgba = torch.rand((NB, NH, NW, AP, 4), generator=g) * 2 - 1
    return pred, fg, drgba, oracle.assemble_mpi(pred.numpy(), fg.numpy(), AP)


def _assemble_cases():
    def net_in(k):
        return {"pred": _net(k)[0], "fg": _net(k)[1]}

    def net_homs_in(k):
        return dict(net_in(k), homs=cam_homs(k, NB, AP, NH, NW))

    def args(b):
        return b["pred"], _st(b["pred"]), b["fg"], _st(b["fg"])

    Case("assemble_mpi", ["mpiv_assemble_mpi"], net_in, {"rgba": ((NB, NH, NW, AP, 4), F32)},
         lambda b, d: _lib._call("mpiv_assemble_mpi", *args(b), NB, NH, NW, AP, b["rgba"], S(d)),
         lambda k: {"rgba": _net(k)[3]})
    Case("assemble_mpi_packed", ["mpiv_assemble_mpi_packed"], net_in, {"packed": ((AP, NH + 4, NW + 4, 4), F32)},
         lambda b, d: _lib._call("mpiv_assemble_mpi_packed", *args(b), 1, NH, NW, AP, b["packed"], S(d)),
         lambda k: {"packed": pack_host(_net(k)[3][1]).numpy()})

    def sampled_check(k):
        def check(got, b, label):
            written = ~torch.isnan(got).any(dim=-1)
            want = torch.from_numpy(_net(k)[3]).to(got.device)
            assert bool(written.any()), label + ": nothing written"
            assert torch.equal(got[written].view(torch.int32), want[written].view(torch.int32)), label
        return check

    def call_sampled(b, d):
        _lib._call("mpiv_assemble_mpi_sampled", *args(b), NB, NH, NW, AP, b["homs"], b["part"], S(d))
        _lib._call("mpiv_render_backward", b["part"], _st(b["part"]), NB, NH, NW, AP, b["homs"], b["dout"], None,
                   b["grad"], b["ws"], b["ws"].numel(), S(d))
    Case("assemble_mpi_sampled-then-backward", ["mpiv_assemble_mpi_sampled", "mpiv_render_backward"],
         lambda k: dict(net_homs_in(k), dout=lc.dout_for((NB, NH, NW, 3), seed=5 + k)),
         {"part": ((NB, NH, NW, AP, 4), F32, float("nan")), "grad": ((NB, NH, NW, AP, 4), F32)}, call_sampled,
         lambda k: {"part": sampled_check(k),
                    "grad": oracle.render_backward(_net(k)[3], cam_homs(k, NB, AP, NH, NW).numpy(),
                                                   lc.dout_for((NB, NH, NW, 3), seed=5 + k).numpy())},
         state={"ws": _ws_bytes(NH, NW, AP)}, after=_no_abort(NH, NW, AP))

    def bwd_in(k):
        return dict(net_in(k), drgba=_net(k)[2])

    def bwd_want(k, dfg):
        pred, fg, drgba, _ = _net(k)
        w = {"dpred": oracle.assemble_mpi_backward(drgba.numpy(), pred.numpy(), fg.numpy(), AP)}
        if dfg:
            w["dfg"] = oracle.assemble_mpi_backward_fg(drgba.numpy(), pred.numpy(), AP)
        return w
    for dfg in (True, False):
        outs = {"dpred": ((NB, 2 * AP + 3, NH, NW), F32)}
        if dfg:
            outs["dfg"] = ((NB, NH, NW, 3), F32)
        Case("assemble_mpi_backward-" + ("dfg" if dfg else "dfg_null"), ["mpiv_assemble_mpi_backward"], bwd_in, outs,
             lambda b, d, dfg=dfg: _lib._call("mpiv_assemble_mpi_backward", b["drgba"], _st(b["drgba"]), *args(b), NB,
                                              NH, NW, AP, b["dpred"], b["dfg"] if dfg else None, S(d)),
             lambda k, dfg=dfg: bwd_want(k, dfg))

    def frames(k, p_end=AP):
        h = np.ascontiguousarray(cam_homs(k, NB, AP, NH, NW).numpy()[:, :p_end])
        return oracle.render(_net(k)[3][:, :, :, :p_end], h)
    Case(f"render_net_output-{_route('render_net_output', NB, NH, NW, AP)}", ["mpiv_render_net_output"], net_homs_in,
         {"out": ((NB, NH, NW, 3), F32)},
         lambda b, d: _lib._call("mpiv_render_net_output", *args(b), NB, NH, NW, AP, b["homs"], b["out"], S(d)),
         lambda k: {"out": frames(k)})

    def ck_check(k):
        def check(got, b, label):
            match(got[:, 1, :, :, :3], frames(k, 8), label + ", slot 1")
        return check
    Case("render_net_output_train", ["mpiv_render_net_output_train"], net_homs_in,
         {"out": ((NB, NH, NW, 3), F32), "ckpt": ((NB, 2, NH, NW, 4), F32)},
         lambda b, d: _lib._call("mpiv_render_net_output_train", *args(b), NB, NH, NW, AP, b["homs"], b["out"],
                                 b["ckpt"], S(d)),
         lambda k: {"out": frames(k), "ckpt": ck_check(k)})


_assemble_cases()


# ---------------------------------------------------------------------------
# plane sweep, inverse warp
# ---------------------------------------------------------------------------

SB, SHS, SWS, SHT, SWT = 2, 64, 64, 48, 80
SWEEP_CD = [(3, 2), (3, 8), (3, 10), (3, 65), (5, 3)]  # direct, pixel per lane, depth lanes (x2), generic


@functools.lru_cache(maxsize=None)
def _sweep(k, C, D):
    """(img, ki [B,9], proj [B,16], depths [D], Ks [B,3,3], pose [B,4,4]) of data set k."""
    g = torch.Generator().manual_seed(600 + 10 * C + D + 1000 * k)
    img = torch.rand((SB, SHS, SWS, C), generator=g)
    f = 64.0 + 6.0 * k
    Ks = configs.f32([configs.intrinsics_matrix(f + b_, f - b_, 32.0 + k, 32.0 - 2 * k) for b_ in range(SB)])
    pose = configs.f32([configs.pose_from(configs.rot_y((2.0 + b_) * (1 - 2 * k)), (0.02 * (b_ + 1), -0.03 * k, 0.01))
                        for b_ in range(SB)])
    ki, proj = _host.psv_matrices(Ks, Ks, pose)
    depths = configs.f32(configs.inv_depths(1.0 + k, 50.0 + 25 * k, D))
    return img, ki.clone(), proj.clone(), depths, Ks, pose


@functools.lru_cache(maxsize=None)
def _sweep_want(k, C, D):
    img, ki, proj, depths, _, _ = _sweep(k, C, D)
    return oracle.plane_sweep(img.numpy(), ki.numpy(), proj.numpy(), depths.tolist(), SHT, SWT)


def pad_host(img):
    B, H, W, C = img.shape
    out = torch.zeros((B, H + 4, W + 4, 4))
    out[:, 2:2 + H, 2:2 + W, :C] = img
    return out


def _wide_check(k, C, D):
    def check(got, b, label):
        match(got[..., 2:2 + D * C], _sweep_want(k, C, D), label)
        assert bool((got[..., :2] == SENT).all()) and bool((got[..., 2 + D * C:] == SENT).all()), label + ": gaps"
    return check


def _sweep_cases():
    for C, D in SWEEP_CD:
        tag = f"C{C}-D{D}-{_route('plane_sweep', SB, SHS, SWS, C, D, SHT, SWT)}"
        pst = D * C + 5

        def base(k, C=C, D=D):
            img, ki, proj, depths, _, _ = _sweep(k, C, D)
            return {"img": img, "ki": ki, "proj": proj, "depths": depths}
        dense = {"out": ((SB, SHT, SWT, D * C), F32)}
        wide = {"wide": ((SB, SHT, SWT, pst), F32)}
        Case(f"plane_sweep-{tag}", ["mpiv_plane_sweep"], base, dense,
             lambda b, d, C=C, D=D: _lib._call("mpiv_plane_sweep", b["img"], _st(b["img"]), SB, SHS, SWS, C, b["ki"],
                                               b["proj"], b["depths"], D, SHT, SWT, b["out"], S(d)),
             lambda k, C=C, D=D: {"out": _sweep_want(k, C, D)})

        def pose_in(k, C=C, D=D):
            img, ki, _, depths, Ks, pose = _sweep(k, C, D)
            return {"img": img, "ki": ki, "Ks": Ks, "pose": pose, "depths": depths}
        Case(f"plane_sweep_pose-{tag}", ["mpiv_plane_sweep_pose"], pose_in,
             dict(dense, proj_scratch=((SB, 16), F32)),  # the caller's own scratch
             lambda b, d, C=C, D=D: _lib._call("mpiv_plane_sweep_pose", b["img"], _st(b["img"]), SB, SHS, SWS, C,
                                               b["ki"], b["Ks"], 9, b["pose"], b["proj_scratch"], b["depths"], D,
                                               SHT, SWT, b["out"], S(d)),
             lambda k, C=C, D=D: {"out": _sweep_want(k, C, D), "proj_scratch": _sweep(k, C, D)[2].numpy()})
        if C > 4:
            continue
        Case(f"plane_sweep_into-{tag}", ["mpiv_plane_sweep_into"], base, wide,
             lambda b, d, C=C, D=D, pst=pst: _lib._call(
                 "mpiv_plane_sweep_into", b["img"], _st(b["img"]), SB, SHS, SWS, C, b["ki"], b["proj"], b["depths"],
                 D, SHT, SWT, b["wide"][..., 2:], SHT * SWT * pst, pst, S(d)),
             lambda k, C=C, D=D: {"wide": _wide_check(k, C, D)})

        def padded_in(k, C=C, D=D):
            img, ki, proj, depths, _, _ = _sweep(k, C, D)
            return {"img4": pad_host(img), "ki": ki, "proj": proj, "depths": depths}
        Case(f"plane_sweep_padded-C{C}-D{D}", ["mpiv_plane_sweep_padded"], padded_in, dense,
             lambda b, d, C=C, D=D: _lib._call("mpiv_plane_sweep_padded", b["img4"], SB, SHS, SWS, C, b["ki"],
                                               b["proj"], b["depths"], D, SHT, SWT, b["out"], S(d)),
             lambda k, C=C, D=D: {"out": _sweep_want(k, C, D)})
        Case(f"plane_sweep_padded_into-C{C}-D{D}", ["mpiv_plane_sweep_padded_into"], padded_in, wide,
             lambda b, d, C=C, D=D, pst=pst: _lib._call(
                 "mpiv_plane_sweep_padded_into", b["img4"], SB, SHS, SWS, C, b["ki"], b["proj"], b["depths"], D, SHT,
                 SWT, b["wide"][..., 2:], SHT * SWT * pst, pst, S(d)),
             lambda k, C=C, D=D: {"wide": _wide_check(k, C, D)})
    C = 3
    Case("pad_texels-C3", ["mpiv_pad_texels"], lambda k: {"img": _sweep(k, C, 2)[0]},
         {"img4": ((SB, SHS + 4, SWS + 4, 4), F32)},
         lambda b, d: _lib._call("mpiv_pad_texels", b["img"], _st(b["img"]), SB, SHS, SWS, C, b["img4"], S(d)),
         lambda k: {"img4": pad_host(_sweep(k, C, 2)[0]).numpy()})

    def warp_in(k):
        img, ki, proj, _, _, _ = _sweep(k, C, 2)
        g = torch.Generator().manual_seed(77 + k)
        return {"img": img, "ki": ki, "proj": proj, "depth": torch.rand((SB, SHT, SWT), generator=g) * 4 + 0.5}

    def warp_want(k):
        w = warp_in(k)
        return {"out": oracle.inverse_warp(w["img"].numpy(), w["ki"].numpy(), w["proj"].numpy(), w["depth"].numpy())}
    Case("inverse_warp-C3", ["mpiv_inverse_warp"], warp_in, {"out": ((SB, SHT, SWT, C), F32)},
         lambda b, d: _lib._call("mpiv_inverse_warp", b["img"], _st(b["img"]), SB, SHS, SWS, C, b["ki"], b["proj"],
                                 b["depth"], _st(b["depth"]), SHT, SWT, b["out"], S(d)),
         warp_want)


_sweep_cases()


# ---------------------------------------------------------------------------
# grid_sample, over_composite
# ---------------------------------------------------------------------------

def _sampler_cases():
    Hi, Wi, C, N = 8, 16, 3, 2

    def inputs(k):
        if k == 0:
            return {"img": torch.cat([lc.image(1, Hi, Wi, C, "finite"), lc.image(1, Hi, Wi, C, "nonfinite")]),
                    "coords": lc.boundary_coords(N, Hi, Wi)}
        g = torch.Generator().manual_seed(91)
        Ho, Wo = lc.boundary_coords(N, Hi, Wi).shape[1:3]
        return {"img": torch.rand((N, Hi, Wi, C), generator=g),
                "coords": torch.rand((N, Ho, Wo, 2), generator=g) * 1.4 - 0.2}
    Ho, Wo = lc.boundary_coords(N, Hi, Wi).shape[1:3]
    for last in (False, True):
        shape = (N, Ho, Wo, C) if last else (N, C, Ho, Wo)

        def call(b, d, last=last):
            ost = _st(b["out"], (0, 3, 1, 2)) if last else _st(b["out"])
            _lib._call("mpiv_grid_sample", b["img"], _st(b["img"], (0, 3, 1, 2)), N, C, Hi, Wi, b["coords"],
                       _st(b["coords"]), Ho, Wo, b["out"], ost, S(d))
        Case("grid_sample-" + ("nhwc" if last else "nchw"), ["mpiv_grid_sample"], inputs, {"out": (shape, F32)}, call,
             lambda k, last=last: {"out": oracle.grid_sample_nchw(inputs(k)["img"].numpy().transpose(0, 3, 1, 2),
                                                                  inputs(k)["coords"].numpy(), last)})
    P, H, W = 5, 33, 70

    def layers(k):
        return {"layers": lc.finite_mpi(H, W, P, seed=20 + k).permute(2, 0, 1, 3).contiguous()}

    def table(b, dev):  # the device pointer table: a static tensor built before the capture
        b["ptrs"] = torch.tensor([b["layers"][i].data_ptr() for i in range(P)], dtype=torch.int64).to(dev)
    Case("over_composite-P5", ["mpiv_over_composite"], layers, {"out": ((H, W, 3), F32)},
         lambda b, d: _lib._call("mpiv_over_composite", b["ptrs"], P, H * W, 4, 1, b["out"], S(d)),
         lambda k: {"out": oracle.over_composite(layers(k)["layers"].numpy())}, prepare=table)


_sampler_cases()


# ---------------------------------------------------------------------------
# u8 and f16 MPIs, the synthetic generators
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _u8_mpi(k, H, W, P):
    g = torch.Generator().manual_seed(31 + H + 1000 * k)
    return torch.randint(0, 256, (H, W, P, 4), generator=g, dtype=torch.uint8)


def _u8_float(k, H, W, P):
    return (_u8_mpi(k, H, W, P).numpy().astype(np.float32) / np.float32(255.0)).astype(np.float32)


def _u8_words(packed_bytes):
    """[P, H+4, W+4, 4] uint8 -> the int32 words (R lowest byte)."""
    return torch.from_numpy(np.ascontiguousarray(packed_bytes.numpy()).view("<i4")[..., 0].copy())


def _synth_u8_words(seed, H, W, P):
    """The u8 generator's bytes from the oracle's float generator: the float channel is the top 24 bits
    of the hash (rgb as 2u - 1, exactly), the byte its top 8."""
    m = oracle.synth_mpi(seed, H, W, 0, P).astype(np.float64)
    m[..., :3] = (m[..., :3] + 1) / 2
    by = np.minimum(np.floor(m * 256), 255).astype(np.uint8)  # (plane 0's alpha 1 -> 255)
    return _u8_words(pack_host(torch.from_numpy(by)))


def _small_cases(H, W, P):
    V, tag = VP, f"{H}x{W}x{P}"
    ranges = ((0, P // 3), (P // 3, P))
    fmt = {
        "u8": dict(mpi=_u8_mpi, fl=_u8_float, dtype=torch.int32, pshape=(P, H + 4, W + 4),
                   pack=lambda m: _u8_words(pack_host(m))),
        "f16": dict(mpi=lambda k, H, W, P: torch.from_numpy(_half_mpi(H, W, P, 50 + k)),
                    fl=lambda k, H, W, P: _half_mpi(H, W, P, 50 + k).astype(np.float32), dtype=torch.float16,
                    pshape=(P, H + 4, W + 4, 4), pack=pack_host),
    }
    for f, d_ in fmt.items():
        def mpi(k, d_=d_):
            return d_["mpi"](k, H, W, P)

        def fl(k, d_=d_):
            return d_["fl"](k, H, W, P)

        def inputs(k, d_=d_, mpi=mpi):
            return {"packed": d_["pack"](mpi(k)), "homs": cam_homs(k, V, P, H, W)}
        Case(f"pack_planes_{f}-{tag}", [f"mpiv_pack_planes_{f}"], lambda k, mpi=mpi: {"mpi": mpi(k)},
             {"out": (d_["pshape"], d_["dtype"])},
             lambda b, d, f=f: _lib._call(f"mpiv_pack_planes_{f}", b["mpi"], _st(b["mpi"]), H, W, P, b["out"], S(d)),
             lambda k, d_=d_, mpi=mpi: {"out": d_["pack"](mpi(k)).numpy()})
        Case(f"unpack_planes_{f}-{tag}", [f"mpiv_unpack_planes_{f}"],
             lambda k, inputs=inputs: {"packed": inputs(k)["packed"]}, {"out": ((P, H + 4, W + 4, 4), F32)},
             lambda b, d, f=f: _lib._call(f"mpiv_unpack_planes_{f}", b["packed"], H, W, P, b["out"], S(d)),
             lambda k, fl=fl: {"out": pack_host(torch.from_numpy(fl(k))).numpy()})
        Case(f"render_packed_{f}-{tag}-{_route('render_packed_' + f, H, W, P, V)}", [f"mpiv_render_packed_{f}"],
             inputs, {"out": ((V, H, W, 3), F32)},
             lambda b, d, f=f: _lib._call(f"mpiv_render_packed_{f}", b["packed"], H, W, P, b["homs"], V, b["out"],
                                          S(d)),
             lambda k, fl=fl: {"out": oracle.render(_bcast(fl(k), V), cam_homs(k, V, P, H, W).numpy())})

        def call_ct(b, d, f=f):
            for i, (p0, p1) in enumerate(ranges):
                _lib._call(f"mpiv_render_packed_{f}_ct", b["packed"], H, W, P, p0, p1, int(p0 == 0), b["homs"], V,
                           b[f"ct{i}"], S(d))
        ct_route = "-" + _route("render_packed_f16_ct", H, W, P, V) if f == "f16" else ""  # (mpiv_route has no u8_ct)
        Case(f"render_packed_{f}_ct-{tag}{ct_route}", [f"mpiv_render_packed_{f}_ct"], inputs,
             {f"ct{i}": ((V, H, W, 4), F32) for i in range(2)}, call_ct,
             lambda k, fl=fl: {f"ct{i}": oracle.render_ct(_bcast(fl(k), V), cam_homs(k, V, P, H, W).numpy(), a, b_,
                                                          back=(a == 0)) for i, (a, b_) in enumerate(ranges)})

    # the generators take no input buffer: the two data sets are two seeds, both written by the closure
    seeds = (7, 0x9E3779B1)

    def call_synth(b, d, entry):
        for i, s in enumerate(seeds):
            _lib._call(entry, _lib.ctypes.c_uint32(s), H, W, 0, P, b[f"mpi{i}"], S(d))
    Case(f"synth_mpi_packed-{tag}", ["mpiv_synth_mpi_packed"], lambda k: {},
         {f"mpi{i}": ((P, H + 4, W + 4, 4), F32) for i in range(2)},
         lambda b, d: call_synth(b, d, "mpiv_synth_mpi_packed"),
         lambda k: {f"mpi{i}": pack_host(torch.from_numpy(oracle.synth_mpi(s, H, W, 0, P))).numpy()
                    for i, s in enumerate(seeds)})
    Case(f"synth_mpi_packed_u8-{tag}", ["mpiv_synth_mpi_packed_u8"], lambda k: {},
         {f"mpi{i}": ((P, H + 4, W + 4), torch.int32) for i in range(2)},
         lambda b, d: call_synth(b, d, "mpiv_synth_mpi_packed_u8"),
         lambda k: {f"mpi{i}": _synth_u8_words(s, H, W, P).numpy() for i, s in enumerate(seeds)})


for _s in PACKED_SHAPES:
    _small_cases(*_s)


# ---------------------------------------------------------------------------
# per-point helpers and the two codecs: the reference's golden inputs and outputs; data set 2 is the
# same input reversed along the batch and point axes and the golden output reversed the same way
# (every point is independent, so no code under test defines the expectation)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _small():
    z = np.load(os.path.join(GOLD, "small.npz"))
    return {k: z[k] for k in z.files}


def _rev(a, k, dims):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.flip(dims) if k else t).contiguous()


def _helper_cases():
    s = _small()
    M, n = 6, 99

    def tp_in(k):
        return {"pts": _rev(s["tp_pts"].reshape(M, n, 3), k, (0, 1)), "homs": _rev(s["tp_H"].reshape(M, 9), k, (0,))}
    Case("transform_points", ["mpiv_transform_points"], tp_in, {"out": ((M, n, 3), F32)},
         lambda b, d: _lib._call("mpiv_transform_points", b["pts"], M, n, b["homs"], b["out"], S(d)),
         lambda k: {"out": _rev(s["tp_out"].reshape(M, n, 3), k, (0, 1)).numpy()})

    def coords_want(k, Ht=9, Wt=11):
        # utils.py:176-188 on the golden transformed points: w == 0 -> w + 1e-8, then (u / w) / (Ht - 1),
        # (v / w) / (Wt - 1), each an fp32 division rounded once
        q = s["tp_out"].reshape(M, n, 3).astype(np.float32)
        w = q[..., 2]
        w = (w + np.float32(1e-8) * (w == 0)).astype(np.float32)
        c = np.stack([(q[..., 0] / w) / np.float32(Ht - 1), (q[..., 1] / w) / np.float32(Wt - 1)], -1)
        return {"out": _rev(c.astype(np.float32), k, (0, 1)).numpy()}
    Case("plane_coords", ["mpiv_plane_coords"], tp_in, {"out": ((M, n, 2), F32)},
         lambda b, d: _lib._call("mpiv_plane_coords", b["pts"], M, n, b["homs"], 9, 11, b["out"], S(d)), coords_want)
    nn = s["nh_in"].size // 3
    Case("normalize_homogeneous", ["mpiv_normalize_homogeneous"],
         lambda k: {"pts": _rev(s["nh_in"].reshape(nn, 3), k, (0,))}, {"out": ((nn, 2), F32)},
         lambda b, d: _lib._call("mpiv_normalize_homogeneous", b["pts"], nn, 2, b["out"], S(d)),
         lambda k: {"out": _rev(s["nh_out"].reshape(nn, 2), k, (0,)).numpy(),
                    "pts": _rev(s["nh_in_after"].reshape(nn, 3), k, (0,)).numpy()})  # w == 0 updated in place
    B, h, w = 2, 6, 7
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    pix = np.broadcast_to(np.stack([xs, ys, np.ones_like(xs)]).reshape(1, 3, h * w), (B, 3, h * w))
    ki = torch.inverse(torch.from_numpy(s["p2c_K"])).reshape(B, 9).numpy()
    Case("pixel2cam", ["mpiv_pixel2cam"],
         lambda k: {"depth": _rev(s["p2c_depth"].reshape(B, h * w), k, (0, 1)), "pix": _rev(pix, k, (0, 2)),
                    "ki": _rev(ki, k, (0,))}, {"cam": ((B, 4, h * w), F32)},
         lambda b, d: _lib._call("mpiv_pixel2cam", b["depth"], b["pix"], b["ki"], B, h * w, 1, b["cam"], S(d)),
         lambda k: {"cam": _rev(s["p2c_out"].reshape(B, 4, h * w), k, (0, 2)).numpy()})
    Case("cam2pixel", ["mpiv_cam2pixel"],
         lambda k: {"cam": _rev(s["p2c_out"].reshape(B, 4, h * w), k, (0, 2)),
                    "proj": _rev(s["c2p_proj"].reshape(B, 16), k, (0,))}, {"out": ((B, h * w, 2), F32)},
         lambda b, d: _lib._call("mpiv_cam2pixel", b["cam"], b["proj"], B, h * w, b["out"], S(d)),
         lambda k: {"out": _rev(s["c2p_out"].reshape(B, h * w, 2), k, (0, 1)).numpy()})
    npre = s["pre_in"].size
    Case("preprocess", ["mpiv_preprocess"], lambda k: {"img": _rev(s["pre_in"].reshape(-1), k, (0,))},
         {"out": ((npre,), F32)}, lambda b, d: _lib._call("mpiv_preprocess", b["img"], npre, b["out"], S(d)),
         lambda k: {"out": _rev(s["pre_out"].reshape(-1), k, (0,)).numpy()})
    ndep = s["dep_in"].size
    Case("deprocess_u8", ["mpiv_deprocess_u8"], lambda k: {"img": _rev(s["dep_in"].reshape(-1), k, (0,))},
         {"out": ((ndep,), torch.uint8)}, lambda b, d: _lib._call("mpiv_deprocess_u8", b["img"], ndep, b["out"], S(d)),
         lambda k: {"out": _rev(s["dep_out"].reshape(-1), k, (0,)).numpy()})


_helper_cases()


# ---------------------------------------------------------------------------
# the matrix chains on the device
# ---------------------------------------------------------------------------

def _matrix_cases():
    B, P = 3, 11

    @functools.lru_cache(maxsize=None)
    def cams(k):
        g = torch.Generator().manual_seed(17 + k)
        pose = configs.f32([configs.pose_from(configs.rot_y(float(torch.rand(1, generator=g)) * 40 - 20),
                                              ((torch.rand(3, generator=g) - 0.5) * (0.3 + v)).tolist())
                            for v in range(B)])
        K = configs.f32([configs.intrinsics_matrix(500.0 + v + 30 * k, 480.0 - k, 320.0, 200.0 + v) for v in range(B)])
        depths = configs.f32(configs.inv_depths(1 + k, 100, P))
        return pose, depths, K

    def hom_in(k):
        pose, depths, K = cams(k)
        return {"pose": pose, "depths": depths, "K": K, "kinv": torch.inverse(K).contiguous()}
    Case("render_homographies_device", ["mpiv_render_homographies_device"], hom_in, {"H": ((B, P, 9), F32)},
         lambda b, d: _lib._call("mpiv_render_homographies_device", b["pose"], b["depths"], b["K"], b["kinv"], B, P,
                                 b["H"], S(d)),
         lambda k: {"H": _host.render_homographies_torch(*cams(k), B).numpy()})

    def proj_want(k):
        pose, _, K = cams(k)
        k4 = torch.cat([K, torch.zeros(B, 3, 1)], dim=2)
        k4 = torch.cat([k4, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).repeat(B, 1, 1)], dim=1)
        return {"proj": torch.matmul(k4, pose).reshape(B, 16).numpy()}
    Case("psv_proj_device", ["mpiv_psv_proj_device"], lambda k: {"Ks": cams(k)[2], "pose": cams(k)[0]},
         {"proj": ((B, 16), F32)},
         lambda b, d: _lib._call("mpiv_psv_proj_device", b["Ks"], 9, b["pose"], B, b["proj"], S(d)), proj_want)


_matrix_cases()

CASE_IDS = [c.name for c in CASES]
