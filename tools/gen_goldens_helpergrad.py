#!/usr/bin/env python3
"""Golden fixtures for the sampler's and the compositor's gradients: the reference's CPU autograd
through `bilinear_wrapper_torch` (utils.py:104-134), `resampler_wrapper_torch` (utils.py:395-407) and
`over_composite` (utils.py:136-157), computed by running the reference's utils.py.  Test tooling only
(see gen_goldens.py for how the reference is imported); writes tests/golden/helpergrad.npz.

Inputs are seeded draws (`helper_inputs` / `over_inputs` below, which the tests import: the file stores
the inputs' sha256, not the inputs):

    bw   bilinear_wrapper_torch, leading dims [2,3], a 9x11x4 source, 13x21 targets
    rs   resampler_wrapper_torch, [2,9,11,3] -> 13x21
         coordinates U(-0.25, 1.25); recorded: <c>_out, <c>_dimgs, <c>_dcoords, <c>_sha (imgs, coords, dout)
    oc<P> over_composite at [2,13,21,4], P in {1, 2, 9, 10, 33}: alphas of exactly 0 and 1 among the
         layers, cotangent pixels of +0 and -0; recorded: oc<P>_out, oc<P>_sha (the P layers stacked, dout),
         oc<P>_dsha = sha256 of the reference's [P,2,13,21,4] gradient block, and the block itself for
         P <= 2, layers 0 and P-1 of it (oc<P>_d0, oc<P>_dlast) above: the full blocks are 480 KB of
         incompressible floats, and over_composite's autograd is five lines of torch arithmetic that the
         tests re-run on the CPU and hold to the recorded digest before they compare.

The generator asserts that more than 30 % of the d imgs, d coords and d layers entries are non-zero.

Usage:  python tools/gen_goldens_helpergrad.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

OVER_P = (1, 2, 9, 10, 33)


def sha(*ts) -> str:
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def helper_inputs(name):
    """(imgs, coords, dout) of sampler case `name` as CPU tensors."""
    g = torch.Generator().manual_seed({"bw": 101, "rs": 102}[name])
    if name == "bw":
        imgs = torch.rand((2, 3, 9, 11, 4), generator=g)
        coords = torch.rand((2, 3, 13, 21, 2), generator=g) * 1.5 - 0.25
        dout = torch.rand((2, 3, 4, 13, 21), generator=g) * 2 - 1
    else:
        imgs = torch.rand((2, 9, 11, 3), generator=g)
        coords = torch.rand((2, 13, 21, 2), generator=g) * 1.5 - 0.25
        dout = torch.rand((2, 13, 21, 3), generator=g) * 2 - 1
    return imgs, coords, dout


def over_inputs(P):
    """(layers: list of P [2,13,21,4] tensors, dout [2,13,21,3]) as CPU tensors: 2 % of the alphas
    exactly 0, 2 % exactly 1; cotangent rows 0 and 1 of view 0 are +0 and -0."""
    g = torch.Generator().manual_seed(200 + P)
    stack = torch.rand((P, 2, 13, 21, 4), generator=g) * 1.5 - 0.25
    pick = torch.rand((P, 2, 13, 21), generator=g)
    stack[..., 3] = torch.where(pick < 0.02, torch.zeros(()), torch.where(pick > 0.98, torch.ones(()), stack[..., 3]))
    dout = torch.rand((2, 13, 21, 3), generator=g) * 2 - 1
    dout[0, 0] = 0.0
    dout[0, 1] = -0.0
    return [stack[p].clone() for p in range(P)], dout


def main():
    from gen_goldens import OUT, load_reference
    ref = load_reference()
    rec = {}
    for name, fn in (("bw", ref.bilinear_wrapper_torch), ("rs", ref.resampler_wrapper_torch)):
        imgs, coords, dout = helper_inputs(name)
        li, lc = imgs.clone().requires_grad_(), coords.clone().requires_grad_()
        out = fn(li, lc)
        out.backward(dout)
        for what, t in (("d imgs", li.grad), ("d coords", lc.grad)):
            nz = float((t != 0).double().mean())
            assert nz > 0.3 and bool(torch.isfinite(t).all()), (name, what, nz)
        rec.update({f"{name}_out": out.detach().numpy(), f"{name}_dimgs": li.grad.numpy(),
                    f"{name}_dcoords": lc.grad.numpy(), f"{name}_sha": np.array(sha(imgs, coords, dout))})
    for P in OVER_P:
        layers, dout = over_inputs(P)
        leaves = [t.clone().requires_grad_() for t in layers]
        out = ref.over_composite(leaves)
        out.backward(dout)
        block = torch.stack([t.grad for t in leaves])
        assert float((block != 0).double().mean()) > 0.3 and bool(torch.isfinite(block).all()), P
        assert any(bool((t[..., 3] == 0).any()) and bool((t[..., 3] == 1).any()) for t in layers)
        assert bool((dout[0, 0] == 0).all()) and bool(torch.signbit(dout[0, 1]).all())
        if P > 1:  # the -0 cotangent survives in layer 0 alone
            assert bool(torch.signbit(block[0, 0, 1, :, :3]).any()) and not bool(torch.signbit(block[1:, 0, 1]).any())
        rec.update({f"oc{P}_out": out.detach().numpy(), f"oc{P}_sha": np.array(sha(torch.stack(layers), dout)),
                    f"oc{P}_dsha": np.array(sha(block))})
        if P <= 2:
            rec[f"oc{P}_dlayers"] = block.numpy()
        else:
            rec[f"oc{P}_d0"], rec[f"oc{P}_dlast"] = block[0].numpy(), block[-1].numpy()
    path = os.path.join(OUT, "helpergrad.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
