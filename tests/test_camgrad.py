"""The camera gradient's host half (CPU): _host.render_homographies_autograd, the reference's
homography chain kept on the autograd graph, against tests/golden/camgrad.npz
(tools/gen_goldens_camgrad.py: the reference's own d frame / d homographies and its gradients
w.r.t. tgt_pose, planes and intrinsics).

The golden cameras have power-of-two focal lengths and dyadic principal points, so their inverses
are exact on every host and the chain -- the same torch ops as the reference -- reproduces its
gradients bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, assert_bits

from mpi_vision_amd import _host  # noqa: E402

CASES = ["ca", "cb", "cl", "cf", "cbc", "c1"]


@pytest.fixture(scope="module")
def cam():
    return np.load(os.path.join(GOLD, "camgrad.npz"))


def cameras(cam, name):
    return tuple(torch.tensor(cam[f"{name}_{k}"]) for k in ("pose", "depths", "K"))


@pytest.mark.parametrize("name", CASES)
def test_autograd_chain_values_equal_render_homographies(name, cam):
    pose, depths, K = cameras(cam, name)
    B = pose.shape[0]
    want = _host.render_homographies(pose, depths, K, B)
    got = _host.render_homographies_autograd(pose.requires_grad_(), depths.requires_grad_(), K.requires_grad_(), B)
    assert got.requires_grad and got.shape == want.shape
    assert_bits(got, want.numpy(), f"{name} homographies")
    assert_bits(got, _host.render_homographies_torch(pose, depths, K, B).numpy(), f"{name} op-by-op homographies")


@pytest.mark.parametrize("name", CASES)
def test_autograd_chain_reproduces_the_reference_gradients(name, cam):
    """Backpropagating the reference's dH through the chain gives its dpose, dplanes and dK."""
    pose, depths, K = (t.requires_grad_() for t in cameras(cam, name))
    homs = _host.render_homographies_autograd(pose, depths, K, pose.shape[0])
    homs.backward(torch.tensor(cam[f"{name}_dH"]))
    assert_bits(pose.grad, cam[f"{name}_dpose"], f"{name} d tgt_pose")
    assert_bits(depths.grad, cam[f"{name}_dplanes"], f"{name} d planes")
    assert_bits(K.grad, cam[f"{name}_dK"], f"{name} d intrinsics")
    assert float(pose.grad.abs().max()) > 0 and float(depths.grad.abs().max()) > 0 and float(K.grad.abs().max()) > 0


def test_autograd_chain_only_tracks_what_requires_grad(cam):
    pose, depths, K = cameras(cam, "ca")
    assert not _host.render_homographies_autograd(pose, depths, K, 2).requires_grad
    homs = _host.render_homographies_autograd(pose.requires_grad_(), depths, K, 2)
    homs.sum().backward()
    assert pose.grad is not None and depths.grad is None and K.grad is None
    assert not bool(pose.grad[:, 3].any())  # the pose's last row takes no part
