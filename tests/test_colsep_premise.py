"""The premise of the rows kernels' column-separable path (render.hip ColSet): the host chain
(_host.render_homographies) gives h[1] == h[7] == 0 for every pose and plane of the benchmark's
camera paths (yaw + translation, zero-skew intrinsics).  If a change to the host chain broke
this, the launches would silently fall back to the per-row recipe."""
import pytest
import torch

from mpi_vision_amd import _host, configs


@pytest.mark.parametrize("name", ["config4", "config2", "config5"])
def test_camera_paths_are_column_separable(name):
    c = getattr(configs, name)()
    V = len(c["poses"])
    homs = _host.render_homographies(configs.f32(c["poses"]), configs.f32(c["depths"]), configs.f32([c["K"]] * V), V)
    assert tuple(homs.shape) == (V, c["P"], 9)
    assert torch.isfinite(homs).all()
    assert (homs[..., 1] == 0).all() and (homs[..., 7] == 0).all()
    # not a degenerate chain: the other entries of the y column and the x terms are live
    assert (homs[..., 4] != 0).all() and (homs[..., 0] != 0).all()
