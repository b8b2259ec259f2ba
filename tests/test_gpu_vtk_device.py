"""VtkSeriesPlayer.preload: the series' entries converted once and kept in device memory, played through
rt_scene_update_triangles_device + rt_scene_update_instances (tests/test_gpu_vtk.py plays it through the host copy)."""
import os

import numpy as np
import pytest

from rtamd import Renderer
from rtamd.vtk import VtkSeriesPlayer, vtk_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VTK_DIR = os.path.join(HERE, "golden", "vtk")
F1 = os.path.join(VTK_DIR, "particle_000000000000100.vtk")
SERIES = os.path.join(VTK_DIR, "particle_mesh.vtk.series")


def test_preloaded_series_playback_equals_fresh_scene(gpu_lib):
    """load(1) from device memory renders the same bytes as a scene created from the second file (the fresh scene of
    test_series_playback_equals_fresh_scene), and load(0) after it the first frame's."""
    r = Renderer(vtk_scene(SERIES)).build_acceleration_structure(0, mode="lbvh").configure_camera(256, 144, ray_trace_depth=2)
    first = r.render(0, want_rgb=True)[1]
    player = VtkSeriesPlayer(r, SERIES).preload("cuda")
    assert len(player) == 2 and player.load(1) == pytest.approx(0.01)
    played = r.render(0, want_rgb=True)[1]
    assert not np.array_equal(first, played)
    fresh = Renderer(vtk_scene(F1)).build_acceleration_structure(0, mode="lbvh").configure_camera(256, 144, ray_trace_depth=2)
    assert np.array_equal(played, fresh.render(0, want_rgb=True)[1])
    player.load(0)
    assert np.array_equal(r.render(0, want_rgb=True)[1], first)
