"""CPU: the three frame-level calls are ONE loop (csrc/vgx_hosttest.cpp) and one kernel family (csrc/vgx_raster.hip) that decide by a
level -- frame < textured < painted -- what three bodies used to decide by being different code. These cases pin that the level does
not leak: the same frame through vgxt_raster_frame, vgxt_raster_textured and vgxt_raster_painted gives each call's own numpy statement
(tests/raster_frame_model.py, raster_textured_model.py, raster_painted_model.py), and an input that only a wider level may refuse is
refused by that level alone. Exact everywhere: np.array_equal on whole uint32 buffers, the stride padding included.
tests/test_gpu_raster_levels.py runs the same cases through the device calls."""
import pytest

import raster_harness as H


@pytest.fixture(scope="module")
def run():
    return H.HostRunner(H.load_host())


# ---- the cases (tests/raster_harness.py): shared with the GPU test, which hands in a runner over the kernels ------------------------
@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", H.LEVEL_FRAMES)
def test_one_frame_three_levels(run, name, clear):
    H.check_one_frame_three_levels(run, name, clear)


def test_statuses_per_level(run):
    H.check_statuses_per_level(run)
