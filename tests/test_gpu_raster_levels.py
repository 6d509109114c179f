"""GPU: the cases of tests/test_raster_levels_cpu.py through the device calls. vgx_raster_frame, vgx_raster_textured and
vgx_raster_painted run ONE kernel family (csrc/vgx_raster.hip: k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, PAINT>) that
decides by a level in its arguments what they draw, check and launch; these cases pin that the level does not leak, neither inside one
call nor from one call to the next on the same context (a tile bitmap or a mesh-state buffer a wider level left behind). Every
comparison is np.array_equal on the whole uint32 buffer, the stride padding included."""
import numpy as np
import pytest

import raster_harness as H
import raster_painted_model as P
from raster_harness import DevRunner, rt, warm_ctx  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
CLEAR = P.CLEAR


@pytest.fixture(scope="module")
def run(rt, warm_ctx):
    return DevRunner(rt, warm_ctx)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", H.LEVEL_FRAMES)
def test_one_frame_three_levels(run, name, clear):
    H.check_one_frame_three_levels(run, name, clear)


def test_statuses_per_level(run):
    H.check_statuses_per_level(run)


def test_levels_one_after_another_on_one_context(rt):
    """(3) painted, frame, textured, frame on a context of their own: each image is its level's, whatever ran before."""
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, 1024, 1 << 14)
        run = DevRunner(rt, ctx)
        for name in H.LEVEL_FRAMES:
            f = P.frame(name)
            for tgt in (f.target.with_clear(CLEAR), f.target):
                for level in ("painted", "frame", "textured", "frame"):
                    got, want = getattr(run, level)(f, tgt), H.model(level, f, tgt)
                    assert np.array_equal(got, want), (name, level, H.where(got, want))
    finally:
        ctx.close()
