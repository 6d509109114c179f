"""GPU: the cases of tests/test_raster_levels_cpu.py through the device calls. vgx_raster_frame, vgx_raster_textured and
vgx_raster_painted run ONE kernel family (csrc/vgx_raster.hip: k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, PAINT>) that
decides by a level in its arguments what they draw, check and launch; these cases pin that the level does not leak, neither inside one
call nor from one call to the next on the same context (a tile bitmap or a mesh-state buffer a wider level left behind). Every
comparison is np.array_equal on the whole uint32 buffer, the stride padding included."""
import importlib

import numpy as np
import pytest

import raster_model as R
import raster_painted_model as P
import test_gpu_raster as G
import test_gpu_raster_frame as GF
import test_gpu_raster_painted as GP
import test_gpu_raster_textured as GT
import test_raster_levels_cpu as cpu

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = P.CLEAR
OK = capi.VGX_OK


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def warm_ctx(rt):
    ctx = rt.Context(0)
    rt.raster_reserve(ctx, 8192, 1 << 17)
    yield ctx
    ctx.close()


class DevRunner:
    """The runner of the cases over the kernels (tests/test_raster_levels_cpu.py: HostRunner)."""

    def __init__(self, rt, ctx):
        self.rt, self.ctx = rt, ctx

    def frame(self, f, tgt, want=OK, **unused):
        return GF.gpu_frame(self.rt, self.ctx, G.DevFrame(f), GF.DevState(f), tgt, want=want)[1]

    def textured(self, f, tgt, images=None, want=OK, **unused):
        return GT.gpu_textured(self.rt, self.ctx, G.DevFrame(f), GF.DevState(f), GT.DevTex(f, images=images), tgt, want=want)[1]

    def painted(self, f, tgt, images=None, gradients=None, want=OK):
        dp = GP.DevPaints(f.gradients if gradients is None else gradients, f.patterns)
        return GP.gpu_painted(self.rt, self.ctx, G.DevFrame(f), GF.DevState(f), GT.DevTex(f, images=images), dp, tgt, want=want)[1]


@pytest.fixture(scope="module")
def run(rt, warm_ctx):
    return DevRunner(rt, warm_ctx)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", cpu.FRAMES)
def test_one_frame_three_levels(run, name, clear):
    cpu.check_one_frame_three_levels(run, name, clear)


def test_statuses_per_level(run):
    cpu.check_statuses_per_level(run)


def test_levels_one_after_another_on_one_context(rt):
    """(3) painted, frame, textured, frame on a context of their own: each image is its level's, whatever ran before."""
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, 1024, 1 << 14)
        run = DevRunner(rt, ctx)
        for name in cpu.FRAMES:
            f = P.frame(name)
            for tgt in (f.target.with_clear(CLEAR), f.target):
                for level in ("painted", "frame", "textured", "frame"):
                    got, want = getattr(run, level)(f, tgt), cpu.model(level, f, tgt)
                    assert np.array_equal(got, want), (name, level, G.where(got, want))
    finally:
        ctx.close()
