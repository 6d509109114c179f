"""CPU: the three frame-level calls are ONE loop (csrc/vgx_hosttest.cpp) and one kernel family (csrc/vgx_raster.hip) that decide by a
level -- frame < textured < painted -- what three bodies used to decide by being different code. These cases pin that the level does
not leak: the same frame through vgxt_raster_frame, vgxt_raster_textured and vgxt_raster_painted gives each call's own numpy statement
(tests/raster_frame_model.py, raster_textured_model.py, raster_painted_model.py), and an input that only a wider level may refuse is
refused by that level alone. Exact everywhere: np.array_equal on whole uint32 buffers, the stride padding included.
tests/test_gpu_raster_levels.py runs the same cases through the device calls."""
import numpy as np
import pytest

import raster_frame_model as M
import raster_model as R
import raster_painted_model as P
import raster_textured_model as T
import test_raster_cpu as base
import test_raster_frame_cpu as fcpu
import test_raster_painted_cpu as pcpu
import test_raster_textured_cpu as tcpu

capi = R.capi
CLEAR = P.CLEAR
OK, BAD = capi.VGX_OK, capi.VGX_E_INVALID_ARG
LEVELS = ("frame", "textured", "painted")
FRAMES = ("classes", "state")


class HostRunner:
    """The three calls on a frame of raster_painted_model; images / gradients: instead of the frame's. Each returns the image."""

    def __init__(self, host):
        self.host = host

    def frame(self, f, tgt, want=OK, **unused):
        return fcpu.host_frame(self.host, f, tgt, want=want)

    def textured(self, f, tgt, images=None, want=OK, **unused):
        return tcpu.host_textured(self.host, f, tgt, images=images, want=want)

    def painted(self, f, tgt, images=None, gradients=None, want=OK):
        return pcpu.host_painted(self.host, f, tgt, images=images, gradients=gradients, want=want)


@pytest.fixture(scope="module")
def run():
    return HostRunner(pcpu.load_host())


def model(level, f, tgt, images=None, gradients=None):
    """The numpy statement of one level: a refused call leaves the background."""
    img = tgt.background()
    if level == "frame":
        return M.render(f, tgt, img)
    if level == "textured":
        return T.render(f, tgt, img, images=images)
    return P.render(f, tgt, img, images=images, gradients=gradients)


def with_tables(f, meshes=None, draws=None):
    """The frame with another mesh or draw table."""
    g = R.make(f.name, f.pos, f.color, f.idx, f.meshes if meshes is None else meshes, f.target)
    g.draws, g.dstate, g.uv, g.images, g.gradients, g.patterns = f.draws if draws is None else draws, f.dstate, f.uv, f.images, f.gradients, f.patterns
    return g


# ---- the cases: shared with the GPU test, which hands in a runner over the kernels ----------------------------------------------
def check_one_frame_three_levels(run, name, clear):
    """(1) UV kinds are absent at the frame level and painted draws show their vertex colours below the painted level."""
    f = P.frame(name)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    got = {}
    for level in LEVELS:
        want = model(level, f, tgt)
        got[level] = getattr(run, level)(f, tgt)
        assert np.array_equal(got[level], want), (level, base.where(got[level], want))
        assert R.guards_intact(tgt, got[level])
    assert np.array_equal(got["painted"], P.expected(name, clear))
    for a, b in (("frame", "textured"), ("textured", "painted"), ("frame", "painted")):
        assert not np.array_equal(got[a], got[b]), (a, b)  # else the frame proves nothing


def check_statuses_per_level(run):
    """(2) what only a wider level checks is refused by that level alone, and a refusal writes nothing."""
    # a gradient draw whose handle lies outside the gradient table
    f = P.frame("state")
    assert any(P.painted(f, m) == P.GRADIENT and (int(f.draws["state_key"][int(f.meshes["draw"][m])]) & 0xFFFF) == 1 for m in range(f.nm))
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        assert np.array_equal(run.painted(f, tgt, gradients=f.gradients[:1], want=BAD), tgt.background())
        for level in ("textured", "frame"):
            got, want = getattr(run, level)(f, tgt), model(level, f, tgt)
            assert np.array_equal(got, want) and not np.array_equal(got, tgt.background()), level
    # a sampled mesh whose image handle lies outside the image table
    f = P.frame("classes")
    assert any(T.sampled(f, m) for m in range(f.nm))
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for level in ("textured", "painted"):
            assert np.array_equal(getattr(run, level)(f, tgt, images=[], want=BAD), tgt.background()), level
        got, want = run.frame(f, tgt), model("frame", f, tgt)
        assert np.array_equal(got, want) and not np.array_equal(got, tgt.background())
    # a TEXT mesh whose draw lies outside the draw table: the draw index is checked before the kind, at every level
    text = [m for m in range(f.nm) if (int(f.meshes["subpath_kind"][m]) >> 28) == R.TEXT]
    meshes = f.meshes.copy()
    meshes["draw"][text[1]] = f.draws.shape[0]
    g = with_tables(f, meshes=meshes)
    for tgt in (g.target, g.target.with_clear(CLEAR)):
        for level in LEVELS:
            assert np.array_equal(getattr(run, level)(g, tgt, want=BAD), tgt.background()), level
            assert np.array_equal(model(level, g, tgt), tgt.background())


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", FRAMES)
def test_one_frame_three_levels(run, name, clear):
    check_one_frame_three_levels(run, name, clear)


def test_statuses_per_level(run):
    check_statuses_per_level(run)
