"""GPU: vgx_command_bounds (csrc/vgx_cmd_bounds.hip: the chunk scan, k_cmdb_tris, k_cmdb_decode) against the numpy statement of the
specification (tests/command_bounds_model.py) and, where a table meets its precondition, against vgx_mesh_bounds: the checks of
tests/test_command_bounds_cpu.py on the kernels, the runs of chunks under a lowered grid, the runtime wrapper, the scratch and a counted
state."""
import ctypes as C
import os

import numpy as np
import pytest

import command_boxes_harness as B
import command_bounds_model as BM
import raster_commands_harness as CH
import raster_harness as H
from raster_harness import rt  # noqa: F401

pytestmark = pytest.mark.gpu
OK, BAD = B.OK, B.BAD


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side(rt, ctx):
    return B.DevSide(rt, ctx)


@pytest.mark.parametrize("name", ["relative", "shared_indices", "odd_lists", "short_table", "count_129", "clip"])
def test_boxes_equal_model(side, name):
    got = B.check_bounds_equal_model(side, CH.scene(name))
    if name == "short_table":
        assert (got[2:] == B.FILL).all()   # the records behind dev_num_cmds: untouched


def test_structural_cases(side):
    B.check_bounds_structural(side)


@pytest.mark.parametrize("grid", [None, 1, 3])
def test_runs_meet_inside_a_command(rt, side, grid):
    """70 chunks of one command: at the default grid every wave has one chunk; with VGX_PICK_GRID (read when the context is created) at 1
    and 3 a wave walks a run of 18 and of 6, the runs meet inside the command, and the first and last run cross into its neighbours."""
    if grid is None:
        B.check_bounds_equal_model(side, B.big_command())
        return
    os.environ["VGX_PICK_GRID"] = str(grid)
    try:
        c = rt.Context(0)
    finally:
        del os.environ["VGX_PICK_GRID"]
    try:
        s = B.DevSide(rt, c)
        B.check_bounds_equal_model(s, B.big_command())
        B.check_bounds_structural(s)
    finally:
        c.close()


def test_range_call_leaves_the_other_entries(side):
    B.check_bounds_range(side)


def test_invalid_records(side):
    B.check_bounds_invalid(side)


@pytest.mark.parametrize("name", B.MESH_BOUNDS_SCENES)
def test_equals_mesh_bounds_where_its_precondition_holds(side, name):
    B.check_bounds_equal_mesh_bounds(side, name)


def test_more_commands_than_one_scan_workgroup_holds(side):
    """1 500 commands: the three-pass form of the scan, and commands without chunks in the walk."""
    sc = CH.scene("clip")
    cmds = np.tile(sc.cmds, 215)[:1500].copy()
    cmds["num_indices"][::7] = 0
    big = sc.with_cmds(cmds)
    B.check_bounds_equal_model(side, big)
    want = BM.boxes(big, 1030, 1100)[0]
    assert B.same_boxes(side.bounds(big, 1030, 1100), want)


def test_runtime_wrapper_scratch_and_host_refusals(rt):
    import torch
    sc = B.structural()
    dev = CH.DevScene(sc)
    n = sc.cmds.shape[0]
    c = rt.Context(0)
    try:
        lib = rt.lib()
        b0 = int(lib.vgx_scratch_bytes(c.handle))
        table, status = rt.command_bounds(c, dev.streams, dev.t[3], n)
        torch.cuda.synchronize()
        assert int(status.item()) == OK and B.same_boxes(table.cpu().numpy(), BM.boxes(sc)[0])
        b1 = int(lib.vgx_scratch_bytes(c.handle))
        assert 8 * n <= b1 - b0 <= 512 * 32 + 3 * 4096 + 64 * n   # the prefix, the state words, the slice sums: on the context's list
        table2, _ = rt.command_bounds(c, dev.streams, dev.t[3], n, cmd_begin=1, cmd_end=2, bounds_dev=torch.full_like(table, 5.0))
        torch.cuda.synchronize()
        got = table2.cpu().numpy()
        assert (got[[0, 2, 3, 4]] == 5.0).all() and B.same_boxes(got[1:2], BM.boxes(sc)[0][1:2])
        assert int(lib.vgx_scratch_bytes(c.handle)) == b1   # a call of the same size or smaller grows nothing
        h, s = c.handle, rt._stream_ptr()
        call = lambda **k: lib.vgx_command_bounds(k.get("h", h), k.get("sm", C.byref(dev.streams)), k.get("cmds", dev.t[3].data_ptr()), n, k.get("real", None), 0, B.ALL,
                                                  k.get("bounds", table.data_ptr()), k.get("status", None), s)
        assert call() == OK
        assert call(h=None) == BAD and call(sm=None) == BAD and call(cmds=None) == BAD and call(bounds=None) == BAD
        assert call(bounds=table.data_ptr() + 8) == BAD and call(cmds=dev.t[3].data_ptr() + 4) == BAD and call(status=table.data_ptr() + 2) == BAD
        torch.cuda.synchronize()
    finally:
        c.close()


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_command_bounds -> vgx_tessellate_emit gives the oracle's meshes."""
    sc = B.structural()
    dev = CH.DevScene(sc)
    want = BM.boxes(sc)[0]
    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, lambda: rt.command_bounds(gpu_ctx, dev.streams, dev.t[3], sc.cmds.shape[0]), want.view(np.uint32))
