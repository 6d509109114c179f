"""CPU: the lane code of vgx_command_bounds (csrc/vgx_cmd_bounds.h through libvgx_hosttest.so: vgxt_command_bounds) against the numpy
statement of the specification (tests/command_bounds_model.py), on tables with overlapping and relative ranges, a short table, the
structural cases of the chunk walk, a range call between guards, invalid records, and against vgxt_mesh_bounds where a table meets its
precondition. The GPU suite (tests/test_gpu_command_bounds.py) makes the same checks on the kernels."""
import ctypes as C

import numpy as np
import pytest

import command_boxes_harness as B
import raster_commands_harness as CH

OK, BAD = B.OK, B.BAD


@pytest.fixture(scope="module")
def side():
    return B.HostSide(B.load_host())


@pytest.mark.parametrize("name", ["relative", "shared_indices", "odd_lists", "short_table", "count_129", "clip"])
def test_boxes_equal_model(side, name):
    got = B.check_bounds_equal_model(side, CH.scene(name))
    if name == "short_table":
        assert (got[2:] == B.FILL).all()   # the records behind dev_num_cmds: untouched


def test_structural_cases(side):
    B.check_bounds_structural(side)


def test_runs_meet_inside_a_command(side):
    B.check_bounds_equal_model(side, B.big_command())


def test_range_call_leaves_the_other_entries(side):
    B.check_bounds_range(side)


def test_invalid_records(side):
    B.check_bounds_invalid(side)


@pytest.mark.parametrize("name", B.MESH_BOUNDS_SCENES)
def test_equals_mesh_bounds_where_its_precondition_holds(side, name):
    B.check_bounds_equal_mesh_bounds(side, name)


def test_host_refusals(side):
    sc = CH.scene("relative")
    host = side.host
    table = np.zeros((4, 4), dtype=np.float32)
    base = table.ctypes.data + (-table.ctypes.data) % 16
    ptrs = (sc.pos.ctypes.data, sc.color.ctypes.data, sc.uv.ctypes.data, sc.idx.ctypes.data)

    def call(sm=None, cmds=sc.cmds.ctypes.data, n=sc.cmds.shape[0], real=None, begin=0, end=B.ALL, bounds=base, status=None):
        sm = CH.streams_struct(sc, ptrs) if sm is None else sm
        return host.vgxt_command_bounds(C.byref(sm) if sm != 0 else None, cmds, n, real, begin, end, bounds, status)

    assert call() == OK
    assert call(sm=0) == BAD and call(cmds=None) == BAD and call(bounds=None) == BAD
    assert call(cmds=None, n=0, bounds=None) == OK and call(bounds=None, begin=2, end=2) == OK and call(bounds=None, begin=2) == OK
    for k, v in (("reserved", 1), ("uv_bytes", 3), ("pos", None), ("color", None), ("idx", None)):
        sm = CH.streams_struct(sc, ptrs)
        setattr(sm, k, v)
        assert call(sm=sm) == BAD, k
    assert call(bounds=base + 8) == BAD and call(cmds=sc.cmds.ctypes.data + 4) == BAD and call(real=base + 2) == BAD and call(status=base + 2) == BAD
