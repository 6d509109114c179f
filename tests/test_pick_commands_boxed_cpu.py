"""CPU: the lane code of vgx_pick_commands_boxed (vgxt_pick_commands_boxed: the loop of vgxt_pick_commands with the one box clause of
csrc/vgx_cmd_bounds.h) against vgxt_pick_commands itself: NULL boxes and true boxes change no word of any hit, the closed edges of every
box included; an empty box hides its command, drawing or clipping; a box is tested per query; owners, limits inside a command and the
invalid-record status are unchanged. The GPU suite (tests/test_gpu_pick_commands_boxed.py) makes the same checks on the kernels."""
import ctypes as C

import numpy as np
import pytest

import command_boxes_harness as B
import pick_commands_harness as PH
import pick_commands_model as PC
import raster_commands_harness as CH

OK, BAD = B.OK, B.BAD


@pytest.fixture(scope="module")
def side():
    return B.HostSide(B.load_host())


@pytest.mark.parametrize("name", B.PICK_SCENES)
def test_null_boxes_are_pick_commands(side, name):
    want = B.check_pick_null_boxes(side, name)
    if name in PH.SCENES:
        assert PH.same(want, PH.expected(name).hits)   # and both are the model's answer


def test_true_boxes_change_no_answer(side):
    on_edge = sum(B.check_pick_true_boxes(side, name) for name in B.PICK_SCENES if name not in PH.NAN_SCENES)
    assert on_edge >= 8   # queries ON a box's edge that hit the box's command: an open box would lose them


def test_empty_box_hides_a_command(side):
    B.check_pick_empty_box(side)


def test_box_is_tested_per_query(side):
    B.check_pick_box_is_per_query(side)


def test_limits_and_invalid_record_under_boxes(side):
    B.check_pick_limits_and_invalid(side)


def test_misaligned_boxes_are_refused(side):
    sc = PH.scene("relative")
    q = PC.centre_queries(sc.target)[:4].copy()
    h = np.zeros(8, dtype=B.capi.pick_cmd_hit_dtype)
    boxes = np.zeros((4, 4), dtype=np.float32)
    base, bb = h.ctypes.data + (-h.ctypes.data) % 16, boxes.ctypes.data + (-boxes.ctypes.data) % 16
    sm = CH.streams_struct(sc, (sc.pos.ctypes.data, sc.color.ctypes.data, sc.uv.ctypes.data, sc.idx.ctypes.data))
    call = lambda b: side.host.vgxt_pick_commands_boxed(C.byref(sm), sc.cmds.ctypes.data, sc.cmds.shape[0], None, b, None, q.ctypes.data, 4, base, None)
    assert call(bb) == OK and call(None) == OK and call(bb + 4) == BAD and call(bb + 8) == BAD
