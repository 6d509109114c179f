"""GPU: vgx_pick_commands_boxed (the BOXED instantiations of k_pickc_cmds and k_pickc_tris in csrc/vgx_pick_cmds.hip) against
vgx_pick_commands on the same device: the checks of tests/test_pick_commands_boxed_cpu.py on the kernels, with the boxes the kernels of
vgx_command_bounds give, and the runtime wrapper."""
import numpy as np
import pytest

import command_boxes_harness as B
import pick_commands_harness as PH
import pick_commands_model as PC
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


def test_runtime_wrapper_and_misaligned_boxes(rt, ctx):
    import ctypes as C
    import torch
    name = "clip"
    sc, q = PH.scene(name), PH.query_set(name)[0][:256]
    dev = CH.DevScene(sc)
    n = sc.cmds.shape[0]
    boxes, st = rt.command_bounds(ctx, dev.streams, dev.t[3], n)
    qd = H.to_dev(q)
    want, s0 = rt.pick_commands(ctx, dev.streams, dev.t[3], n, qd, 256)
    got, s1 = rt.pick_commands_boxed(ctx, dev.streams, dev.t[3], n, boxes, qd, 256)
    null, s2 = rt.pick_commands_boxed(ctx, dev.streams, dev.t[3], n, None, qd, 256)
    torch.cuda.synchronize()
    assert [int(s.item()) for s in (st, s0, s1, s2)] == [OK] * 4
    assert torch.equal(got[:256 * 16], want[:256 * 16]) and torch.equal(null[:256 * 16], want[:256 * 16])
    assert PH.same(want.cpu().numpy()[:256 * 16].view(B.capi.pick_cmd_hit_dtype), PH.expected(name, owners=False).hits[:256])
    assert rt.lib().vgx_pick_commands_boxed(ctx.handle, C.byref(dev.streams), dev.t[3].data_ptr(), n, None, boxes.data_ptr() + 8, None, qd.data_ptr(), 256,
                                            got.data_ptr(), None, rt._stream_ptr()) == BAD
    torch.cuda.synchronize()
