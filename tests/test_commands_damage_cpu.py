"""CPU: the lane code of vgx_raster_commands_damaged (vgxt_raster_commands_damaged: the loop of vgxt_raster_commands restricted by the
damage bits and the command boxes) against vgxt_raster_commands: `where(pixel in a marked tile, image of the full call, image before)`,
in every byte, stride padding and guard rows included; boxes NULL and true; "what the table holds decides"; the redraw property over five
edit steps with the chain vgx_command_bounds -> vgx_damage_meshes -> edit -> vgx_command_bounds -> vgx_damage_meshes ->
vgx_raster_commands_damaged. The GPU suite (tests/test_gpu_commands_damage.py) makes the same checks on the kernels."""
import pytest

import command_boxes_harness as B
import raster_commands_harness as CH


@pytest.fixture(scope="module")
def side():
    return B.HostSide(B.load_host())


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", sorted(CH.SCENES))
def test_every_bit_set_is_the_full_call(side, name, clear):
    B.check_all_bits(side, name, clear)


def test_no_bit_set_writes_nothing_and_still_reports_an_invalid_record(side):
    B.check_no_bits(side)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", B.QUARTER_SCENES)
def test_a_random_quarter_of_the_tiles(side, name, clear):
    B.check_random_quarter(side, name, clear)


def test_clip_command_partly_in_unmarked_tiles(side):
    B.check_clip_partly_unmarked(side)


def test_tile_of_five_chunks_alone_then_its_neighbours_alone(side):
    B.check_trips_tile_and_neighbours(side)


def test_bits_across_a_word_boundary(side):
    B.check_word_boundary(side)


def test_what_the_box_table_holds_decides(side):
    B.check_boxes_decide(side)


def test_redraw_property(side):
    B.check_redraw_property(side)
