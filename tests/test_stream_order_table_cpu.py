"""CPU: the table of tests/stream_order.py stays complete -- one row for every prototype of include/vgx.h with a `void* stream`
parameter, each resting on a line of the header -- and the decoys that have a CPU oracle keep the structure of the real inputs."""
import pytest

import stream_order as SO


def test_every_stream_entry_has_a_row():
    entries = SO.stream_entries()
    assert len(entries) >= 49 and "vgx_pick_rect" in entries and "vgx_create" not in entries
    rows = set(r.entry for r in SO.CASES)
    assert not (rows & set(SO.EXCLUDED)), rows & set(SO.EXCLUDED)
    assert entries == rows | set(SO.EXCLUDED), {"without a row": sorted(entries - rows - set(SO.EXCLUDED)), "not in the header": sorted((rows | set(SO.EXCLUDED)) - entries)}
    assert all(SO.EXCLUDED.values())
    names = [r.name for r in SO.CASES + SO.SENSITIVITY]
    assert len(names) == len(set(names))


def test_every_row_rests_on_a_line_of_the_header():
    lines = SO.header_text().splitlines()
    for r in SO.CASES:
        assert r.cls in (SO.ASYNC, SO.HOST), r.name
        assert r.header and any(r.header in line for line in lines), (r.name, r.header)
    # the entries that return data to the host say so themselves; the others may rest on the general convention
    assert all(r.header != SO.GENERAL for r in SO.CASES if r.cls == SO.HOST)
    assert any(SO.GENERAL in line for line in lines)


def test_sensitivity_rows_cover_the_three_families():
    assert sorted(r.entry for r in SO.SENSITIVITY) == ["vgx_pick", "vgx_raster", "vgx_tessellate_immediate"]
    assert all(r.sensitivity for r in SO.SENSITIVITY) and not any(r.sensitivity for r in SO.CASES)


def test_the_parser_reads_prototypes_that_span_lines():
    text = "int vgx_a(vgx_ctx* ctx, void* stream);\nint vgx_b(vgx_ctx* ctx,\n          uint32_t n, void* stream);\nint vgx_c(vgx_ctx* ctx, void* rccl_comm);\n/* int vgx_d(void* stream) */\n"
    assert SO.stream_entries(text) == {"vgx_a", "vgx_b"}


@pytest.mark.parametrize("check", SO.structure_checks(), ids=lambda c: getattr(c, "__name__", None) or "draws_x%d" % c.args[0])
def test_decoys_keep_the_structure_of_the_real_inputs(oracle, check):
    check()
