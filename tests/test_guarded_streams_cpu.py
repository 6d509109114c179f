"""CPU: the helper of the placement tests (tests/guarded_streams.py) and their inputs (tests/placement_cases.py), without a GPU.
check_guards finds one changed byte on either side of every stream's range, next to it and at the far end, and names the stream,
the side and the offset; place() reaches every residue of the skew table from every base address a device allocation can have;
the reference's sizes meet the conditions tests/test_gpu_output_placement.py states of its inputs. When a case of that file fails
while this file is green, the helper and the inputs are settled and the kernel is what is wrong."""
import numpy as np
import pytest

import guarded_streams as GS
import placement_cases as PC

RANGE_BYTES = {"pos": 8 * 37, "color": 4 * 37, "idx": 2 * 91, "meshes": 32 * 3, "uv": 4 * 37}


def arena(k, base=0, residue=0):
    n = RANGE_BYTES[k]
    a = np.full(GS.arena_bytes(n), GS.PATTERN[k], dtype=np.uint8)
    b = GS.place(base, residue)
    a[b:b + n] = np.arange(n, dtype=np.uint8) ^ 0x55  # the range itself holds anything
    return a, b, b + n


@pytest.mark.parametrize("k", GS.STREAMS)
def test_untouched_guards_pass(k):
    a, b, e = arena(k)
    GS.check_guards(a, b, e, GS.PATTERN[k], stream=k)
    a[b:e] = GS.PATTERN[k]  # (a range that happens to hold the pattern is no trouble either)
    GS.check_guards(a, b, e, GS.PATTERN[k], stream=k)


@pytest.mark.parametrize("where", ["next_to_the_range", "far_end"])
@pytest.mark.parametrize("side", ["front", "behind"])
@pytest.mark.parametrize("k", GS.STREAMS)
def test_one_changed_byte_is_found_and_named(k, side, where):
    a, b, e = arena(k, base=0x7F0000001238, residue=GS.SKEWS["S2"]["uv4" if k == "uv" else k])
    if side == "front":
        at = b - 1 if where == "next_to_the_range" else 0
        offset = at - b
    else:
        at = e if where == "next_to_the_range" else a.shape[0] - 1
        offset = at - e
    a[at] ^= 0x01
    with pytest.raises(AssertionError) as err:
        GS.check_guards(a, b, e, GS.PATTERN[k], stream=k)
    msg = str(err.value)
    assert msg.startswith("%s: %s guard touched at offset %d " % (k, side, offset)), msg
    assert "byte %d of the arena" % at in msg and "1 bytes differ" in msg, msg


def test_the_first_difference_is_the_one_named():
    a, b, e = arena("idx")
    a[b - 7] = a[b - 3] = a[e + 5] = 0
    with pytest.raises(AssertionError, match=r"idx: front guard touched at offset -7 .*2 bytes differ"):
        GS.check_guards(a, b, e, GS.PATTERN["idx"], stream="idx")
    a[b - 7] = a[b - 3] = GS.PATTERN["idx"]
    with pytest.raises(AssertionError, match=r"idx: behind guard touched at offset 5 "):
        GS.check_guards(a, b, e, GS.PATTERN["idx"], stream="idx")


def test_patterns_differ_per_stream():
    assert len(set(GS.PATTERN.values())) == len(GS.STREAMS) == len(GS.PATTERN)


@pytest.mark.parametrize("skew", GS.SKEW_NAMES)
def test_placement_reaches_every_residue_from_every_base(skew):
    """Base addresses with every multiple of 8 modulo 128 stand in for data_ptr(): the range starts at the residue, at least GUARD
    bytes into the arena and less than a line further, at an offset a typed view of the arena can start at, and the arena holds
    GUARD bytes behind it."""
    align = {"pos": 8, "color": 4, "idx": 2, "meshes": 8, "uv4": 4, "uv8": 8}
    for k, residue in GS.SKEWS[skew].items():
        assert residue % align[k] == 0 and 0 <= residue < GS.LINE
        for base in range(0x7F3200000000, 0x7F3200000000 + GS.LINE, 8):
            off = GS.place(base, residue)
            assert (base + off) % GS.LINE == residue, (k, base, off)
            assert GS.GUARD <= off < GS.GUARD + GS.LINE
            assert off % align[k] == 0  # (.view(dtype) of a uint8 slice wants its offset a multiple of the element size)
            for n in (0, 2, 8 * 12061):
                assert GS.arena_bytes(n) - (off + n) >= GS.GUARD


def test_skew_table_is_the_stated_one():
    rows = {s: tuple(GS.SKEWS[s][k] for k in ("pos", "color", "idx", "meshes", "uv4", "uv8")) for s in GS.SKEW_NAMES}
    assert rows == {"S0": (0, 0, 0, 0, 0, 0), "S1": (8, 4, 2, 8, 4, 8), "S2": (120, 124, 126, 24, 124, 120), "S3": (56, 12, 14, 16, 12, 56)}
    # S1: the least alignment each element type allows, and no 16-byte word starts there; S2: the first element is the last of a line
    assert all(rows["S1"][i] % 16 != 0 for i in range(6))
    assert (rows["S2"][0] + 8, rows["S2"][1] + 4, rows["S2"][2] + 2) == (128, 128, 128)


# ---- the inputs of tests/test_gpu_output_placement.py ---------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(PC.ROUTES))
def test_every_route_has_an_odd_vertex_total_an_index_stream_off_16_bytes_and_an_odd_first_vertex(route):
    outs = [PC.of_ref(PC.reference(n)) for n in PC.ROUTES[route]]
    for n, (nv, ni, m) in zip(PC.ROUTES[route], outs):
        print(route, n, nv, ni, m.shape[0], PC.conditions(nv, ni, m))
    PC.assert_route(route, outs)


def test_route_inputs_are_what_their_routes_need():
    """a / b / g: frame-sized batches (at most 2 048 draws); c: 40 and 39 instances of one drawing; d: every polyline of 128 vertices
    or more, every mesh behind the leading fill a stroke; e: 33 instances, more than 2 048 draws, three classes."""
    for n in ("fuzz3", "tiger1", "asm_fuzz3"):
        assert PC.inputs(n)[1].shape[0] <= 2048
    ps, d40 = PC.inputs("closed40")
    assert d40.shape[0] == 40 * ps.npaths and PC.inputs("closed39")[1].shape[0] == 39 * ps.npaths
    for n in ("walks", "walks_after_fill"):
        ref = PC.reference(n)
        assert int(ref.subpaths["num_vertices"].min()) >= 128
        strokes = np.isin(ref.meshes["subpath_kind"] >> 28, (PC.capi.MESH_STROKE, PC.capi.MESH_STROKE_AA))
        assert strokes[1:].all() and strokes[0] == (n == "walks")
    for n in ("tmpl_miter", "tmpl_round", "tmpl_classes", "asm_tmpl"):
        ps, d = PC.inputs(n)
        assert d.shape[0] == PC.TMPL_INSTANCES * ps.npaths > 2048
    assert PC.inputs("tmpl_static")[1].shape[0] > 2048


@pytest.mark.parametrize("which", ["slices", "three"])
def test_copying_entries_inputs(which):
    """More than one scan slice (1 024 items) of meshes / instances, or three meshes; cached meshes whose index counts are no
    multiples of 4; merged and submitted frames that meet the three conditions between them."""
    a, b, _, merged = PC.merge_inputs(which)
    cache, inst, frame = PC.submit_inputs(which)
    assert frame is not None
    if which == "slices":
        assert merged.meshes.shape[0] > 1024 and inst.shape[0] > 1024
    else:
        assert merged.meshes.shape[0] == 3 and cache.meshes.shape[0] == 3
    used = np.zeros(cache.meshes.shape[0], dtype=bool)
    for f, n in zip(inst["first_mesh"], inst["num_meshes"]):
        used[int(f):int(f) + int(n)] = True
    assert np.any(cache.meshes["num_indices"][used] % 4 != 0)
    PC.assert_route("merge", [PC.of_stream(PC.merge_inputs(w)[3]) for w in ("slices", "three")])
    PC.assert_route("submit", [PC.of_stream(PC.submit_inputs(w)[2]) for w in ("slices", "three")])


def test_concave_inputs():
    """More than one scan slice of fills, and three; between them an odd vertex total, an index stream off a 16-byte end, fills that
    start at odd vertices (where k_concave_emit's 16-byte position stores begin at 8 mod 16)."""
    big, small = PC.concave_reference("slices"), PC.concave_reference("three")
    assert big[2].shape[0] > 1024 and small[2].shape[0] == 3
    for nv, ni, m in (big, small):  # (here each of the two meets all three)
        assert all(PC.conditions(nv, ni, m).values()), (nv, ni, PC.conditions(nv, ni, m))
    PC.assert_route("concave", [big, small])
