"""Damage redraw (vgx_damage_meshes, vgx_damage_instances, vgx_raster_damaged): a numpy statement of the rules in include/vgx.h, the
inputs the CPU and GPU tests share, and the conditions those inputs must meet (tests/test_damage_cpu.py: the lane code through
libvgx_hosttest.so; tests/test_gpu_damage.py: the kernels).

The bitmap rule is restated here from the header's words (the span rule in float64, tile = pixel // 16). The restricted raster is built ON
raster_concave_model: pixels are independent of one another, so the image of vgx_raster_damaged is the full call's image inside the
marked tiles and the image it was given everywhere else. Every comparison is exact.

The property scene (scene()) is a frame of instances of a hand-built cache, so that vgx_cache_update can edit it; its images are never
computed by the model, only its marks: the check is product against product (a damaged redraw against a full redraw).
"""
import math

import numpy as np

import cache_cull_model as CM
import cache_update_model as U
import raster_concave_model as K
import raster_frame_model as M
import raster_model as R

capi = R.capi
oracle = CM.oracle
F = np.float32
D = np.float64
TILE = 16
CLEAR = K.CLEAR
SENTINEL = 0x51EEDBAD  # an image no call has written


# ---- the bitmap ----------------------------------------------------------------------------------------------------------------------
def tiles_wh(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def words(width, height):
    tw, th = tiles_wh(width, height)
    return (tw * th + 31) // 32


def span(lo, hi, origin, n):
    """The pixels of [0, n) whose sample origin + i + 0.5 may lie in [lo, hi], as an inclusive pair, or None. A NaN bound compares false
    and leaves its side at the image's edge."""
    base = D(origin) + D(0.5)
    with np.errstate(all="ignore"):
        dlo, dhi = D(F(lo)) - base, D(F(hi)) - base
    fa, fb = D(0.0), D(n) - D(1.0)
    if dlo > fa:
        fa = np.floor(dlo)
    if dhi < fb:
        fb = np.ceil(dhi)
    if not fa <= fb:
        return None
    return int(fa), int(fb)


def box_tiles(box, width, height, x0, y0):
    """(tx0, ty0, tx1, ty1) inclusive, or None."""
    a, b = span(box[0], box[2], x0, width), span(box[1], box[3], y0, height)
    if a is None or b is None:
        return None
    return a[0] // TILE, b[0] // TILE, a[1] // TILE, b[1] // TILE


def mark(bits, box, width, height, x0, y0):
    """ORs the tiles of one box into `bits` (uint32 [words], changed in place)."""
    r = box_tiles(box, width, height, x0, y0)
    if r is None:
        return
    tw, _ = tiles_wh(width, height)
    for ty in range(r[1], r[3] + 1):
        for tx in range(r[0], r[2] + 1):
            k = ty * tw + tx
            bits[k >> 5] |= np.uint32(1 << (k & 31))


def mark_meshes(bits, bounds, begin, end, num_meshes, width, height, x0, y0):
    for m in range(begin, min(end, num_meshes)):
        mark(bits, bounds[m], width, height, x0, y0)
    return bits


def mark_instances(bits, bounds, num_meshes, slots, ninst, dirty, limit, width, height, x0, y0):
    """Returns the status the call leaves."""
    status = capi.VGX_OK
    n = dirty.shape[0] if limit is None else min(dirty.shape[0], int(limit))
    for d in [int(x) for x in dirty[:n]]:
        if d >= ninst:
            status = capi.VGX_E_INVALID_ARG
            continue
        a, b = int(slots["first_mesh"][d]), int(slots["first_mesh"][d + 1])
        if b > num_meshes or b < a:
            status = capi.VGX_E_INVALID_ARG
            continue
        for m in range(a, b):
            mark(bits, bounds[m], width, height, x0, y0)
    return status


def bit_set(bits, k):
    return bool((int(bits[k >> 5]) >> (k & 31)) & 1)


def tile_mask(bits, tgt):
    """[rows, stride] bool: the pixels of the marked tiles (inside the image)."""
    tw, th = tiles_wh(tgt.width, tgt.height)
    mask = np.zeros((tgt.rows(), tgt.stride), dtype=bool)
    for ty in range(th):
        for tx in range(tw):
            if bit_set(bits, ty * tw + tx):
                mask[TILE * ty:min(TILE * ty + TILE, tgt.height), TILE * tx:min(TILE * tx + TILE, tgt.width)] = True
    return mask


def marked(bits, width, height):
    tw, th = tiles_wh(width, height)
    return sum(bit_set(bits, k) for k in range(tw * th))


def all_bits(width, height):
    tw, th = tiles_wh(width, height)
    bits = np.zeros(words(width, height), dtype=np.uint32)
    for k in range(tw * th):
        bits[k >> 5] |= np.uint32(1 << (k & 31))
    return bits


def checkerboard(width, height, phase=0):
    tw, th = tiles_wh(width, height)
    bits = np.zeros(words(width, height), dtype=np.uint32)
    for ty in range(th):
        for tx in range(tw):
            if (tx + ty + phase) % 2 == 0:
                k = ty * tw + tx
                bits[k >> 5] |= np.uint32(1 << (k & 31))
    return bits


# ---- the restricted raster -------------------------------------------------------------------------------------------------------------
def render_damaged(fr, tgt, image, bits, mesh_begin=0, mesh_end=None):
    """vgx_raster_damaged into `image` ([rows, stride] uint32, changed in place): the full call's pixels inside the marked tiles."""
    full = K.render(fr, tgt, image.copy(), mesh_begin, mesh_end)
    m = tile_mask(bits, tgt)
    image[m] = full[m]
    return image


# ---- marking cases: (name, width, height, x0, y0, boxes) ---------------------------------------------------------------------------------
EMPTY = CM.EMPTY
NAN = float("nan")


def below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def above(x):
    return float(np.nextafter(F(x), F(np.inf)))


def mark_cases():
    """Boxes against small images. 40 x 24: 3 x 2 tiles with partial edge tiles, all in one word; 528 x 20: 33 tiles a row, so the second
    row of tiles starts inside word 1 and a rectangle straddles two words; a negative origin."""
    cases = []
    cases.append(("small", 40, 24, 0, 0, [
        (1.0, 1.0, 5.0, 5.0),                      # one tile
        (0.0, 0.0, 16.5, 3.0),                     # maxx exactly on the centre of pixel 16: reaches tile 1
        (0.0, 17.0, below(16.5), 20.0),            # ... the next float below holds no sample of tile 1, but the span rule takes the outer
                                                   #     integer (ceil): still tile 1 -- a superset, as the rule says
        (15.5, 0.25, 15.5, 0.75),                  # a degenerate box on the centre of pixel 15: tile 0 alone
        (38.0, 20.0, 39.75, 23.75),                # the partial corner tile
        (0.0, 17.0, above(15.5), 20.0),            # where the rule's own boundary lies: past the centre of pixel 15 it reaches tile 1
        (16.5, 0.0, 20.0, 3.0),                    # minx on the centre of pixel 16: tile 1 alone
        (below(16.5), 0.0, 20.0, 3.0),             # ... the next float below: floor gives pixel 15, tile 0 as well
    ]))
    cases.append(("outside", 40, 24, 0, 0, [
        (-30.0, -30.0, -2.0, -2.0), (41.0, 2.0, 60.0, 9.0), (3.0, 24.6, 9.0, 50.0), (-9.0, 3.0, -0.75, 9.0),
    ]))
    cases.append(("over_edges", 40, 24, 0, 0, [
        (-10.0, 4.0, 3.0, 6.0), (35.0, 4.0, 99.0, 6.0), (20.0, -7.0, 22.0, 2.0), (20.0, 20.0, 22.0, 77.0), (-1e30, -1e30, 1e30, 1e30),
    ]))
    cases.append(("empty_nan", 40, 24, 0, 0, [
        tuple(EMPTY), (NAN, 3.0, 5.0, 6.0), (20.0, 3.0, NAN, 6.0), (20.0, NAN, 22.0, NAN), (np.inf, 0.0, np.inf, 5.0),
    ]))
    cases.append(("wide", 528, 20, 0, 0, [
        (500.0, 2.0, 527.0, 3.0),                  # row 0, bits 31 .. 32: two words
        (3.0, 17.0, 40.0, 19.0),                   # row 1, bits 33 .. 35
        (480.0, 1.0, 520.0, 19.5),                 # both rows, each across a word boundary (29 .. 32, 62 .. 65)
        (0.0, 16.5, 600.0, 16.5),                  # a whole row of tiles: bits 33 .. 65
    ]))
    cases.append(("origin", 40, 24, -7, -5, [
        (-7.0, -5.0, -6.0, -4.0), (8.5, 10.5, 9.5, 11.5), (below(9.5), 0.0, below(9.5), 1.0), (9.5, 0.0, 9.5, 1.0), (32.0, 18.0, 32.9, 18.9),
    ]))
    return cases


def mark_case_conditions():
    """Each case does what it is for, decided on the model alone."""
    by = {c[0]: c for c in mark_cases()}
    t = lambda c, k: box_tiles(by[c][5][k], *by[c][1:5])
    assert t("small", 0) == (0, 0, 0, 0) and t("small", 1) == (0, 0, 1, 0) and t("small", 2) == (0, 1, 1, 1) and t("small", 3) == (0, 0, 0, 0)
    assert t("small", 4) == (2, 1, 2, 1) and t("small", 5) == (0, 1, 1, 1) and t("small", 6) == (1, 0, 1, 0) and t("small", 7) == (0, 0, 1, 0)
    assert box_tiles((0.0, 17.0, 15.5, 20.0), 40, 24, 0, 0) == (0, 1, 0, 1)   # at the centre of pixel 15 itself: tile 0 alone
    assert all(t("outside", k) is None for k in range(4))
    assert t("over_edges", 0) == (0, 0, 0, 0) and t("over_edges", 1) == (2, 0, 2, 0) and t("over_edges", 2) == (1, 0, 1, 0)
    assert t("over_edges", 3) == (1, 1, 1, 1) and t("over_edges", 4) == (0, 0, 2, 1)
    assert t("empty_nan", 0) is None and t("empty_nan", 1) == (0, 0, 0, 0) and t("empty_nan", 2) == (1, 0, 2, 0) and t("empty_nan", 3) == (1, 0, 1, 1)
    assert t("empty_nan", 4) is None
    assert t("wide", 0) == (31, 0, 32, 0) and t("wide", 1) == (0, 1, 2, 1) and t("wide", 2) == (29, 0, 32, 1) and t("wide", 3) == (0, 1, 32, 1)
    assert tiles_wh(528, 20) == (33, 2) and words(528, 20) == 3 and words(40, 24) == 1
    assert t("origin", 0) == (0, 0, 0, 0) and t("origin", 1) == (0, 0, 1, 1) and t("origin", 2) == (0, 0, 1, 0) and t("origin", 3) == (1, 0, 1, 0)
    return True


# ---- dirty lists over a table of instances with different mesh counts ------------------------------------------------------------------------
def list_scene():
    """(bounds [nm, 4], slots [ninst + 1], width, height, x0, y0): 40 one-mesh instances, one of 300 meshes, a culled 0-mesh instance and
    some more one-mesh instances, every mesh a small box on a 528 x 40 image."""
    rs = np.random.RandomState(77)
    counts = [1] * 40 + [300] + [0] + [1] * 8
    nm = sum(counts)
    x, y = rs.uniform(-20, 540, nm), rs.uniform(-10, 45, nm)
    w, h = rs.uniform(0, 30, nm), rs.uniform(0, 12, nm)
    bounds = np.stack([x, y, x + w, y + h], axis=1).astype(F)
    slots = np.zeros(len(counts) + 1, dtype=capi.cache_slot_dtype)
    slots["first_mesh"] = np.concatenate([[0], np.cumsum(counts)])
    return bounds, slots, 528, 40, 0, 0


def dirty_lists():
    """name -> (dirty, limit, wanted status)."""
    OK, BAD = capi.VGX_OK, capi.VGX_E_INVALID_ARG
    u = lambda *v: np.array(v, dtype=np.uint32)
    return {
        "empty": (u(), None, OK),
        "one_big": (u(40), None, OK),
        "duplicates": (u(3, 3, 7, 3, 7), None, OK),
        "reverse": (np.arange(49, -1, -1, dtype=np.uint32), None, OK),
        "culled": (u(41), None, OK),
        "culled_between": (u(39, 41, 42), None, OK),
        "invalid_index": (u(5, 50, 6, 4000000000), None, BAD),
        "limit": (u(1, 2, 40, 45), 2, OK),
        "limit_zero": (u(1, 2), 0, OK),
        "limit_above": (u(1, 2), 99, OK),
        "big_beside_many": (np.concatenate([np.arange(0, 40, dtype=np.uint32), u(40), np.arange(42, 50, dtype=np.uint32)]), None, OK),
        "long": (np.tile(np.arange(50, dtype=np.uint32), 30), None, OK),   # 1 500 entries: the scan's three-pass form
    }


# ---- the property scene ------------------------------------------------------------------------------------------------------------------
class Cache:
    pass


def scene_cache():
    """Three ranges of one mesh each, in local space around (0, 0): an AA fill (its own vertex colours), a non-AA stroke-like quad (takes
    the instance's colour) and a contour mesh (a concave notch)."""
    b = K.Builder()
    inn, out = M.quad(-5.0, -4.0, 5.0, 4.0), M.quad(-6.0, -5.0, 6.0, 5.0)
    verts, cols, idx = [], [], []
    for k in range(4):
        verts += [inn[k], out[k]]
        cols += [0xC040A0FF, 0x0040A0FF]
        i0, i2 = 2 * k, 2 * ((k + 1) % 4)
        idx += [i0, i2, i0 + 1, i2, i2 + 1, i0 + 1]
    idx += [0, 2, 4, 0, 4, 6]
    b.mesh(verts, cols, idx, kind=capi.MESH_FILL_AA)
    b.mesh(M.quad(-7.0, -1.5, 7.0, 1.5), 0xFFFFFFFF, M.QUAD, kind=capi.MESH_STROKE)
    b.contours([K.NOTCH(-6.0, -6.0, 12.0, 12.0)], 0xB0E06030)
    f = b.frame("damage_cache", None)
    c = Cache()
    c.pos, c.color, c.idx, c.meshes = f.pos, f.color, f.idx, f.meshes
    c.meshes["draw"] = 0
    return c


WIDTH, HEIGHT, STRIDE = 96, 80, 99
CLIP_INST, IN_INST, OUT_INST = 2, 3, 4


def scene_instances():
    """13 instances: 12 drawings and, at index 2, the instance of a Clip draw (the stroke quad, stretched) with a user under In and one
    under Out right behind it."""
    rs = np.random.RandomState(5)
    inst = np.zeros(13, dtype=capi.cache_instance_dtype)
    for k in range(13):
        first = k % 3
        inst["first_mesh"][k], inst["num_meshes"][k] = (0, 3) if k in (7, 11) else (first, 1)
        inst["color"][k] = (0xC0 << 24) | int(rs.randint(0, 1 << 24))
        inst["mtx"][k] = [1.0, 0.0, 0.0, 1.0, 10.0 + 19.0 * (k % 5) + rs.uniform(-2, 2), 10.0 + 26.0 * (k // 5) + rs.uniform(-2, 2)]
    inst["first_mesh"][CLIP_INST], inst["num_meshes"][CLIP_INST] = 1, 1
    inst["mtx"][CLIP_INST] = [1.5, 0.0, 0.0, 6.0, 70.0, 20.0]
    inst["first_mesh"][IN_INST], inst["num_meshes"][IN_INST] = 2, 1
    inst["mtx"][IN_INST] = [1.0, 0.0, 0.0, 1.0, 66.0, 14.0]
    inst["first_mesh"][OUT_INST], inst["num_meshes"][OUT_INST] = 0, 1
    inst["mtx"][OUT_INST] = [1.0, 0.0, 0.0, 1.0, 76.0, 24.0]
    return inst


def scene_draws(ninst):
    """The draw table a cached frame is drawn with: one draw per instance (vgx_cache_submit leaves the instance's index in vgx_mesh::draw),
    all type 0 without a scissor but the Clip draw and its two users."""
    types = [0] * ninst
    states = [M.state()] * ninst
    types[CLIP_INST] = K.CLIP
    states[IN_INST] = M.state(region=(CLIP_INST, 1), rule=0)
    states[OUT_INST] = M.state(region=(CLIP_INST, 1), rule=1)
    return types, states


def scene_steps():
    """Five edits with fixed seeds: (name, [(instance, new mtx or None, new colour or None)])."""
    rs = np.random.RandomState(9)
    base = scene_instances()

    def moved(k, dx, dy):
        m = base["mtx"][k].copy()
        m[4] += F(dx); m[5] += F(dy)
        return m
    return [
        ("move_one", [(0, moved(0, 3.25, 1.5), None)]),
        ("move_two", [(7, moved(7, -4.0, 2.75), None), (9, moved(9, rs.uniform(2, 5), rs.uniform(-4, -2)), None)]),
        ("recolour", [(1, None, 0xE010F0A0), (10, None, 0xFF2040E0)]),
        ("move_clip", [(CLIP_INST, moved(CLIP_INST, -3.5, 1.0), None)]),
        ("partly_off", [(12, moved(12, -52.0, 25.0), None), (5, moved(5, 0.0, -20.0), None)]),
    ]


def submit(cache, inst):
    """The frame vgx_cache_submit writes for the array, as host arrays (the CPU oracle), and its slots."""
    fr = oracle.cache_submit(cache, inst)
    status, slots = U.layout_model(cache, inst)
    assert status == capi.VGX_OK
    return fr, slots


def scene_frame(cache, inst):
    """An R.Frame of the submitted array with the draw table, for the raster calls."""
    fr, slots = submit(cache, inst)
    f = R.make("damage_scene", fr.pos, fr.color, fr.idx, fr.meshes, R.Target(WIDTH, HEIGHT, STRIDE, 0, 0))
    types, states = scene_draws(inst.shape[0])
    return K.finish(f, [int(d) for d in fr.meshes["draw"]], types, states), slots


def scene_marks(steps=None):
    """Per step, on the model: (dirty list, bits of old + new boxes, bits of the new boxes alone, edited instance array). The instance
    arrays chain: step k edits what step k - 1 left."""
    cache = scene_cache()
    inst = scene_instances()
    out = []
    for name, edits in (scene_steps() if steps is None else steps):
        fr0, slots = submit(cache, inst)
        b0 = CM.mesh_boxes(fr0.pos, fr0.meshes)
        nxt = inst.copy()
        for k, mtx, col in edits:
            if mtx is not None:
                nxt["mtx"][k] = mtx
            if col is not None:
                nxt["color"][k] = col
        fr1, _ = submit(cache, nxt)
        b1 = CM.mesh_boxes(fr1.pos, fr1.meshes)
        dirty = np.array([e[0] for e in edits], dtype=np.uint32)
        both, new = np.zeros(words(WIDTH, HEIGHT), np.uint32), np.zeros(words(WIDTH, HEIGHT), np.uint32)
        mark_instances(both, b0, fr0.meshes.shape[0], slots, inst.shape[0], dirty, None, WIDTH, HEIGHT, 0, 0)
        mark_instances(both, b1, fr1.meshes.shape[0], slots, inst.shape[0], dirty, None, WIDTH, HEIGHT, 0, 0)
        mark_instances(new, b1, fr1.meshes.shape[0], slots, inst.shape[0], dirty, None, WIDTH, HEIGHT, 0, 0)
        out.append((name, dirty, both, new, nxt))
        inst = nxt
    return out


def scene_conditions(marks):
    """At every step at least one tile is marked and at least one is not (else the test shows nothing about skipping); one step moves
    an instance partly off the image."""
    tw, th = tiles_wh(WIDTH, HEIGHT)
    for name, dirty, both, new, _ in marks:
        n = marked(both, WIDTH, HEIGHT)
        assert 1 <= n < tw * th, (name, n)
        assert np.array_equal(both | new, both)
    last = marks[-1][4]
    cache = scene_cache()
    fr, slots = submit(cache, last)
    b = CM.mesh_boxes(fr.pos, fr.meshes)
    m12 = int(slots["first_mesh"][12])
    assert b[m12][0] < 0 < b[m12][2]  # partly off the left edge
    return True
