// vgx_cmd_bounds.h -- what vgx_command_bounds decides per command and per triangle, and what vgx_pick_commands_boxed adds to
// vgx_pick_commands: host + device. The kernels of vgx_cmd_bounds.hip / vgx_pick_cmds.hip and the host loops of vgx_hosttest.cpp
// (vgxt_command_bounds, vgxt_pick_commands_boxed) call the same functions, so the CPU suite pins the rules without a GPU. The
// specification is in include/vgx.h.
//
// Nothing of the arithmetic is restated: the triangles of a command are vgx_rasterc_triangle, minimum and maximum are taken on the
// order-preserving images of vgx_bounds.h (integer min / max: independent of the order and of the decomposition of the work).
#ifndef VGX_CMD_BOUNDS_H
#define VGX_CMD_BOUNDS_H

#include "vgx_bounds.h"
#include "vgx_raster_cmds.h"
#include "vgx_damage.h"

// A record the call can walk: vgx_rasterc_ranges_valid alone. Type, handle, scissor, clip fields and `reserved` are not examined:
// nothing they name is read
VGX_HD bool vgx_cmdb_valid(const vgx_raster_cmd& c, uint64_t numVertices, uint64_t numIndices) { return vgx_rasterc_ranges_valid(c, numVertices, numIndices); }

// the chunks of 64 consecutive triangles the call walks for the record: none for an invalid one
VGX_HD uint32_t vgx_cmdb_chunks(const vgx_raster_cmd& c, uint64_t numVertices, uint64_t numIndices)
{
	return vgx_cmdb_valid(c, numVertices, numIndices) ? vgx_rasterc_chunks(c) : 0u;
}

// The commands written: [*begin, *end) = [cmd_begin, min(cmd_end, realCmds)), empty when cmd_begin lies at or behind the end
VGX_HD uint32_t vgx_cmdb_range(uint32_t realCmds, uint32_t cmdBegin, uint32_t cmdEnd)
{
	const uint32_t end = cmdEnd < realCmds ? cmdEnd : realCmds;
	return cmdBegin < end ? end - cmdBegin : 0u;
}

// A box as four order-preserving images
struct VgxOrdBox { uint32_t minx, miny, maxx, maxy; };

VGX_HD VgxOrdBox vgx_ordbox_empty() { VgxOrdBox b; b.minx = VGX_ORD_POS_INF; b.miny = VGX_ORD_POS_INF; b.maxx = VGX_ORD_NEG_INF; b.maxy = VGX_ORD_NEG_INF; return b; }
VGX_HD VgxOrdBox vgx_ordbox_union(VgxOrdBox a, VgxOrdBox b)
{
	VgxOrdBox r;
	r.minx = a.minx < b.minx ? a.minx : b.minx; r.miny = a.miny < b.miny ? a.miny : b.miny;
	r.maxx = a.maxx > b.maxx ? a.maxx : b.maxx; r.maxy = a.maxy > b.maxy ? a.maxy : b.maxy;
	return r;
}
VGX_HD VgxOrdBox vgx_ordbox_point(float x, float y)
{
	VgxOrdBox b;
	b.minx = b.maxx = vgx_ord_from_float(x); b.miny = b.maxy = vgx_ord_from_float(y);
	return b;
}

// The box of triangle t of command c over its three corners; the empty box when vgx_rasterc_triangle refuses it
VGX_HD VgxOrdBox vgx_cmdb_triangle(const vgx_raster_cmd& c, const uint16_t* idx, const float* pos, uint32_t t)
{
	uint64_t v[3];
	if (!vgx_rasterc_triangle(c, idx, t, v)) { return vgx_ordbox_empty(); }
	const VgxOrdBox a = vgx_ordbox_point(pos[2 * v[0]], pos[2 * v[0] + 1]), b = vgx_ordbox_point(pos[2 * v[1]], pos[2 * v[1] + 1]);
	return vgx_ordbox_union(vgx_ordbox_union(a, b), vgx_ordbox_point(pos[2 * v[2]], pos[2 * v[2] + 1]));
}

// Does command c exist at the point for vgx_pick_commands_boxed? The closed box of its entry in binary32; a NaN in the entry, and the
// empty box, compare false
VGX_HD bool vgx_cmdb_holds(const float* box, float x, float y) { return box[0] <= x && x <= box[2] && box[1] <= y && y <= box[3]; }

// Does command c take part in vgx_raster_commands_damaged? The tiles its entry reaches over the whole image (vgx_damage_box_tiles: the
// rule the mark calls mark by) hold a set bit
VGX_HD bool vgx_cmdb_damaged(const float* box, const uint32_t* bits, int32_t x0, int32_t y0, uint32_t width, uint32_t height)
{
	VgxRasterRect r;
	if (!vgx_damage_box_tiles(box, x0, y0, width, height, &r)) { return false; }
	return vgx_damage_rect_count(bits, r, vgx_damage_tiles_w(width)) != 0u;
}

// What vgx_command_bounds refuses before anything runs (host only): VGX_OK or VGX_E_INVALID_ARG. color and uv are never read
static inline int vgx_cmdb_check_args(const vgx_raster_streams* sm, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds, uint32_t cmd_begin,
                                      uint32_t cmd_end, const float* bounds, const uint32_t* status)
{
	if (vgx_streams_check(sm, cmds, num_cmds, dev_num_cmds) != VGX_OK) { return VGX_E_INVALID_ARG; }
	if (vgx_cmdb_range(num_cmds, cmd_begin, cmd_end) && !bounds) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)bounds & 15u) || ((uintptr_t)status & 3u)) { return VGX_E_INVALID_ARG; }
	return VGX_OK;
}

#endif
