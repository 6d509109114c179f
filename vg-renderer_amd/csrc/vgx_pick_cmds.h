// vgx_pick_cmds.h -- what vgx_pick_commands decides per command, per triangle and per (command, query): host + device.
// The kernels of vgx_pick_cmds.hip and the host loop of vgx_hosttest.cpp (vgxt_pick_commands) call the same functions, so the CPU suite
// pins the rule without a GPU. The specification is in include/vgx.h (vgx_pick_commands).
//
// Nothing of the arithmetic is restated: the point is vgx_pickf_point, coverage is vgx_raster_setup / vgx_raster_cover, the stamp test
// is vgx_raster_stamp_pass, the triangles of a command are vgx_rasterc_triangle. What is added is the state of a command in FRAME pixels
// (vgx_rasterc_cmd_state is relative to a target and looks at handles; a hit is a statement about geometry and state alone), the
// (command, triangle) limit of a query and the way from a hit triangle to the mesh that owns it.
#ifndef VGX_PICK_CMDS_H
#define VGX_PICK_CMDS_H

#include "vgx_pick.h"
#include "vgx_raster_cmds.h"

#define VGX_PICKC_ALL 0xFFFFFFFFu // vgx_pick_cmd_query::cmd_end: no limit

// Mode (VGX_RF_PLAIN / IN / OUT / STAMP; VGX_RF_INVALID for a record that ends the call with VGX_E_INVALID_ARG), f, n of command c, its
// triangle count and its scissor as frame pixels [rect[0], rect[2]) x [rect[1], rect[3]): the record of vgx_pick_frame, command c
// playing mesh c and draw c. Handles are not looked at: nothing they name is read
VGX_HD void vgx_pickc_cmd_state(const vgx_raster_cmd& c, uint32_t index, uint64_t numVertices, uint64_t numIndices, uint32_t realCmds, VgxPickfMesh* st)
{
	st->mode = VGX_RF_INVALID; st->f = st->n = st->elems = 0u;
	st->rect[0] = st->rect[1] = st->rect[2] = st->rect[3] = 0u;
	if (c.type > 3u || c.reserved != 0u || !vgx_rasterc_ranges_valid(c, numVertices, numIndices)) { return; }
	if (c.clip_first_cmd != VGX_RASTERC_NONE && (uint64_t)c.clip_first_cmd + (uint64_t)c.clip_num_cmds > (uint64_t)realCmds) { return; }
	if (c.type == 3u) {
		st->mode = VGX_RF_STAMP; st->f = index;
	} else if (c.clip_first_cmd == VGX_RASTERC_NONE || c.clip_num_cmds == 0u) {
		st->mode = VGX_RF_PLAIN;
	} else {
		st->mode = c.clip_rule == 0u ? VGX_RF_IN : VGX_RF_OUT;
		st->f = c.clip_first_cmd; st->n = c.clip_num_cmds;
	}
	st->elems = vgx_rasterc_triangles(c);
	st->rect[0] = c.scissor[0]; st->rect[1] = c.scissor[1];
	st->rect[2] = (uint32_t)c.scissor[0] + c.scissor[2]; st->rect[3] = (uint32_t)c.scissor[1] + c.scissor[3];
}

// a query takes part at all: reserved == 0 and a point by vgx_pickf_point
VGX_HD bool vgx_pickc_point(const vgx_pick_cmd_query& q, double* px, double* py, int32_t* X, int32_t* Y)
{
	const bool point = vgx_pickf_point(q.x, q.y, px, py, X, Y);
	return point && q.reserved == 0u;
}

// (c, t) < (cmd_end, tri_end) lexicographically; cmd_end == 0xFFFFFFFF: everything (no command has that index)
VGX_HD bool vgx_pickc_below(uint32_t c, uint32_t t, uint32_t cmdEnd, uint32_t triEnd) { return c < cmdEnd || (c == cmdEnd && t < triEnd); }

// A covering triangle t of command c of mode `mode`, with the OR of "a vertex has alpha 0" in `transparent`: does it count for the
// query? For a clip command always (stamping is the image's, not the query's); else the limit and the transparency rule
VGX_HD bool vgx_pickc_counts(uint32_t mode, uint32_t c, uint32_t t, bool transparent, uint32_t cmdEnd, uint32_t triEnd, uint32_t queryFlags)
{
	if (mode == VGX_RF_STAMP) { return true; }
	return vgx_pickc_below(c, t, cmdEnd, triEnd) && !(transparent && (queryFlags & VGX_PICK_SKIP_TRANSPARENT) != 0u);
}

// Command c of state (mode, f, n) with a counting triangle, under the stamp S the commands below it left: a hit?
VGX_HD bool vgx_pickc_hit(uint32_t mode, uint32_t f, uint32_t n, uint32_t S)
{
	if (mode == VGX_RF_STAMP) { return false; }
	return mode == VGX_RF_PLAIN || vgx_raster_stamp_pass(S, f, n, mode == VGX_RF_IN ? 0u : 1u);
}

// The mesh that owns position p of the index stream: the smallest m with first_index + num_indices > p, provided first_index <= p;
// else 0xFFFFFFFF. Index ranges ascend and are disjoint (the ends do not decrease), so the first such m is found by bisection
VGX_HD uint32_t vgx_pickc_owner(const vgx_mesh* meshes, uint64_t numMeshes, uint64_t p)
{
	uint64_t lo = 0, hi = numMeshes;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (meshes[mid].first_index + (uint64_t)meshes[mid].num_indices > p) { hi = mid; } else { lo = mid + 1u; }
	}
	if (lo >= numMeshes || lo >= 0xFFFFFFFFull || meshes[lo].first_index > p) { return VGX_PICK_NONE; }
	return (uint32_t)lo;
}

// The record of a hit (cmd == 0xFFFFFFFF: none). meshes may be null: no owners
VGX_HD vgx_pick_cmd_hit vgx_pickc_record(uint32_t cmd, uint32_t triangle, const vgx_raster_cmd* cmds, const vgx_mesh* meshes, uint64_t numMeshes)
{
	vgx_pick_cmd_hit h;
	h.cmd = cmd; h.triangle = cmd == VGX_PICK_NONE ? VGX_PICK_NONE : triangle; h.mesh = VGX_PICK_NONE; h.draw = VGX_PICK_NONE;
	if (cmd != VGX_PICK_NONE && meshes) {
		h.mesh = vgx_pickc_owner(meshes, numMeshes, cmds[cmd].first_index + 3ull * triangle);
		if (h.mesh != VGX_PICK_NONE) { h.draw = meshes[h.mesh].draw; }
	}
	return h;
}

// What vgx_pick_commands refuses before anything runs (host only): VGX_OK, VGX_E_INVALID_ARG or VGX_E_RANGE, the latter last
static inline int vgx_pickc_check_args(const vgx_raster_streams* sm, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                                       const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, const vgx_pick_cmd_hit* hits,
                                       const uint32_t* status)
{
	if (vgx_streams_check(sm, cmds, num_cmds, dev_num_cmds) != VGX_OK || (nqueries && (!queries || !hits))) { return VGX_E_INVALID_ARG; }
	if (owners && ((owners->num_meshes && !owners->meshes) || ((uintptr_t)owners->meshes & 7u))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)queries & 7u) || ((uintptr_t)hits & 15u) || ((uintptr_t)status & 3u)) { return VGX_E_INVALID_ARG; }
	if (nqueries > VGX_PICK_MAX_QUERIES) { return VGX_E_RANGE; }
	return VGX_OK;
}

#endif
