// vgx_raster_cmds.h -- what vgx_raster_commands decides per command, per chunk and per triangle BEFORE a pixel is touched: host + device.
// The kernels of vgx_raster_cmds.hip and the host loop of vgx_hosttest.cpp (vgxt_raster_commands) call the same functions, so the CPU
// suite pins the binning -- chunk rectangles, entry counts, per-tile chunk runs -- and not only the pixel rule (vgx_raster.h).
//
// A command is, to the rule, a mesh of kind TRILIST under a draw of its own (include/vgx.h: "command c plays both mesh c and draw c"),
// so its state IS vgx_raster_mesh_state at the painted level; what is new is the validity of the record itself and the chunk.
#ifndef VGX_RASTER_CMDS_H
#define VGX_RASTER_CMDS_H

#include "vgx_raster.h"

#define VGX_RASTERC_CHUNK 64u         // triangles per chunk: one wave sets a chunk up, one lane per triangle
#define VGX_RASTERC_TRIP 4u           // chunk entries a tile's workgroup takes per trip: 4 x 64 triangles = its 256 lanes
#define VGX_RASTERC_NONE 0xFFFFFFFFu  // clip_first_cmd of a command without a region

VGX_HD uint32_t vgx_rasterc_triangles(const vgx_raster_cmd& c) { return c.num_indices / 3u; }
VGX_HD uint32_t vgx_rasterc_chunks(const vgx_raster_cmd& c) { return (vgx_rasterc_triangles(c) + VGX_RASTERC_CHUNK - 1u) / VGX_RASTERC_CHUNK; }

// The ranges of a record lie inside the streams (in 64 bits) and it has at most 65536 vertices: what every call asks before it walks one
VGX_HD bool vgx_rasterc_ranges_valid(const vgx_raster_cmd& c, uint64_t numVertices, uint64_t numIndices)
{
	return c.num_vertices <= 65536u && c.first_vertex <= numVertices && (uint64_t)c.num_vertices <= numVertices - c.first_vertex
	    && c.first_index <= numIndices && (uint64_t)c.num_indices <= numIndices - c.first_index;
}

// The tables a command may name: the streams' sizes, the real command count, the images and the two paint tables (null with a count of
// 0 when the caller gave no paints)
struct VgxRastercTables
{
	uint64_t num_vertices, num_indices;
	uint32_t real_cmds;
	uint32_t has_uv;
	const vgx_raster_image* images; uint32_t num_images;
	const vgx_paint* gradients; uint32_t num_gradients;
	const vgx_paint* patterns; uint32_t num_patterns;
};

// The state of command c of the table: mode (VGX_RF_*; VGX_RF_INVALID for a record that ends the call with VGX_E_INVALID_ARG), region,
// rectangle = the target's scissor cut by the command's, and in `pad` what it is drawn with. Only the records the command names are read
VGX_HD void vgx_rasterc_cmd_state(const vgx_raster_cmd& c, uint32_t index, const VgxRastercTables& tb, int32_t x0, int32_t y0, const uint32_t* scissor,
                                  VgxRasterMeshState* st)
{
	st->mode = VGX_RF_INVALID; st->f = st->n = st->pad = 0u;
	st->rect[0] = st->rect[1] = st->rect[2] = st->rect[3] = 0u;
	if (c.type > 3u || c.reserved != 0u || !vgx_rasterc_ranges_valid(c, tb.num_vertices, tb.num_indices)) { return; }
	if (c.clip_first_cmd != VGX_RASTERC_NONE && (uint64_t)c.clip_first_cmd + (uint64_t)c.clip_num_cmds > (uint64_t)tb.real_cmds) { return; }
	if (c.type == 0u && !tb.has_uv) { return; }
	vgx_mesh me;
	me.first_vertex = c.first_vertex; me.first_index = c.first_index; me.num_vertices = c.num_vertices; me.num_indices = c.num_indices;
	me.draw = index; me.subpath_kind = (uint32_t)VGX_MESH_TRILIST << 28;
	vgx_draw_state ds;
	for (int k = 0; k < 4; ++k) { ds.scissor[k] = c.scissor[k]; }
	ds.clip_rule = c.clip_rule; ds.clip_first_draw = c.clip_first_cmd; ds.clip_num_draws = c.clip_num_cmds; ds.raw_color = 0u;
	vgx_raster_mesh_state(VGX_RL_PAINTED, me, (c.type << 16) | (c.handle & 0xFFFFu), ds, x0, y0, scissor, tb.images, tb.num_images, tb.gradients, tb.num_gradients,
	                      tb.patterns, tb.num_patterns, st);
}

// has the command chunks? (an invalid one, and one both scissors leave nothing of, has none)
VGX_HD uint32_t vgx_rasterc_state_chunks(const vgx_raster_cmd& c, const VgxRasterMeshState& st)
{
	return st.mode == VGX_RF_INVALID || st.mode == VGX_RF_NOTHING ? 0u : vgx_rasterc_chunks(c);
}

// An integer rectangle of tiles under union: empty is tx0 > tx1
VGX_HD VgxRasterRect vgx_rasterc_rect_empty() { VgxRasterRect r; r.tx0 = r.ty0 = 0xFFFFFFFFu; r.tx1 = r.ty1 = 0u; return r; }
VGX_HD bool vgx_rasterc_rect_is_empty(const VgxRasterRect& r) { return r.tx0 > r.tx1; }
VGX_HD uint32_t vgx_rasterc_rect_entries(const VgxRasterRect& r) { return vgx_rasterc_rect_is_empty(r) ? 0u : (r.tx1 - r.tx0 + 1u) * (r.ty1 - r.ty0 + 1u); }
VGX_HD VgxRasterRect vgx_rasterc_rect_union(const VgxRasterRect& a, const VgxRasterRect& b)
{
	VgxRasterRect r;
	r.tx0 = a.tx0 < b.tx0 ? a.tx0 : b.tx0; r.ty0 = a.ty0 < b.ty0 ? a.ty0 : b.ty0;
	r.tx1 = a.tx1 > b.tx1 ? a.tx1 : b.tx1; r.ty1 = a.ty1 > b.ty1 ? a.ty1 : b.ty1;
	return r;
}

// Triangle t of command c: its three vertices in the streams. false: no such triangle, or an index >= num_vertices
VGX_HD bool vgx_rasterc_triangle(const vgx_raster_cmd& c, const uint16_t* idx, uint32_t t, uint64_t* v)
{
	if (t >= vgx_rasterc_triangles(c)) { return false; }
	const uint16_t* ip = idx + c.first_index + 3ull * t;
	const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
	if (i0 >= c.num_vertices || i1 >= c.num_vertices || i2 >= c.num_vertices) { return false; }
	v[0] = c.first_vertex + i0; v[1] = c.first_vertex + i1; v[2] = c.first_vertex + i2;
	return true;
}

// The tiles triangle (a, b, c) can reach inside `rect` (image pixels, half open, not empty): those of its box, when it covers
// anything at all. A NaN gives none
VGX_HD VgxRasterRect vgx_rasterc_triangle_tiles(V2 a, V2 b, V2 c, int32_t x0, int32_t y0, const uint32_t* rect)
{
	VgxRasterTri T;
	uint32_t i0, i1, j0, j1;
	if (!vgx_raster_setup(a, b, c, 0u, 0u, 0u, &T) || !vgx_raster_span(T.minx, T.maxx, x0, rect[0], rect[2], &i0, &i1)
	 || !vgx_raster_span(T.miny, T.maxy, y0, rect[1], rect[3], &j0, &j1)) {
		return vgx_rasterc_rect_empty();
	}
	VgxRasterRect r;
	r.tx0 = i0 / VGX_RASTER_TILE; r.tx1 = i1 / VGX_RASTER_TILE; r.ty0 = j0 / VGX_RASTER_TILE; r.ty1 = j1 / VGX_RASTER_TILE;
	return r;
}

// the status of the call from what the one reduction found (include/vgx.h: RANGE > INVALID_ARG > GROWN)
VGX_HD uint32_t vgx_rasterc_status(uint64_t chunks, uint64_t entries, bool invalid, uint64_t chunkCap, uint64_t entryCap)
{
	uint32_t st = VGX_OK;
	if (chunks > chunkCap || entries > entryCap) { st = VGX_E_GROWN; }
	if (invalid) { st = VGX_E_INVALID_ARG; }
	if (chunks > 0xFFFFFFFFull || entries > 0xFFFFFFFFull) { st = VGX_E_RANGE; }
	return st;
}

#ifdef __HIPCC__
#include "vgx_wave.h"
// ---- the device parts the three command-table families share (vgx_raster_cmds.hip, vgx_pick_cmds.hip, vgx_cmd_bounds.hip) -----------
// The commands a call looks at: the host's count, clamped by the device's when the caller gave one
__device__ __forceinline__ uint32_t vgx_real_cmds(uint32_t num_cmds, const uint32_t* dev_num_cmds)
{
	if (!dev_num_cmds) { return num_cmds; }
	const uint32_t n = *dev_num_cmds;
	return n < num_cmds ? n : num_cmds;
}

// One wave's CONTIGUOUS run [k0, k1) of the `total` chunks (wave w of `waves`, the launch's fixed grid) and its walk over the command
// prefix cmd_first[0 .. n], cmd_first[n] = total: one search for the run's first command, then one load per command passed, where a
// stride over the chunks pays a search and the command's loads for every chunk. Wave-uniform; nothing synchronises the workgroup. The
// kernel works out w and waves: blockDim read in a device function is not folded with the launch bounds and costs a vector load.
// k_pickc_tris and k_cmdb_tris walk this way; k_rasterc_count still strides with a search per chunk, and this is here for it
struct VgxChunkWalk
{
	const uint64_t* cmd_first;
	uint64_t k0, k1;      // k0 >= k1: the wave has no chunk and returns; c, first and next are not set
	uint64_t first, next; // the chunks [first, next) of command c
	uint32_t c;
	__device__ __forceinline__ VgxChunkWalk(const uint64_t* cmdFirst, uint32_t n, uint64_t total, uint64_t w, uint64_t waves) : cmd_first(cmdFirst), first(0), next(0), c(0)
	{
		const uint64_t per = (total + waves - 1u) / waves;
		k0 = w * per < total ? w * per : total; k1 = k0 + per < total ? k0 + per : total;
		if (k0 >= k1) { return; }
		c = (uint32_t)find_owner_u64(cmd_first, 0, n, k0); // the last command whose first chunk is <= k0: the one with chunks
		first = cmd_first[c]; next = cmd_first[c + 1u];
	}
	// to the command of chunk k (k ascends by one); true when it is another one: the caller loads what it keeps per command.
	// cmd_first[n] = total > k, so the walk ends inside the table; commands without chunks are passed over
	__device__ __forceinline__ bool advance(uint64_t k)
	{
		if (k < next) { return false; }
		do { ++c; first = next; next = cmd_first[c + 1u]; } while (k >= next);
		return true;
	}
};
#endif

// ---- the host parts both libraries share -------------------------------------------------------------------------------------------
// A vgx_raster_streams + command-table pair, as vgx_raster_commands, vgx_pick_commands and vgx_command_bounds all ask for it: VGX_OK or
// VGX_E_INVALID_ARG (vgx_raster.h: the order of the checks cannot be observed). uv and uv_bytes are validated whether the call reads them or not
static inline int vgx_streams_check(const vgx_raster_streams* sm, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds)
{
	if (!sm || (num_cmds && !cmds)) { return VGX_E_INVALID_ARG; }
	if ((sm->uv_bytes != 0u && sm->uv_bytes != 4u && sm->uv_bytes != 8u) || (sm->uv != nullptr && sm->uv_bytes == 0u) || sm->reserved != 0u) { return VGX_E_INVALID_ARG; }
	if (sm->uv && ((uintptr_t)sm->uv & (sm->uv_bytes - 1u))) { return VGX_E_INVALID_ARG; }
	if ((sm->num_vertices && (!sm->pos || !sm->color)) || (sm->num_indices && !sm->idx)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)dev_num_cmds & 3u) || ((uintptr_t)cmds & 7u) || ((uintptr_t)sm->pos & 7u) || ((uintptr_t)sm->color & 3u) || ((uintptr_t)sm->idx & 1u)) { return VGX_E_INVALID_ARG; }
	return VGX_OK;
}

// What vgx_raster_commands refuses before anything runs: VGX_OK or VGX_E_INVALID_ARG
static inline int vgx_rasterc_check_args(const vgx_raster_streams* sm, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                                         const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target,
                                         const uint32_t* status)
{
	if (vgx_streams_check(sm, cmds, num_cmds, dev_num_cmds) != VGX_OK || vgx_target_check(target) != VGX_OK) { return VGX_E_INVALID_ARG; }
	if (paints) {
		if ((paints->num_gradients && !paints->gradients) || (paints->num_patterns && !paints->patterns)) { return VGX_E_INVALID_ARG; }
		if (((uintptr_t)paints->gradients & 3u) || ((uintptr_t)paints->patterns & 3u)) { return VGX_E_INVALID_ARG; }
	}
	if ((num_images && !images) || ((uintptr_t)images & 7u) || ((uintptr_t)status & 3u)) { return VGX_E_INVALID_ARG; }
	return VGX_OK;
}

// vgx_submit_order (include/vgx.h): host code of libvgx.so; stated here so that the host test library carries the same text
static inline int vgx_rasterc_submit_order(const vgx_raster_cmd* draw_cmds, uint32_t ndraw, const vgx_raster_cmd* clip_cmds, uint32_t nclip, vgx_raster_cmd* out,
                                           uint32_t cap, uint32_t* num_out)
{
	if (!num_out || (ndraw && !draw_cmds) || (nclip && !clip_cmds) || (cap && !out)) { return VGX_E_INVALID_ARG; }
	uint64_t n = 0;
	uint32_t prev = VGX_RASTERC_NONE, landed = VGX_RASTERC_NONE;
	for (uint32_t k = 0; k < ndraw; ++k) {
		vgx_raster_cmd c = draw_cmds[k];
		if (c.clip_first_cmd != VGX_RASTERC_NONE && (uint64_t)c.clip_first_cmd + (uint64_t)c.clip_num_cmds > (uint64_t)nclip) { return VGX_E_INVALID_ARG; }
		if (c.clip_first_cmd != prev) {
			prev = c.clip_first_cmd;
			landed = VGX_RASTERC_NONE;
			if (c.clip_first_cmd != VGX_RASTERC_NONE && c.clip_num_cmds > 0u) {
				landed = (uint32_t)n;
				for (uint32_t j = 0; j < c.clip_num_cmds; ++j, ++n) {
					if (n < cap) {
						out[n] = clip_cmds[c.clip_first_cmd + j];
						out[n].type = 3u; out[n].clip_first_cmd = VGX_RASTERC_NONE; out[n].clip_num_cmds = 0u;
					}
				}
			}
		}
		if (c.clip_first_cmd != VGX_RASTERC_NONE && c.clip_num_cmds > 0u) { c.clip_first_cmd = landed; }
		if (n < cap) { out[n] = c; }
		++n;
	}
	*num_out = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
	return n > cap ? VGX_E_NOSPACE : VGX_OK;
}

#endif
