// vgx_raster_cmds.hip -- a draw-command table to an RGBA8 image on gfx950 (include/vgx.h: vgx_raster_commands; the arithmetic: vgx_raster.h,
// the binning rules: vgx_raster_cmds.h), and vgx_raster_cmds_from_assembly, which writes such a table from the product's assembled frame.
//
// The families of vgx_raster.hip bin by MESH: every tile a mesh's box reaches sets up all its triangles. A draw command is a mesh of
// tens of thousands of triangles, so this family (k_rasterc_*) bins CHUNKS of 64 consecutive triangles of one command. The launch
// sequence stays count, scan, entries, sort, tiles, with one scan in front that turns commands into chunks:
//   k_rasterc_cmds     one lane per command (grid-stride: the real count may live on the device): what the command does
//                      (vgx_rasterc_cmd_state: validity of the record, stamp / test In / test Out / untested / nothing, its region, the
//                      target's scissor cut by its own, sampled / gradient / pattern and the handle), kept per command
//   scan OpRastercCmds every command's first chunk, the chunk total, and the mark of an invalid command
//   k_rasterc_count    one WAVE per chunk (grid-stride), one lane per triangle: three indices, three positions, vgx_raster_setup and the
//                      two vgx_raster_span calls against the command's rectangle -> a rectangle of tiles; a wave min / max reduction of
//                      the integer rectangles gives the chunk's rectangle (16 bytes) and its command. Chunks behind the scratch's
//                      capacity are still counted (one atomic add of their entries), so that the need the mirror carries is exact
//   scan OpRastercBin  every chunk's first entry. finish() is where the call decides ON THE DEVICE: VGX_E_RANGE > VGX_E_INVALID_ARG >
//                      VGX_E_GROWN. Every kernel behind it looks at the state word and does nothing unless it says VGX_OK
//   k_rasterc_entries  one lane per chunk writes its entries, key = tile, value = global chunk ordinal (ascending in (command, chunk));
//                      the sentinel behind the total; one bit per tile a painted command reaches
//   radix_sort_pairs   rocprim's, stable, on the bits of the sentinel: every tile's run stays ascending
//   k_rasterc_tiles    <PAINT>: the hot path. The workgroup finds its run and takes FOUR chunk entries per trip: lane tid takes triangle
//                      tid & 63 of chunk tid >> 6 -- no prefix of triangle counts, no search. Setup once, then the ordered compaction
//                      of k_raster_tiles (ballot + per-wave prefix, the wave counts through LDS) and the pixel walk with the lane
//                      functions of vgx_raster.h; d and the stamp S live in registers across the trips. Per-command state is kept for
//                      the four slots of a trip. A tile a painted command reaches runs <true>, every other tile <false>, which
//                      carries no paint code (DESIGN.md has the resource report).
// vgx_raster_commands_damaged runs the DAMAGE instantiations of the same kernels (k_rasterc_cmds: the box test; count, scan and
// entries: marked tiles only; tiles: an unmarked tile returns ahead of the clear); vgx_raster_commands keeps those without it.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_raster_cmds.h"
#include "vgx_damage.h"
#include "vgx_cmd_bounds.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {

__device__ __forceinline__ VgxRastercTables rasterc_tables(const VgxRasterCmdArgs& A, uint32_t real)
{
	VgxRastercTables tb;
	tb.num_vertices = A.num_vertices; tb.num_indices = A.num_indices; tb.real_cmds = real; tb.has_uv = A.uv != nullptr ? 1u : 0u;
	tb.images = A.images; tb.num_images = A.num_images;
	tb.gradients = A.gradients; tb.num_gradients = A.num_gradients; tb.patterns = A.patterns; tb.num_patterns = A.num_patterns;
	return tb;
}

// DAMAGE (vgx_raster_commands_damaged; vgx_raster_commands runs the instantiations without it, which hold none of its code): a bin
// entry is a pair of a chunk and a MARKED tile (A.damage, vgx_damage.h), an unmarked tile is left alone ahead of the clear, and with
// A.cmd_bounds a VALID command whose box reaches no marked tile does nothing: no chunks, so the count pass never reads its triangles.
// An invalid record stays invalid whatever its box says
template <bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterc_cmds(VgxRasterCmdArgs A)
{
	const uint32_t n = vgx_real_cmds(A.num_cmds, A.dev_num_cmds);
	const VgxRastercTables tb = rasterc_tables(A, n);
	for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) {
		VgxRasterMeshState st;
		vgx_rasterc_cmd_state(A.cmds[c], (uint32_t)c, tb, A.x0, A.y0, A.scissor, &st);
		if (DAMAGE && A.cmd_bounds && st.mode != VGX_RF_INVALID && st.mode != VGX_RF_NOTHING) {
			const float4 b = *(const float4*)(A.cmd_bounds + 4ull * c);
			const float box[4] = { b.x, b.y, b.z, b.w };
			if (!vgx_cmdb_damaged(box, A.damage, A.x0, A.y0, A.width, A.height)) { st.mode = VGX_RF_NOTHING; }
		}
		A.cmd_state[c] = st;
	}
}

// the bin entries of a chunk whose triangles reach the tiles of r
template <bool DAMAGE>
__device__ __forceinline__ uint32_t rasterc_entries_of(const VgxRasterCmdArgs& A, const VgxRasterRect& r)
{
	return DAMAGE ? vgx_damage_rect_count(A.damage, r, A.tiles_w) : vgx_rasterc_rect_entries(r);
}

struct OpRastercCmds
{
	VgxRasterCmdArgs A;
	__device__ uint64_t size() const { return vgx_real_cmds(A.num_cmds, A.dev_num_cmds); }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const VgxRasterMeshState st = A.cmd_state[i];
		r.a = vgx_rasterc_state_chunks(A.cmds[i], st);
		r.c = st.mode == VGX_RF_INVALID ? 1u : 0u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { A.cmd_first[i] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		const uint32_t n = vgx_real_cmds(A.num_cmds, A.dev_num_cmds);
		A.cmd_first[n] = t.a;
		A.state[VGX_RASC_CHUNKS] = t.a; A.state[VGX_RASC_INVALID] = t.c; A.state[VGX_RASC_BEYOND] = 0ull; A.state[VGX_RASC_CMDS] = n;
	}
};

template <bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterc_count(VgxRasterCmdArgs A)
{
	const uint64_t total = A.state[VGX_RASC_CHUNKS];
	if (total > 0xFFFFFFFFull) { return; } // VGX_E_RANGE by the chunks alone
	const uint32_t n = (uint32_t)A.state[VGX_RASC_CMDS];
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / VGX_WAVE);
	// a stride over the chunks with a search per chunk; VgxChunkWalk (vgx_raster_cmds.h) is the contiguous walk, should this move to it
	for (uint64_t k = (uint64_t)blockIdx.x * (blockDim.x / VGX_WAVE) + (threadIdx.x / VGX_WAVE); k < total; k += waves) { // wave-uniform
		const uint32_t c = (uint32_t)find_owner_u64(A.cmd_first, 0, n, k); // the last command whose first chunk is <= k: the one with chunks
		const vgx_raster_cmd cmd = A.cmds[c];
		const VgxRasterMeshState st = A.cmd_state[c];
		const uint32_t t = (uint32_t)(k - A.cmd_first[c]) * VGX_RASTERC_CHUNK + (uint32_t)lane;
		VgxRasterRect r = vgx_rasterc_rect_empty();
		uint64_t v[3];
		if (vgx_rasterc_triangle(cmd, A.idx, t, v)) {
			const float2* pp = (const float2*)A.pos;
			const float2 p0 = pp[v[0]], p1 = pp[v[1]], p2 = pp[v[2]];
			r = vgx_rasterc_triangle_tiles(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), A.x0, A.y0, st.rect);
		}
		r.tx0 = wave_min_u32(r.tx0); r.ty0 = wave_min_u32(r.ty0); r.tx1 = wave_max_u32(r.tx1); r.ty1 = wave_max_u32(r.ty1);
		if (lane == 0) {
			if (k < A.chunk_cap) { A.chunk_rect[k] = r; A.chunk_cmd[k] = c; }
			else { atomicAdd(&A.state[VGX_RASC_BEYOND], (unsigned long long)rasterc_entries_of<DAMAGE>(A, r)); }
		}
	}
}

__device__ __forceinline__ uint64_t rasterc_stored_chunks(const VgxRasterCmdArgs& A)
{
	const uint64_t total = A.state[VGX_RASC_CHUNKS];
	return total > 0xFFFFFFFFull ? 0ull : (total < A.chunk_cap ? total : A.chunk_cap);
}

template <bool DAMAGE>
struct OpRastercBin
{
	VgxRasterCmdArgs A;
	__device__ uint64_t size() const { return rasterc_stored_chunks(A); }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		r.a = rasterc_entries_of<DAMAGE>(A, A.chunk_rect[i]);
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { A.chunk_first[i] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		const uint64_t chunks = A.state[VGX_RASC_CHUNKS], entries = t.a + A.state[VGX_RASC_BEYOND];
		const uint32_t st = vgx_rasterc_status(chunks, entries, A.state[VGX_RASC_INVALID] != 0ull, A.chunk_cap, A.entry_cap);
		A.state[VGX_RASC_STATUS] = st; A.state[VGX_RASC_ENTRIES] = entries;
		if (A.status) { *A.status = st; }
	}
};

template <bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterc_entries(VgxRasterCmdArgs A)
{
	if (A.state[VGX_RASC_STATUS] != VGX_OK) { return; }
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	// the unused tail of what the sort will look at
	if (k >= A.state[VGX_RASC_ENTRIES] && k < A.sort_n) { A.keys[k] = A.sentinel; A.vals[k] = 0u; }
	if (k >= A.state[VGX_RASC_CHUNKS]) { return; } // <= chunk_cap: checked by finish()
	const VgxRasterRect r = A.chunk_rect[k];
	if (vgx_rasterc_rect_is_empty(r)) { return; }
	uint64_t at = A.chunk_first[k]; // + the chunk's entries <= the total <= entry_cap: checked by finish()
	for (uint32_t ty = r.ty0; ty <= r.ty1; ++ty) {
		for (uint32_t tx = r.tx0; tx <= r.tx1; ++tx) {
			const uint32_t key = ty * A.tiles_w + tx;
			if (DAMAGE && !vgx_damage_bit(A.damage, key)) { continue; } // as many pass as the scan found: the bits do not change under the call
			A.keys[at] = key; A.vals[at] = (uint32_t)k;
			++at;
		}
	}
	if (A.cmd_state[A.chunk_cmd[k]].pad & VGX_RT_PAINTED) { mark_tiles(A.tile_paint, r, A.tiles_w); }
}

// 168 bytes: the setup record; its chunk's slot | mode << 8 | VGX_RT_SAMPLED / VGX_RT_GRADIENT / VGX_RT_PATTERN; the command's rectangle in
// this tile as a mask of columns (bits 0 .. 15) and of rows (bits 16 .. 31); the three UVs of a sampled triangle
struct VgxRastercTri { VgxRasterTri T; uint32_t slot_mode, mask; double uv[6]; };
// the chunk in hand of slot s: where its triangles are and what its command does in this tile
struct VgxRastercSlot
{
	uint64_t first_vertex, first_index;                // of the command
	uint32_t num_vertices, tri0, tri1;                 // the chunk's triangles [tri0, tri1) of the command
	uint32_t mode_rect, f, n, flags;                   // mode << 20 | y1 << 15 | x1 << 10 | y0 << 5 | x0, tile-local, half open
};

struct VgxRastercTexelFetch
{
	const uint32_t* pixels; uint32_t stride;
	__device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return pixels[(uint64_t)y * stride + x]; }
};

// what a slot keeps of the table it names: the image of a sampled command, or with PAINT the paint record (whose image part serves a sampled one)
template <bool PAINT> struct RastercPaintSlot { typedef vgx_raster_image type; };
template <> struct RastercPaintSlot<true> { typedef VgxRasterPaint type; };
__device__ __forceinline__ vgx_raster_image& slot_image(vgx_raster_image& s) { return s; }
__device__ __forceinline__ vgx_raster_image& slot_image(VgxRasterPaint& s) { return s.im; }

template <bool PAINT, bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterc_tiles(VgxRasterCmdArgs A)
{
	typedef typename RastercPaintSlot<PAINT>::type Paint;
	__shared__ VgxRastercTri s_tri[256];
	__shared__ VgxRastercSlot s_slot[VGX_RASTERC_TRIP];
	__shared__ Paint s_paint[VGX_RASTERC_TRIP]; // written for the sampled and the painted slots only, and not read for the others
	__shared__ uint32_t s_count[4];
	if (A.state[VGX_RASC_STATUS] != VGX_OK) { return; }
	const uint32_t tx = A.tile_x0 + blockIdx.x, ty = A.tile_y0 + blockIdx.y;
	const uint32_t key = ty * A.tiles_w + tx;
	if (DAMAGE && !vgx_damage_bit(A.damage, key)) { return; } // block-uniform, ahead of the clear: the tile is not redrawn
	if ((((A.tile_paint[key >> 5] >> (key & 31u)) & 1u) != 0u) != PAINT) { return; } // block-uniform: the tile of the other instantiation
	const uint32_t tid = threadIdx.x;
	const int lane = tid & (VGX_WAVE - 1);
	const uint32_t wave = tid >> 6;
	const uint32_t lx = tid & 15u, ly = tid >> 4;
	const uint32_t ox = tx * VGX_RASTER_TILE, oy = ty * VGX_RASTER_TILE;
	const uint32_t i = ox + lx, j = oy + ly;
	const bool inside = i >= A.scissor[0] && i < A.scissor[2] && j >= A.scissor[1] && j < A.scissor[3];
	const uint32_t r0 = lower_bound_u32(A.sorted_keys, (uint32_t)A.sort_n, key), r1 = lower_bound_u32(A.sorted_keys, (uint32_t)A.sort_n, key + 1u);
	const bool clear = (A.flags & VGX_RASTER_CLEAR) != 0;
	if (r0 == r1 && !clear) { return; } // block-uniform
	uint32_t* const pixel = A.pixels + (uint64_t)j * A.stride + i;
	const uint32_t before = inside ? (clear ? A.clear_color : *pixel) : 0u;
	uint32_t d = before;
	uint32_t S = VGX_RASTER_STAMP_NONE;
	const double px = (double)(A.x0 + (int32_t)i) + 0.5, py = (double)(A.y0 + (int32_t)j) + 0.5;
	for (uint32_t eb = r0; eb < r1; eb += VGX_RASTERC_TRIP) { // block-uniform loops throughout
		const uint32_t ne = min(VGX_RASTERC_TRIP, r1 - eb);
		if (tid < ne) {
			const uint32_t k = A.sorted_vals[eb + tid];
			const uint32_t c = A.chunk_cmd[k];
			const vgx_raster_cmd cmd = A.cmds[c];
			const VgxRasterMeshState ms = A.cmd_state[c];
			VgxRastercSlot sl;
			sl.first_vertex = cmd.first_vertex; sl.first_index = cmd.first_index; sl.num_vertices = cmd.num_vertices;
			sl.tri0 = (uint32_t)((uint64_t)k - A.cmd_first[c]) * VGX_RASTERC_CHUNK;
			sl.tri1 = min(sl.tri0 + VGX_RASTERC_CHUNK, vgx_rasterc_triangles(cmd));
			// the command's rectangle cut to this tile (an entry means a triangle's box reaches the tile inside the rectangle: not empty)
			const uint32_t cx0 = max(ox, ms.rect[0]), cx1 = min(ox + VGX_RASTER_TILE, ms.rect[2]);
			const uint32_t cy0 = max(oy, ms.rect[1]), cy1 = min(oy + VGX_RASTER_TILE, ms.rect[3]);
			sl.f = ms.f; sl.n = ms.n;
			sl.mode_rect = cx0 < cx1 && cy0 < cy1 ? (ms.mode << 20) | ((cy1 - oy) << 15) | ((cx1 - ox) << 10) | ((cy0 - oy) << 5) | (cx0 - ox) : (uint32_t)VGX_RF_NOTHING << 20;
			sl.flags = 0u;
			// handles and records are inside their tables and valid: k_rasterc_cmds
			if (ms.pad & VGX_RT_SAMPLED) { sl.flags = VGX_RT_SAMPLED; slot_image(s_paint[tid]) = A.images[ms.pad & 0xFFFFu]; }
			if constexpr (PAINT) {
				if (ms.pad & VGX_RT_PAINTED) {
					const bool grad = (ms.pad & VGX_RT_GRADIENT) != 0u;
					sl.flags = grad ? VGX_RT_GRADIENT : VGX_RT_PATTERN;
					VgxRasterPaint rec;
					vgx_raster_paint_record((grad ? A.gradients : A.patterns)[ms.pad & 0xFFFFu], A.images, &rec);
					s_paint[tid] = rec;
				}
			}
			s_slot[tid] = sl;
		}
		__syncthreads();
		bool keep = false;
		VgxRastercTri R;
		if (wave < ne) {
			const VgxRastercSlot sl = s_slot[wave];
			const uint32_t mr = sl.mode_rect, mode = mr >> 20;
			const uint32_t t = sl.tri0 + (uint32_t)lane;
			if (mode != VGX_RF_NOTHING && t < sl.tri1) {
				const uint16_t* ip = A.idx + sl.first_index + 3ull * t;
				const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
				if (i0 < sl.num_vertices && i1 < sl.num_vertices && i2 < sl.num_vertices) {
					const float2* pp = (const float2*)A.pos + sl.first_vertex;
					const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
					uint32_t c0 = 0u, c1 = 0u, c2 = 0u; // a clip command's colours are not read
					if (mode != VGX_RF_STAMP) { const uint32_t* cp = A.color + sl.first_vertex; c0 = cp[i0]; c1 = cp[i1]; c2 = cp[i2]; }
					uint32_t a0, a1, b0, b1;
					const uint32_t cols = ((1u << ((mr >> 10) & 31u)) - 1u) & ~((1u << (mr & 31u)) - 1u), rows = ((1u << ((mr >> 15) & 31u)) - 1u) & ~((1u << ((mr >> 5) & 31u)) - 1u);
					R.slot_mode = wave | (mode << 8) | sl.flags; R.mask = cols | (rows << 16);
					keep = vgx_raster_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), c0, c1, c2, &R.T)
					    && vgx_raster_span(R.T.minx, R.T.maxx, A.x0, ox + (mr & 31u), ox + ((mr >> 10) & 31u), &a0, &a1)
					    && vgx_raster_span(R.T.miny, R.T.maxy, A.y0, oy + ((mr >> 5) & 31u), oy + ((mr >> 15) & 31u), &b0, &b1);
					if (keep && (sl.flags & VGX_RT_SAMPLED)) {
						vgx_raster_uv_widen(A.uv, A.uv_bytes, sl.first_vertex + i0, R.uv);
						vgx_raster_uv_widen(A.uv, A.uv_bytes, sl.first_vertex + i1, R.uv + 2);
						vgx_raster_uv_widen(A.uv, A.uv_bytes, sl.first_vertex + i2, R.uv + 4);
					}
				}
			}
		}
		const uint64_t kept = wave_ballot(keep);
		if (lane == 0) { s_count[wave] = (uint32_t)__popcll(kept); }
		__syncthreads();
		uint32_t base = 0, n = 0;
#pragma unroll
		for (uint32_t w = 0; w < 4u; ++w) { const uint32_t c = s_count[w]; base += w < wave ? c : 0u; n += c; }
		if (keep) {
			VgxRastercTri* const dst = &s_tri[base + (uint32_t)__popcll(kept & lanemask_lt(lane))];
			dst->T = R.T; dst->slot_mode = R.slot_mode; dst->mask = R.mask;
			if (R.slot_mode & VGX_RT_SAMPLED) {
#pragma unroll
				for (int c = 0; c < 6; ++c) { dst->uv[c] = R.uv[c]; }
			}
		}
		__syncthreads();
		for (uint32_t t = 0; t < n; ++t) { // every lane walks the records: no lane leaves between the barriers
			const VgxRastercTri& rec = s_tri[t];
			const uint32_t mk = rec.mask;
			if (((mk >> lx) & (mk >> (16u + ly)) & 1u) != 0u) {
				const uint32_t sm = rec.slot_mode;
				const uint32_t mode = (sm >> 8) & 255u;
				uint32_t f = 0u, nn = 0u;
				if (mode != VGX_RF_PLAIN) { f = s_slot[sm & 3u].f; nn = s_slot[sm & 3u].n; }
				if (sm & VGX_RT_SAMPLED) {
					const vgx_raster_image im = slot_image(s_paint[sm & 3u]);
					VgxRastercTexelFetch fetch;
					fetch.pixels = im.pixels; fetch.stride = im.stride;
					d = vgx_raster_textured_pixel(rec.T, rec.uv, im, mode, f, nn, px, py, S, d, fetch);
				} else {
					bool painted = false;
					if constexpr (PAINT) {
						if (sm & VGX_RT_GRADIENT) {
							d = vgx_raster_gradient_pixel(rec.T, s_paint[sm & 3u], mode, f, nn, px, py, S, d);
							painted = true;
						} else if (sm & VGX_RT_PATTERN) {
							const VgxRasterPaint pr = s_paint[sm & 3u];
							VgxRastercTexelFetch fetch;
							fetch.pixels = pr.im.pixels; fetch.stride = pr.im.stride;
							d = vgx_raster_pattern_pixel(rec.T, pr, mode, f, nn, px, py, S, d, fetch);
							painted = true;
						}
					}
					if (!painted) { d = vgx_raster_frame_pixel(rec.T, mode, f, nn, px, py, &S, d); }
				}
			}
		}
		__syncthreads(); // s_tri, s_count and the slots are written again
	}
	if (inside && (clear || d != before)) { *pixel = d; }
}

// ---- vgx_raster_cmds_from_assembly --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t asm_real_cmds(const VgxCmdsFromAsmArgs& a)
{
	if (!a.dev_num_drawcmds) { return a.cap_drawcmds; }
	const uint64_t n = *a.dev_num_drawcmds;
	return n < a.cap_drawcmds ? n : a.cap_drawcmds;
}

// the draw of command k: that of its first mesh. 0xFFFFFFFF for a first_mesh outside the table (the command's own lane reports it)
__device__ __forceinline__ uint32_t asm_cmd_draw(const VgxCmdsFromAsmArgs& a, uint64_t k)
{
	const uint64_t m = a.drawcmds[k].first_mesh;
	return m < a.num_meshes ? a.meshes[m].draw : 0xFFFFFFFFu;
}

// the first command of [0, n) whose draw is >= d, else n (the draws do not decrease over the table)
__device__ __forceinline__ uint64_t asm_first_cmd_of_draw(const VgxCmdsFromAsmArgs& a, uint64_t n, uint64_t d)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if ((uint64_t)asm_cmd_draw(a, mid) < d) { lo = mid + 1u; } else { hi = mid; }
	}
	return lo;
}

// the flagged reduction over the frame's meshes: a contour mesh is no list of triangles
__global__ __launch_bounds__(256) void k_raster_cmds_meshes(VgxCmdsFromAsmArgs a)
{
	bool bad = false;
	for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < a.num_meshes; m += (uint64_t)gridDim.x * blockDim.x) {
		bad = bad || vgx_raster_kind_is_contours(a.meshes[m].subpath_kind);
	}
	if (bad) { atomicOr(a.flag, 1u); }
}

__global__ __launch_bounds__(256) void k_raster_cmds_from_assembly(VgxCmdsFromAsmArgs a)
{
	const uint64_t n = asm_real_cmds(a);
	for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
		const vgx_drawcmd dc = a.drawcmds[k];
		vgx_raster_cmd c;
		c.first_vertex = dc.first_vertex; c.first_index = dc.first_index; c.num_vertices = dc.num_vertices; c.num_indices = dc.num_indices;
		c.type = vgx_raster_draw_type(dc.state_key); c.handle = dc.state_key & 0xFFFFu;
		c.scissor[0] = c.scissor[1] = c.scissor[2] = c.scissor[3] = 0;
		c.clip_rule = 0u; c.clip_first_cmd = VGX_RASTERC_NONE; c.clip_num_cmds = 0u; c.reserved = 0u;
		const uint32_t d = asm_cmd_draw(a, k);
		if (dc.first_mesh >= a.num_meshes || d >= a.num_draws) {
			atomicOr(a.flag, 1u);
		} else {
			const vgx_draw_state ds = a.draw_state[d];
			for (int q = 0; q < 4; ++q) { c.scissor[q] = ds.scissor[q]; }
			c.clip_rule = ds.clip_rule;
			if (ds.clip_first_draw != VGX_RASTER_STAMP_NONE && ds.clip_num_draws != 0u) {
				const uint64_t first = asm_first_cmd_of_draw(a, n, ds.clip_first_draw);
				const uint64_t end = asm_first_cmd_of_draw(a, n, (uint64_t)ds.clip_first_draw + ds.clip_num_draws);
				c.clip_first_cmd = (uint32_t)first; c.clip_num_cmds = (uint32_t)(end - first);
			}
		}
		a.out[k] = c;
	}
}

__global__ void k_raster_cmds_finish(VgxCmdsFromAsmArgs a)
{
	*a.dev_num_cmds = (uint32_t)asm_real_cmds(a);
	if (a.status) { *a.status = *a.flag ? (uint32_t)VGX_E_INVALID_ARG : (uint32_t)VGX_OK; }
}

} // namespace

namespace {

template <bool DAMAGE>
hipError_t launch_commands(const VgxRasterCmdArgs& a, void* partial, void* sortTemp, size_t sortBytes, hipStream_t s)
{
	if (a.num_cmds) {
		const uint64_t blocks = ((uint64_t)a.num_cmds + 255u) / 256u;
		hipLaunchKernelGGL(k_rasterc_cmds<DAMAGE>, dim3((unsigned)(blocks < 1024u ? blocks : 1024u)), dim3(256), 0, s, a);
	}
	const OpRastercCmds cmds = { a };
	vgx_device_scan(cmds, (Sum3*)partial, s, a.num_cmds);
	if (a.num_cmds) { // the chunk count lives on the device: a fixed grid of waves, each striding over the chunks
		const uint64_t blocks = (a.chunk_cap + 3u) / 4u;
		hipLaunchKernelGGL(k_rasterc_count<DAMAGE>, dim3((unsigned)(blocks < 1u ? 1u : (blocks < 4096u ? blocks : 4096u))), dim3(256), 0, s, a);
	}
	const OpRastercBin<DAMAGE> bin = { a };
	vgx_device_scan(bin, (Sum3*)partial, s, a.chunk_cap);
	const uint64_t items = a.chunk_cap > a.sort_n ? a.chunk_cap : a.sort_n;
	if (items) { hipLaunchKernelGGL(k_rasterc_entries<DAMAGE>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a); }
	if (a.sort_n) {
		const hipError_t e = rocprim::radix_sort_pairs(sortTemp, sortBytes, (const uint32_t*)a.keys, a.sorted_keys, (const uint32_t*)a.vals, a.sorted_vals,
		                                               (size_t)a.sort_n, 0u, a.sort_bits, s);
		if (e != hipSuccess) { return e; }
	}
	if (a.tiles_x && a.tiles_y) {
		hipLaunchKernelGGL((k_rasterc_tiles<false, DAMAGE>), dim3(a.tiles_x, a.tiles_y), dim3(256), 0, s, a);
		if (a.num_gradients || a.num_patterns) { hipLaunchKernelGGL((k_rasterc_tiles<true, DAMAGE>), dim3(a.tiles_x, a.tiles_y), dim3(256), 0, s, a); }
	}
	return hipSuccess;
}

} // namespace

// a.damage set: vgx_raster_commands_damaged
hipError_t vgx_launch_raster_commands(const VgxRasterCmdArgs& a, void* partial, void* sortTemp, size_t sortBytes, hipStream_t s)
{
	return a.damage ? launch_commands<true>(a, partial, sortTemp, sortBytes, s) : launch_commands<false>(a, partial, sortTemp, sortBytes, s);
}

void vgx_launch_cmds_from_assembly(const VgxCmdsFromAsmArgs& a, hipStream_t s)
{
	if (a.num_meshes) {
		const uint64_t blocks = (a.num_meshes + 255u) / 256u;
		hipLaunchKernelGGL(k_raster_cmds_meshes, dim3((unsigned)(blocks < 1024u ? blocks : 1024u)), dim3(256), 0, s, a);
	}
	if (a.cap_drawcmds) {
		const uint64_t blocks = (a.cap_drawcmds + 255u) / 256u;
		hipLaunchKernelGGL(k_raster_cmds_from_assembly, dim3((unsigned)(blocks < 1024u ? blocks : 1024u)), dim3(256), 0, s, a);
	}
	hipLaunchKernelGGL(k_raster_cmds_finish, dim3(1), dim3(1), 0, s, a);
}
