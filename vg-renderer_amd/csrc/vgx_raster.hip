// vgx_raster.hip -- a frame's mesh streams to an RGBA8 image on gfx950 (include/vgx.h: vgx_raster, vgx_raster_frame, vgx_raster_textured,
// vgx_raster_painted, vgx_raster_concave; the arithmetic: vgx_raster.h). Two kernel families and one launch sequence (count, scan, entries,
// sort, tiles): the plain family (k_raster_*) serves vgx_raster and carries no draw state, which measurably keeps it the faster one; the
// frame family (k_rasterf_*, further down) serves the four frame-level calls, which differ in a level carried in the arguments, and
// vgx_raster_damaged, the concave level restricted to the tiles of a damage bitmap (the DAMAGE instantiations; vgx_damage.h).
//
// Blending is not commutative: a pixel must see its triangles in ascending (mesh, triangle) order, and no atomic on a pixel gives
// that. So a pixel belongs to ONE lane for the whole call: the image is cut into tiles of 16 x 16 pixels, a tile is one workgroup of
// 256 lanes, and the work in front of the tile kernel only finds, per tile, the meshes that can reach it, in ascending order.
//   k_raster_count    one lane per mesh of the range: the mesh's box (vgx_mesh_bounds) clipped to image and scissor -> a rectangle of
//                     tiles -> its number of (tile, mesh) entries and its triangles
//   scan OpRasterBin  (vgx_scan.h) every mesh's first entry and the totals. finish() is where the call decides ON THE DEVICE: more
//                     entries than the scratch holds -> VGX_E_GROWN, more than 2^32 - 1 entries or triangles -> VGX_E_RANGE. Every
//                     kernel behind it looks at the state word and does nothing unless it says VGX_OK, the clear included
//   k_raster_entries  one lane per mesh writes its entries, key = tile number, value = mesh: ascending by mesh. One lane per slot of
//                     the sorted range behind the total writes the sentinel key (the entry count is known on the device only)
//   radix_sort_pairs  rocprim's, on bits [0, bits of the sentinel): stable, so every tile's run stays ascending by mesh
//   k_raster_tiles    the hot path. The workgroup finds its run by two searches in the sorted keys, takes the run's meshes 256 at a
//                     time (mesh records -> exclusive scan of their triangle counts in LDS) and the triangles of those meshes 256 at
//                     a time, whatever mesh they belong to: a lane finds its triangle's mesh by a search in the LDS prefix, loads
//                     three uint16 indices, three positions and three colours, does the setup once (orientation, the three canonical
//                     edges, tie flags, box) and tests the box against the tile; the survivors are compacted IN ORDER (ballot + prefix
//                     count per wave, the wave counts through LDS) into 104-byte setup records in LDS. Then every pixel lane walks the
//                     records in LDS order -- all lanes read the same address, a broadcast -- with coverage, colour and blend in
//                     registers. The pixel is read once (after the clear decision) and written once, when something changed.
// No host round trip, nothing comes back but the status and, through the context's pinned mirror, the entry count for the next call.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_raster.h"
#include "vgx_damage.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace {

__device__ __forceinline__ bool raster_rect(const VgxRasterArgs& A, uint64_t k, VgxRasterRect* r)
{
	const uint64_t m = A.mesh_begin + k;
	const float4 box = ((const float4*)A.mesh_bounds)[m];
	const float b[4] = { box.x, box.y, box.z, box.w };
	return vgx_raster_mesh_tiles(A.meshes[m], b, A.x0, A.y0, A.scissor, VGX_RL_PLAIN, r);
}

__global__ __launch_bounds__(256) void k_raster_count(VgxRasterArgs A)
{
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= A.nrange) { return; }
	VgxRasterRect r;
	A.mesh_entries[k] = raster_rect(A, k, &r) ? (r.tx1 - r.tx0 + 1u) * (r.ty1 - r.ty0 + 1u) : 0u;
}

struct OpRasterBin
{
	VgxRasterArgs A;
	__device__ uint64_t size() const { return A.nrange; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		r.a = A.mesh_entries[i];
		r.b = r.a ? A.meshes[A.mesh_begin + i].num_indices / 3u : 0u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { A.mesh_first[i] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		uint32_t st = VGX_OK;
		if (t.a > A.entry_cap) { st = VGX_E_GROWN; }
		if (t.a > 0xFFFFFFFFull || t.b > 0xFFFFFFFFull) { st = VGX_E_RANGE; }
		A.state[0] = st; A.state[1] = t.a;
		if (A.status) { *A.status = st; }
	}
};

__global__ __launch_bounds__(256) void k_raster_entries(VgxRasterArgs A)
{
	if (A.state[0] != VGX_OK) { return; }
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	// the unused tail of what the sort will look at
	if (k >= A.state[1] && k < A.sort_n) { A.keys[k] = A.sentinel; A.vals[k] = 0u; }
	if (k >= A.nrange || A.mesh_entries[k] == 0u) { return; }
	VgxRasterRect r;
	(void)raster_rect(A, k, &r);
	uint64_t at = A.mesh_first[k]; // + the mesh's entries <= the total <= entry_cap: checked by finish()
	for (uint32_t ty = r.ty0; ty <= r.ty1; ++ty) {
		for (uint32_t tx = r.tx0; tx <= r.tx1; ++tx, ++at) { A.keys[at] = ty * A.tiles_w + tx; A.vals[at] = (uint32_t)(A.mesh_begin + k); }
	}
}

__global__ __launch_bounds__(256) void k_raster_tiles(VgxRasterArgs A)
{
	__shared__ VgxRasterTri s_tri[256];
	__shared__ uint64_t s_first[257];   // exclusive prefix of the triangle counts of the (at most 256) meshes in hand
	__shared__ uint32_t s_mesh[256];
	__shared__ Sum3 s_wave[4];
	__shared__ uint32_t s_count[4];
	if (A.state[0] != VGX_OK) { return; }
	const uint32_t tid = threadIdx.x;
	const int lane = tid & (VGX_WAVE - 1);
	const uint32_t wave = tid >> 6;
	const uint32_t tx = A.tile_x0 + blockIdx.x, ty = A.tile_y0 + blockIdx.y;
	const uint32_t i = tx * VGX_RASTER_TILE + (tid & 15u), j = ty * VGX_RASTER_TILE + (tid >> 4);
	const bool inside = i >= A.scissor[0] && i < A.scissor[2] && j >= A.scissor[1] && j < A.scissor[3];
	// the pixels of this tile inside the scissor, for the triangles' box test
	const uint32_t cx0 = max(tx * VGX_RASTER_TILE, A.scissor[0]), cx1 = min((tx + 1u) * VGX_RASTER_TILE, A.scissor[2]);
	const uint32_t cy0 = max(ty * VGX_RASTER_TILE, A.scissor[1]), cy1 = min((ty + 1u) * VGX_RASTER_TILE, A.scissor[3]);
	const uint32_t key = ty * A.tiles_w + tx;
	const uint32_t r0 = lower_bound_u32(A.sorted_keys, A.sort_n, key), r1 = lower_bound_u32(A.sorted_keys, A.sort_n, key + 1u);
	const bool clear = (A.flags & VGX_RASTER_CLEAR) != 0;
	if (r0 == r1 && !clear) { return; }
	uint32_t* const pixel = A.pixels + (uint64_t)j * A.stride + i;
	const uint32_t before = inside ? (clear ? A.clear_color : *pixel) : 0u;
	uint32_t d = before;
	const double px = (double)(A.x0 + (int32_t)i) + 0.5, py = (double)(A.y0 + (int32_t)j) + 0.5;
	for (uint32_t eb = r0; eb < r1; eb += 256u) { // block-uniform loops throughout
		const uint32_t ne = min(256u, r1 - eb);
		Sum3 v = sum3_zero();
		if (tid < ne) {
			const uint32_t m = A.sorted_vals[eb + tid];
			s_mesh[tid] = m;
			v.a = A.meshes[m].num_indices / 3u;
		}
		Sum3 tot;
		const Sum3 incl = block_incl_scan<256>(v, s_wave, &tot);
		s_first[tid + 1u] = incl.a;
		if (tid == 0u) { s_first[0] = 0; }
		__syncthreads();
		for (uint64_t tb = 0; tb < tot.a; tb += 256u) {
			const uint64_t g = tb + tid;
			bool keep = false;
			VgxRasterTri T;
			if (g < tot.a) {
				uint32_t lo = 0, hi = ne; // the last mesh whose first triangle is <= g
				while (hi - lo > 1u) {
					const uint32_t mid = (lo + hi) >> 1;
					if (s_first[mid] <= g) { lo = mid; } else { hi = mid; }
				}
				const vgx_mesh me = A.meshes[s_mesh[lo]];
				const uint16_t* ip = A.idx + me.first_index + 3ull * (g - s_first[lo]);
				const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
				if (i0 < me.num_vertices && i1 < me.num_vertices && i2 < me.num_vertices) {
					const float2* pp = (const float2*)A.pos + me.first_vertex;
					const uint32_t* cp = A.color + me.first_vertex;
					const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
					uint32_t a0, a1, b0, b1;
					keep = vgx_raster_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), cp[i0], cp[i1], cp[i2], &T)
					    && vgx_raster_span(T.minx, T.maxx, A.x0, cx0, cx1, &a0, &a1) && vgx_raster_span(T.miny, T.maxy, A.y0, cy0, cy1, &b0, &b1);
				}
			}
			const uint64_t kept = wave_ballot(keep);
			if (lane == 0) { s_count[wave] = (uint32_t)__popcll(kept); }
			__syncthreads();
			uint32_t base = 0, n = 0;
#pragma unroll
			for (uint32_t w = 0; w < 4u; ++w) { const uint32_t c = s_count[w]; base += w < wave ? c : 0u; n += c; }
			if (keep) { s_tri[base + (uint32_t)__popcll(kept & lanemask_lt(lane))] = T; }
			__syncthreads();
			if (inside) {
				for (uint32_t t = 0; t < n; ++t) { d = vgx_raster_pixel(s_tri[t], px, py, d); }
			}
			__syncthreads(); // s_tri and s_count are written again
		}
	}
	if (inside && (clear || d != before)) { *pixel = d; }
}

// ---- the frame family: vgx_raster_frame, vgx_raster_textured, vgx_raster_painted, vgx_raster_concave ---------------------------------
// The same steps with the state of every mesh's draw; VgxRasterFrameArgs::level says which of the four calls runs. (What the concave
// level adds -- a third tile bit and the CONTOUR instantiation -- is described at k_rasterf_tiles.)
//   k_rasterf_count    also decides what the mesh does (vgx_raster_mesh_state: stamp / test In / test Out / untested / nothing, its
//                      region, the target's scissor cut by its draw's; from the textured level on "sampled", at the painted level
//                      "gradient" / "pattern", with the handle, in the state's pad word) and keeps that per mesh of the range; the tiles
//                      are those of the box inside that rectangle. A draw index outside the table -- checked first, whatever the kind
//                      -- or a handle, image or paint record that is no good marks the mesh; the scan's third lane carries the mark to
//                      finish(), which ends the call with VGX_E_INVALID_ARG before anything is written. At the frame level a mesh of
//                      kind TEXT / TRILIST gets no entries
//   k_rasterf_entries  also marks, in one bit per tile of the image and class (tile_tex, tile_paint: zeroed by the host part before
//                      the launches, null at a level that cannot set them), the tiles a sampled / a painted mesh has an entry in
//   k_rasterf_tiles    <TEX, PAINT>: four instantiations over the same grid, of which a level launches those it can need (1, 2, 4); a
//                      tile runs the one its two bits name, the others leave at once. <false, false> is k_raster_tiles with one more
//                      register per pixel, the stamp S, carried across all batches; the state of the meshes in hand lies in LDS beside
//                      s_mesh (12 bytes: mode and the rectangle cut to the tile in one word, f, n), a setup record names its mesh's slot
//                      there and carries the mode and the rectangle as row / column masks. A triangle is tested against the tile cut by
//                      BOTH scissors, so what a cut draw cannot write never reaches the pixel loop; clip triangles take the same ordered
//                      compaction. TEX adds, per slot, the image record of a sampled mesh and, per setup record, the three UVs widened
//                      to binary64 at setup (int16: the division by 32767 happens there). PAINT adds, per slot, a 48-byte paint record
//                      (six matrix floats and either four params and the two ends packed to 8 bits, or the image record) built from the
//                      96-byte table entry; with PAINT a sampled slot keeps its image in the same record, so TEX and PAINT together
//                      need no second table. Slots are loaded once per batch of meshes by the lane that loads the slot. The pixel loop
//                      reads slot and UVs from LDS -- one address for all lanes, a broadcast -- and nothing but texels from global
//                      memory: 1 (nearest) or 4 (linear) independent loads. Every lane walks every record, so the loop stays
//                      barrier-uniform. A frame without sampled or painted meshes pays one bit test per tile for a wide kernel, not
//                      its LDS.
__device__ __forceinline__ bool frame_rect(const VgxRasterFrameArgs& F, uint64_t m, const VgxRasterMeshState& st, VgxRasterRect* r)
{
	const VgxRasterArgs& A = F.R;
	const float4 box = ((const float4*)A.mesh_bounds)[m];
	const float b[4] = { box.x, box.y, box.z, box.w };
	return vgx_raster_mesh_tiles(A.meshes[m], b, A.x0, A.y0, st.rect, F.level, r);
}

// DAMAGE (vgx_raster_damaged; every other call runs the instantiations without it -- DESIGN.md has the resource report that chose a
// template parameter over a null-means-all pointer): a bin entry is a pair of a mesh and a MARKED tile (F.damage, vgx_damage.h). The
// count takes the set bits of the mesh's tile rectangle, the entries pass emits those tiles, the tile kernel leaves an unmarked tile
// ahead of the clear. The state of every mesh, and with it VGX_E_INVALID_ARG, is decided as without it
template <bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterf_count(VgxRasterFrameArgs F)
{
	const VgxRasterArgs& A = F.R;
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= A.nrange) { return; }
	const uint64_t m = A.mesh_begin + k;
	const vgx_mesh me = A.meshes[m];
	VgxRasterMeshState st;
	uint32_t entries = 0;
	if (me.draw >= F.num_draws) {
		st.mode = VGX_RF_INVALID; st.f = st.n = st.pad = 0u;
		st.rect[0] = st.rect[1] = st.rect[2] = st.rect[3] = 0u;
	} else {
		vgx_raster_mesh_state(F.level, me, F.draws[me.draw].state_key, F.draw_state[me.draw], A.x0, A.y0, A.scissor, F.images, F.num_images,
		                      F.gradients, F.num_gradients, F.patterns, F.num_patterns, &st);
		VgxRasterRect r;
		if (st.mode != VGX_RF_NOTHING && st.mode != VGX_RF_INVALID && frame_rect(F, m, st, &r)) {
			entries = DAMAGE ? vgx_damage_rect_count(F.damage, r, A.tiles_w) : (r.tx1 - r.tx0 + 1u) * (r.ty1 - r.ty0 + 1u);
		}
	}
	F.mesh_state[k] = st;
	A.mesh_entries[k] = entries;
}

struct OpRasterFrameBin
{
	VgxRasterFrameArgs F;
	__device__ uint64_t size() const { return F.R.nrange; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		r.a = F.R.mesh_entries[i];
		r.b = r.a ? vgx_raster_mesh_elements(F.R.meshes[F.R.mesh_begin + i]) : 0u; // a contour mesh has entries at VGX_RL_CONCAVE only
		r.c = F.mesh_state[i].mode == VGX_RF_INVALID ? 1u : 0u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { F.R.mesh_first[i] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		const VgxRasterArgs& A = F.R;
		uint32_t st = VGX_OK;
		if (t.a > A.entry_cap) { st = VGX_E_GROWN; }
		if (t.c != 0u) { st = VGX_E_INVALID_ARG; }
		if (t.a > 0xFFFFFFFFull || t.b > 0xFFFFFFFFull) { st = VGX_E_RANGE; }
		A.state[0] = st; A.state[1] = t.a;
		if (A.status) { *A.status = st; }
	}
};

// (mark_tiles: vgx_damage.h)
template <bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterf_entries(VgxRasterFrameArgs F)
{
	const VgxRasterArgs& A = F.R;
	if (A.state[0] != VGX_OK) { return; }
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= A.state[1] && k < A.sort_n) { A.keys[k] = A.sentinel; A.vals[k] = 0u; }
	if (k >= A.nrange || A.mesh_entries[k] == 0u) { return; }
	const uint64_t m = A.mesh_begin + k;
	const VgxRasterMeshState st = F.mesh_state[k];
	VgxRasterRect r;
	if (!frame_rect(F, m, st, &r)) { return; } // (not taken: the count found entries)
	uint64_t at = A.mesh_first[k]; // + the mesh's entries <= the total <= entry_cap: checked by finish()
	for (uint32_t ty = r.ty0; ty <= r.ty1; ++ty) {
		for (uint32_t tx = r.tx0; tx <= r.tx1; ++tx) {
			const uint32_t key = ty * A.tiles_w + tx;
			if (DAMAGE && !vgx_damage_bit(F.damage, key)) { continue; } // as many pass as the count found: the bits do not change under the call
			A.keys[at] = key; A.vals[at] = (uint32_t)m;
			++at;
		}
	}
	// a level that cannot set a flag has no bitmap for it
	if (st.pad & VGX_RT_SAMPLED) { mark_tiles(F.tile_tex, r, A.tiles_w); }
	if (st.pad & VGX_RT_PAINTED) { mark_tiles(F.tile_paint, r, A.tiles_w); }
	if (st.pad & VGX_RT_CONTOUR) { mark_tiles(F.tile_contour, r, A.tiles_w); }
}

// 112 bytes: the record; its mesh's slot in s_state | mode << 8 | VGX_RT_SAMPLED / VGX_RT_GRADIENT / VGX_RT_PATTERN; the mesh's rectangle
// in this tile as a mask of columns (bits 0 .. 15) and a mask of rows (bits 16 .. 31), so that a pixel's test is two shifts and an AND
struct VgxRasterFrameTri { VgxRasterTri T; uint32_t slot_mode, mask; };
struct VgxRasterTileState { uint32_t mode_rect, f, n; };          // mode << 20 | y1 << 15 | x1 << 10 | y0 << 5 | x0, tile-local, half open
// 160 bytes with TEX: the record and the three UVs, written for a sampled triangle only
struct VgxRasterTexTri { VgxRasterFrameTri R; double uv[6]; };

struct VgxRasterTexelFetch
{
	const uint32_t* pixels; uint32_t stride;
	__device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return pixels[(uint64_t)y * stride + x]; }
};

__device__ __forceinline__ void store_uv(VgxRasterTexTri* r, const double* uv)
{
#pragma unroll
	for (int c = 0; c < 6; ++c) { r->uv[c] = uv[c]; }
}
__device__ __forceinline__ void store_uv(VgxRasterFrameTri*, const double*) { }
__device__ __forceinline__ const double* record_uv(const VgxRasterTexTri& r) { return r.uv; }
__device__ __forceinline__ const double* record_uv(const VgxRasterFrameTri&) { return nullptr; }
__device__ __forceinline__ VgxRasterFrameTri& frame_part(VgxRasterTexTri& r) { return r.R; }
__device__ __forceinline__ VgxRasterFrameTri& frame_part(VgxRasterFrameTri& r) { return r; }
template <bool TEX> struct RasterTexRecord { typedef VgxRasterFrameTri type; };
template <> struct RasterTexRecord<true> { typedef VgxRasterTexTri type; };

// what a slot of s_state keeps beside it: nothing, the image of a sampled mesh, or the paint record (whose image part serves a sampled mesh)
template <bool TEX, bool PAINT> struct RasterPaintSlot { typedef uint32_t type; enum { N = 1 }; };
template <> struct RasterPaintSlot<true, false> { typedef vgx_raster_image type; enum { N = 256 }; };
template <bool TEX> struct RasterPaintSlot<TEX, true> { typedef VgxRasterPaint type; enum { N = 256 }; };
__device__ __forceinline__ vgx_raster_image& slot_image(vgx_raster_image& s) { return s; }
__device__ __forceinline__ vgx_raster_image& slot_image(VgxRasterPaint& s) { return s.im; }

// bit `key` of a tile bitmap; a null bitmap (a level that cannot set it) has every bit clear. Block-uniform
__device__ __forceinline__ bool tile_bit(const uint32_t* bits, uint32_t key) { return bits != nullptr && ((bits[key >> 5] >> (key & 31u)) & 1u) != 0u; }

// Element k of the contour mesh `me` (mesh m of the frame) for the tile at (ox, oy), mr = the mesh's mode and rectangle cut to the tile:
// edge k, or the flush behind the last edge. R->slot_mode is the caller's. false: the element is not kept
__device__ __forceinline__ bool contour_element(const VgxRasterArgs& A, const vgx_mesh& me, uint32_t m, uint64_t k, uint32_t mr, uint32_t ox, uint32_t oy, VgxRasterFrameTri* R)
{
	const uint32_t cx0 = mr & 31u, cy0 = (mr >> 5) & 31u, cx1 = (mr >> 10) & 31u, cy1 = (mr >> 15) & 31u; // tile-local, half open, not empty
	if (k == me.num_indices / 2u) { // the flush: rule, box and colour of the mesh, under its rectangle's masks
		const float4 box = ((const float4*)A.mesh_bounds)[m];
		R->T.minx = box.x; R->T.miny = box.y; R->T.maxx = box.z; R->T.maxy = box.w;
		R->T.col[0] = A.color[me.first_vertex]; // num_vertices > 0: a contour mesh without a vertex has no entry
		R->T.flags = me.subpath_kind;
		R->slot_mode |= VGX_RT_FLUSH;
		R->mask = (((1u << cx1) - 1u) & ~((1u << cx0) - 1u)) | ((((1u << cy1) - 1u) & ~((1u << cy0) - 1u)) << 16);
		return true;
	}
	const uint16_t* ip = A.idx + me.first_index + 2ull * k;
	const uint32_t i0 = ip[0], i1 = ip[1];
	if (i0 >= me.num_vertices || i1 >= me.num_vertices) { return false; }
	const float2* pp = (const float2*)A.pos + me.first_vertex;
	const float2 u = pp[i0], v = pp[i1];
	R->mask = 0u;
	// the samples of the rectangle's rows, and its last column
	return vgx_raster_contour_edge(v2(u.x, u.y), v2(v.x, v.y), &R->T)
	    && vgx_raster_contour_edge_reaches(R->T, (double)(A.y0 + (int32_t)(oy + cy0)) + 0.5, (double)(A.y0 + (int32_t)(oy + cy1 - 1u)) + 0.5,
	                                       (double)(A.x0 + (int32_t)(ox + cx1 - 1u)) + 0.5);
}

// CONTOUR (vgx_raster_concave; one instantiation, of the widest shape, for every tile a contour mesh reaches -- DESIGN.md): a contour
// mesh in hand counts its edges and ONE more element, the flush. An edge is set up like a triangle's edge 0 and kept when it can add
// to the winding number of a sample of the tile (its rows, and nothing to the right of the tile); every pixel lane adds the kept edges
// to a private W, which lives across the batches of 256 records as d and S do. The flush is always kept -- the mesh's last edges may
// be culled -- and applies fill rule, box and colour, then clears W for the next contour mesh. Records stay in (mesh, element) order,
// so the mesh takes one place in painter's order
template <bool TEX, bool PAINT, bool CONTOUR, bool DAMAGE>
__global__ __launch_bounds__(256) void k_rasterf_tiles(VgxRasterFrameArgs F)
{
	static_assert(!CONTOUR || (TEX && PAINT), "the contour instantiation serves every class of tile");
	typedef typename RasterTexRecord<TEX>::type Record;
	typedef typename RasterPaintSlot<TEX, PAINT>::type Slot;
	__shared__ Record s_tri[256];
	__shared__ uint64_t s_first[257];   // exclusive prefix of the triangle counts of the (at most 256) meshes in hand
	__shared__ uint32_t s_mesh[256];
	__shared__ VgxRasterTileState s_state[256];
	__shared__ Slot s_slot[RasterPaintSlot<TEX, PAINT>::N]; // written for the sampled and the painted slots only, and not read for the others
	__shared__ uint32_t s_flags[TEX || PAINT ? 256 : 1];   // VGX_RT_SAMPLED / VGX_RT_GRADIENT / VGX_RT_PATTERN or 0 per slot
	__shared__ Sum3 s_wave[4];
	__shared__ uint32_t s_count[4];
	const VgxRasterArgs& A = F.R;
	if (A.state[0] != VGX_OK) { return; }
	const uint32_t tx = A.tile_x0 + blockIdx.x, ty = A.tile_y0 + blockIdx.y;
	const uint32_t key = ty * A.tiles_w + tx;
	if (DAMAGE && !vgx_damage_bit(F.damage, key)) { return; } // block-uniform, ahead of the clear: the tile is not redrawn
	if (tile_bit(F.tile_contour, key) != CONTOUR) { return; } // block-uniform: the tile of another instantiation
	if (!CONTOUR && (tile_bit(F.tile_tex, key) != TEX || tile_bit(F.tile_paint, key) != PAINT)) { return; }
	const uint32_t tid = threadIdx.x;
	const int lane = tid & (VGX_WAVE - 1);
	const uint32_t wave = tid >> 6;
	const uint32_t lx = tid & 15u, ly = tid >> 4;
	const uint32_t ox = tx * VGX_RASTER_TILE, oy = ty * VGX_RASTER_TILE;
	const uint32_t i = ox + lx, j = oy + ly;
	const bool inside = i >= A.scissor[0] && i < A.scissor[2] && j >= A.scissor[1] && j < A.scissor[3];
	const uint32_t r0 = lower_bound_u32(A.sorted_keys, A.sort_n, key), r1 = lower_bound_u32(A.sorted_keys, A.sort_n, key + 1u);
	const bool clear = (A.flags & VGX_RASTER_CLEAR) != 0;
	if (r0 == r1 && !clear) { return; } // block-uniform
	uint32_t* const pixel = A.pixels + (uint64_t)j * A.stride + i;
	const uint32_t before = inside ? (clear ? A.clear_color : *pixel) : 0u;
	uint32_t d = before;
	uint32_t S = VGX_RASTER_STAMP_NONE;
	int32_t W = 0; // CONTOUR: the winding number of the contour mesh whose edges are being walked
	const double px = (double)(A.x0 + (int32_t)i) + 0.5, py = (double)(A.y0 + (int32_t)j) + 0.5;
	for (uint32_t eb = r0; eb < r1; eb += 256u) { // block-uniform loops throughout
		const uint32_t ne = min(256u, r1 - eb);
		Sum3 v = sum3_zero();
		if (tid < ne) {
			const uint32_t m = A.sorted_vals[eb + tid];
			s_mesh[tid] = m;
			v.a = A.meshes[m].num_indices / 3u;
			// the mesh's rectangle cut to this tile (an entry means its box reaches the tile inside the rectangle: not empty)
			const VgxRasterMeshState ms = F.mesh_state[m - A.mesh_begin];
			if constexpr (CONTOUR) {
				if (ms.pad & VGX_RT_CONTOUR) { v.a = (uint64_t)(A.meshes[m].num_indices / 2u) + 1u; } // its edges and the flush
			}
			const uint32_t cx0 = max(ox, ms.rect[0]), cx1 = min(ox + VGX_RASTER_TILE, ms.rect[2]);
			const uint32_t cy0 = max(oy, ms.rect[1]), cy1 = min(oy + VGX_RASTER_TILE, ms.rect[3]);
			VgxRasterTileState ts;
			ts.f = ms.f; ts.n = ms.n;
			ts.mode_rect = cx0 < cx1 && cy0 < cy1 ? (ms.mode << 20) | ((cy1 - oy) << 15) | ((cx1 - ox) << 10) | ((cy0 - oy) << 5) | (cx0 - ox) : (uint32_t)VGX_RF_NOTHING << 20;
			s_state[tid] = ts;
			if constexpr (TEX || PAINT) {
				uint32_t fl = CONTOUR ? ms.pad & VGX_RT_CONTOUR : 0u;
				// handles and records are inside their tables and valid: k_rasterf_count
				if constexpr (TEX) {
					if (ms.pad & VGX_RT_SAMPLED) { fl |= VGX_RT_SAMPLED; slot_image(s_slot[tid]) = F.images[ms.pad & 0xFFFFu]; }
				}
				if constexpr (PAINT) {
					if (ms.pad & VGX_RT_PAINTED) {
						const bool grad = (ms.pad & VGX_RT_GRADIENT) != 0u;
						fl |= grad ? VGX_RT_GRADIENT : VGX_RT_PATTERN;
						VgxRasterPaint rec;
						vgx_raster_paint_record((grad ? F.gradients : F.patterns)[ms.pad & 0xFFFFu], F.images, &rec);
						s_slot[tid] = rec;
					}
				}
				s_flags[tid] = fl;
			}
		}
		Sum3 tot;
		const Sum3 incl = block_incl_scan<256>(v, s_wave, &tot);
		s_first[tid + 1u] = incl.a;
		if (tid == 0u) { s_first[0] = 0; }
		__syncthreads();
		for (uint64_t tb = 0; tb < tot.a; tb += 256u) {
			const uint64_t g = tb + tid;
			bool keep = false;
			Record R;
			VgxRasterFrameTri& RF = frame_part(R);
			double uv[6];
			if (g < tot.a) {
				uint32_t lo = 0, hi = ne; // the last mesh whose first triangle is <= g
				while (hi - lo > 1u) {
					const uint32_t mid = (lo + hi) >> 1;
					if (s_first[mid] <= g) { lo = mid; } else { hi = mid; }
				}
				const uint32_t mr = s_state[lo].mode_rect;
				const uint32_t fl = TEX || PAINT ? s_flags[lo] : 0u;
				const vgx_mesh me = A.meshes[s_mesh[lo]];
				// a contour mesh's elements are its edges and the flush (contour_element); no index triple is read for it, and the
				// indices below, ~0u >= every num_vertices, keep it out of the triangle branch. Constant false without CONTOUR
				const bool edges = CONTOUR && (fl & VGX_RT_CONTOUR) != 0u;
				if (edges) {
					RF.slot_mode = lo | ((mr >> 20) << 8) | fl;
					keep = (mr >> 20) != VGX_RF_NOTHING && contour_element(A, me, s_mesh[lo], g - s_first[lo], mr, ox, oy, &RF);
				}
				const uint16_t* ip = A.idx + me.first_index + (edges ? 0ull : 3ull * (g - s_first[lo]));
				const uint32_t i0 = edges ? ~0u : ip[0], i1 = edges ? ~0u : ip[1], i2 = edges ? ~0u : ip[2];
				if ((mr >> 20) != VGX_RF_NOTHING && i0 < me.num_vertices && i1 < me.num_vertices && i2 < me.num_vertices) {
					const float2* pp = (const float2*)A.pos + me.first_vertex;
					const uint32_t* cp = A.color + me.first_vertex;
					const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
					uint32_t a0, a1, b0, b1;
					const uint32_t cols = ((1u << ((mr >> 10) & 31u)) - 1u) & ~((1u << (mr & 31u)) - 1u), rows = ((1u << ((mr >> 15) & 31u)) - 1u) & ~((1u << ((mr >> 5) & 31u)) - 1u);
					RF.slot_mode = lo | ((mr >> 20) << 8) | fl; RF.mask = cols | (rows << 16);
					keep = vgx_raster_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), cp[i0], cp[i1], cp[i2], &RF.T)
					    && vgx_raster_span(RF.T.minx, RF.T.maxx, A.x0, ox + (mr & 31u), ox + ((mr >> 10) & 31u), &a0, &a1)
					    && vgx_raster_span(RF.T.miny, RF.T.maxy, A.y0, oy + ((mr >> 5) & 31u), oy + ((mr >> 15) & 31u), &b0, &b1);
					if (TEX && keep && (fl & VGX_RT_SAMPLED)) {
						vgx_raster_uv_widen(F.uv, F.uv_bytes, me.first_vertex + i0, uv);
						vgx_raster_uv_widen(F.uv, F.uv_bytes, me.first_vertex + i1, uv + 2);
						vgx_raster_uv_widen(F.uv, F.uv_bytes, me.first_vertex + i2, uv + 4);
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
				Record* const dst = &s_tri[base + (uint32_t)__popcll(kept & lanemask_lt(lane))];
				frame_part(*dst) = RF;
				if (TEX && (RF.slot_mode & VGX_RT_SAMPLED)) { store_uv(dst, uv); }
			}
			__syncthreads();
			for (uint32_t t = 0; t < n; ++t) { // every lane walks the records: no lane leaves between the barriers
				const VgxRasterFrameTri& rec = frame_part(s_tri[t]);
				if constexpr (CONTOUR) {
					const uint32_t sm = rec.slot_mode; // block-uniform
					if (sm & VGX_RT_CONTOUR) {
						if (!(sm & VGX_RT_FLUSH)) { W += vgx_raster_contour_winding(rec.T, px, py); continue; }
						const float box[4] = { rec.T.minx, rec.T.miny, rec.T.maxx, rec.T.maxy };
						if (((rec.mask >> lx) & (rec.mask >> (16u + ly)) & 1u) != 0u && vgx_raster_contour_covered(W, rec.T.flags, box, px, py)) {
							const VgxRasterTileState ts = s_state[sm & 255u];
							const VgxRasterPaint& pr = s_slot[sm & 255u]; // written, and read, for a painted mesh only
							VgxRasterTexelFetch fetch;
							fetch.pixels = nullptr; fetch.stride = 0u;
							if (sm & VGX_RT_PATTERN) { fetch.pixels = pr.im.pixels; fetch.stride = pr.im.stride; }
							d = vgx_raster_contour_pixel(rec.T.col[0], sm, pr, (sm >> 8) & 255u, ts.f, ts.n, px, py, &S, d, fetch);
						}
						W = 0;
						continue;
					}
				}
				const uint32_t mk = rec.mask; // beside the record: an untested mesh needs no second, dependent LDS read
				if (((mk >> lx) & (mk >> (16u + ly)) & 1u) != 0u) {
					const uint32_t sm = rec.slot_mode;
					const uint32_t mode = (sm >> 8) & 255u;
					uint32_t f = 0u, n = 0u;
					if (mode != VGX_RF_PLAIN) { const VgxRasterTileState ts = s_state[sm & 255u]; f = ts.f; n = ts.n; }
					if (TEX && (sm & VGX_RT_SAMPLED)) {
						if constexpr (TEX) {
							const vgx_raster_image im = slot_image(s_slot[sm & 255u]);
							VgxRasterTexelFetch fetch;
							fetch.pixels = im.pixels; fetch.stride = im.stride;
							d = vgx_raster_textured_pixel(rec.T, record_uv(s_tri[t]), im, mode, f, n, px, py, S, d, fetch);
						}
					} else {
						// (this shape of the dispatch is the measured one: DESIGN.md, "the two raster kernel families")
						bool painted = false;
						if constexpr (PAINT) {
							if (sm & VGX_RT_GRADIENT) {
								d = vgx_raster_gradient_pixel(rec.T, s_slot[sm & 255u], mode, f, n, px, py, S, d);
								painted = true;
							} else if (sm & VGX_RT_PATTERN) {
								const VgxRasterPaint pr = s_slot[sm & 255u];
								VgxRasterTexelFetch fetch;
								fetch.pixels = pr.im.pixels; fetch.stride = pr.im.stride;
								d = vgx_raster_pattern_pixel(rec.T, pr, mode, f, n, px, py, S, d, fetch);
								painted = true;
							}
						}
						if (!painted) { d = vgx_raster_frame_pixel(rec.T, mode, f, n, px, py, &S, d); }
					}
				}
			}
			__syncthreads(); // s_tri and s_count are written again
		}
		__syncthreads(); // s_mesh, s_state, s_slot, s_flags and s_first are written again
	}
	if (inside && (clear || d != before)) { *pixel = d; }
}

} // namespace

size_t vgx_raster_sort_bytes(uint64_t n, uint32_t bits)
{
	size_t bytes = 0;
	if (n == 0 || rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
	                                        (size_t)n, 0u, bits, (hipStream_t)0) != hipSuccess) {
		return 0;
	}
	return bytes ? bytes : 1;
}

namespace {

// count, scan, entries, sort, tiles: the one sequence of both families. `a` is the plain part of `args`, Op the family's scan operator,
// tiles(grid) launches the family's tile kernel(s)
template <class Op, class Args, class Tiles>
hipError_t launch_sequence(const Args& args, const VgxRasterArgs& a, void (*count)(Args), void (*entries)(Args), Tiles tiles, void* partial, void* sortTemp,
                           size_t sortBytes, hipStream_t s)
{
	if (a.nrange) { hipLaunchKernelGGL(count, dim3((unsigned)((a.nrange + 255) / 256)), dim3(256), 0, s, args); }
	const Op op = { args };
	vgx_device_scan(op, (Sum3*)partial, s, a.nrange);
	const uint64_t items = a.nrange > a.sort_n ? a.nrange : a.sort_n;
	if (items) { hipLaunchKernelGGL(entries, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, args); }
	if (a.sort_n) {
		const hipError_t e = rocprim::radix_sort_pairs(sortTemp, sortBytes, (const uint32_t*)a.keys, a.sorted_keys, (const uint32_t*)a.vals, a.sorted_vals,
		                                               (size_t)a.sort_n, 0u, a.sort_bits, s);
		if (e != hipSuccess) { return e; }
	}
	if (a.tiles_x && a.tiles_y) { tiles(dim3(a.tiles_x, a.tiles_y)); }
	return hipSuccess;
}

} // namespace

hipError_t vgx_launch_raster(const VgxRasterArgs& a, void* partial, void* sortTemp, size_t sortBytes, hipStream_t s)
{
	const auto tiles = [&](dim3 grid) { hipLaunchKernelGGL(k_raster_tiles, grid, dim3(256), 0, s, a); };
	return launch_sequence<OpRasterBin>(a, a, k_raster_count, k_raster_entries, tiles, partial, sortTemp, sortBytes, s);
}

namespace {

template <bool DAMAGE>
hipError_t launch_frame(const VgxRasterFrameArgs& f, void* partial, void* sortTemp, size_t sortBytes, hipStream_t s)
{
	const auto tiles = [&](dim3 grid) { // the instantiations whose tiles the level can have
		hipLaunchKernelGGL((k_rasterf_tiles<false, false, false, DAMAGE>), grid, dim3(256), 0, s, f);
		if (f.level >= VGX_RL_TEXTURED) { hipLaunchKernelGGL((k_rasterf_tiles<true, false, false, DAMAGE>), grid, dim3(256), 0, s, f); }
		if (f.level >= VGX_RL_PAINTED) {
			hipLaunchKernelGGL((k_rasterf_tiles<false, true, false, DAMAGE>), grid, dim3(256), 0, s, f);
			hipLaunchKernelGGL((k_rasterf_tiles<true, true, false, DAMAGE>), grid, dim3(256), 0, s, f);
		}
		if (f.level >= VGX_RL_CONCAVE) { hipLaunchKernelGGL((k_rasterf_tiles<true, true, true, DAMAGE>), grid, dim3(256), 0, s, f); }
	};
	return launch_sequence<OpRasterFrameBin>(f, f.R, k_rasterf_count<DAMAGE>, k_rasterf_entries<DAMAGE>, tiles, partial, sortTemp, sortBytes, s);
}

} // namespace

// f.damage set: vgx_raster_damaged (the concave level)
hipError_t vgx_launch_raster_frame(const VgxRasterFrameArgs& f, void* partial, void* sortTemp, size_t sortBytes, hipStream_t s)
{
	return f.damage ? launch_frame<true>(f, partial, sortTemp, sortBytes, s) : launch_frame<false>(f, partial, sortTemp, sortBytes, s);
}
