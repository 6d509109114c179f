// vgx_pick_rect.hip -- rectangles against a mesh stream on gfx950: pick tolerance and marquee selection (include/vgx.h: vgx_pick_rect;
// the arithmetic: vgx_pick_rect.h). The answer is a set per query, so every plane is one 64-bit word per mesh, one bit per query:
//   k_pickr_meshes   one lane per mesh, the queries staged once per workgroup in LDS (2 KB): the queries the mesh is a candidate of (in
//                    range, it has a triangle, its box overlaps R), its `inside` word (1 for a query that does not look at it: neutral
//                    under AND), a zeroed `touch` word, its triangle count (0 for no query's candidate) with the run-head flag
//                    draw != the mesh before's draw in bit 31, and the neutral run words of run number m. The `inside` plane is written
//                    only when some query has VGX_PICK_RECT_WINDOW, the run words only when one has VGX_PICK_RECT_BY_DRAW: nobody reads them else
//   scan OpPickrCand (vgx_scan.h) the dense ascending candidate list, the exclusive prefix of the candidates' triangle counts, and riding
//                    along the number of run heads: the run of every mesh and the first mesh of every run
//   k_pickr_tris     k_pick_tris's traversal: a fixed grid strides over tiles of 256 candidate triangles, wave_owners gives a lane its
//                    triangle, vgx_pickr_setup runs once, then a wave-uniform loop over the queries set in the union of the wave's
//                    candidate words. The lanes of one mesh are consecutive: their bits are ORed along the segment and its last lane
//                    publishes them with ONE 64-bit atomicOr per (wave, mesh) that has a touching lane
//   k_pickr_runs     one lane per mesh, skipped without a VGX_PICK_RECT_BY_DRAW query: touch ORed and the missing `inside` bits cleared
//                    along the lanes of a run, one atomicOr / atomicAnd per (wave, run) that changes anything
//   k_pickr_select   one wave per block of 64 meshes: the entry word (vgx_pickr_entry_word) of every mesh, written over its candidate
//                    word, its top word (vgx_pickr_top_word), and per (block, query) the entry count and the largest mesh with a top
//                    bit -- ballots, lane q keeps query q's
//   k_pickr_finish   one workgroup per query: the exclusive prefix of its block counts in ascending steps of 2048 blocks, eight per thread
//                    (written over the counts), count[q], the largest top mesh, then a second look at that one mesh for its largest touching triangle
//                    (as k_pickf_resolve does for its winner) and top[q]
//   k_pickr_list     one wave per block: rank = the block's prefix + the ballot bits below the lane; the entries below list_cap are stored
// OR, AND and maxima do not depend on the order, the counts are summed in block order: the same bytes every run. No host round trip, a
// fixed number of launches, every table sized by num_meshes.
// Not done: "a triangle whose box lies inside R needs only A != 0". With inexact products e(third corner) of the edges b->c and c->a is
// A only as a real number, so the shortcut could differ from the header's rule in a word; the one-corner form costs three edge values.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_pick_rect.h"

namespace {

#define VGX_PICKR_TILE 256
#define VGX_PICKR_HEAD 0x80000000u // in cand_tris: the mesh begins a run
#define VGX_PICKR_PER 8            // blocks a thread of k_pickr_finish takes a step: 2048 blocks = 131 072 meshes a step

// OR of `w` over the lanes [head, lane] of my segment (head: seg_head of the segment's first lane, < 0: from lane 0)
__device__ __forceinline__ uint64_t seg_incl_or(uint64_t w, int head, int lane)
{
	const int first = head < 0 ? 0 : head;
#pragma unroll
	for (int d = 1; d < VGX_WAVE; d <<= 1) {
		const uint64_t o = __shfl_up((unsigned long long)w, d);
		if (lane - d >= first) { w |= o; }
	}
	return w;
}

// the queries with `flag`, one bit each: every wave for itself, no LDS
__device__ __forceinline__ uint64_t query_flag_mask(const VgxPickrArgs& A, uint32_t flag, int lane)
{
	return wave_ballot((uint32_t)lane < A.nqueries && (A.queries[lane].flags & flag) != 0u);
}

__global__ __launch_bounds__(256) void k_pickr_meshes(VgxPickrArgs A)
{
	__shared__ vgx_pick_rect_query s_q[VGX_PICK_RECT_MAX_QUERIES];
	__shared__ uint32_t s_valid[VGX_PICK_RECT_MAX_QUERIES];
	uint32_t myFlags = 0u;
	if (threadIdx.x < A.nqueries) {
		const vgx_pick_rect_query Q = A.queries[threadIdx.x];
		s_q[threadIdx.x] = Q;
		s_valid[threadIdx.x] = vgx_pickr_query_valid(Q) ? 1u : 0u;
		myFlags = Q.flags;
	}
	// a plane nobody will read is not written: `inside` without a window query, the run words without a VGX_PICK_RECT_BY_DRAW query
	const bool anyWindow = __syncthreads_or((myFlags & VGX_PICK_RECT_WINDOW) ? 1 : 0) != 0;
	const bool anyByDraw = __syncthreads_or((myFlags & VGX_PICK_RECT_BY_DRAW) ? 1 : 0) != 0;
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= A.num_meshes) { return; }
	const vgx_mesh me = A.meshes[m];
	const uint32_t tris = vgx_pick_mesh_triangles(me);
	const float4 box = ((const float4*)A.mesh_bounds)[m];
	uint64_t cand = 0ull, inside = ~0ull;
	for (uint32_t q = 0; q < A.nqueries; ++q) {
		const vgx_pick_rect_query Q = s_q[q];
		if (!s_valid[q] || !vgx_pickr_in_range(Q, m)) { continue; }
		if (tris && vgx_pickr_box_overlap(Q, box.x, box.y, box.z, box.w)) { cand |= 1ull << q; }
		if (!vgx_pickr_box_inside(Q, box.x, box.y, box.z, box.w)) { inside &= ~(1ull << q); }
	}
	const bool head = m == 0 || A.meshes[m - 1].draw != me.draw;
	A.cand[m] = cand; A.touch[m] = 0ull;
	if (anyWindow) { A.inside[m] = inside; }
	A.cand_tris[m] = (cand ? tris : 0u) | (head ? VGX_PICKR_HEAD : 0u);
	if (anyByDraw) { A.run_touch[m] = 0ull; A.run_inside[m] = ~0ull; } // run numbers are <= mesh numbers: every run's words are among these
}

struct OpPickrCand // vgx_pick.hip's OpPickCand, with the run heads counted in the third sum
{
	const uint32_t* candTris;
	uint64_t numMeshes;
	uint32_t* candMesh;
	uint64_t* candPrefix; // [numCand + 1]
	uint32_t* runOf; uint32_t* runFirst;
	uint64_t* totals;     // numCand, total triangles, runs
	__device__ uint64_t size() const { return numMeshes; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t w = candTris[i], t = w & ~VGX_PICKR_HEAD;
		r.a = t ? 1u : 0u; r.b = t; r.c = w >> 31;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		const uint32_t w = candTris[i];
		if (w & ~VGX_PICKR_HEAD) { candMesh[e.a] = (uint32_t)i; candPrefix[e.a] = e.b; }
		const uint64_t run = e.c + (w >> 31) - 1u; // mesh 0 is a head: the inclusive count is >= 1
		runOf[i] = (uint32_t)run;
		if (w >> 31) { runFirst[run] = (uint32_t)i; }
	}
	__device__ void finish(Sum3 t) const { totals[0] = t.a; totals[1] = t.b; totals[2] = t.c; candPrefix[t.a] = t.b; }
};

__global__ __launch_bounds__(256) void k_pickr_tris(VgxPickrArgs A)
{
	__shared__ vgx_pick_rect_query s_q[VGX_PICK_RECT_MAX_QUERIES];
	bool wantAlpha = false;
	if (threadIdx.x < A.nqueries) {
		const vgx_pick_rect_query Q = A.queries[threadIdx.x];
		s_q[threadIdx.x] = Q;
		wantAlpha = (Q.flags & VGX_PICK_SKIP_TRANSPARENT) != 0;
	}
	const bool anyAlpha = __syncthreads_or(wantAlpha ? 1 : 0) != 0;
	const uint64_t numCand = A.totals[0], totalTris = A.totals[1];
	const uint64_t numTiles = (totalTris + VGX_PICKR_TILE - 1) / VGX_PICKR_TILE;
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	for (uint64_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
		const uint64_t T0 = tile * VGX_PICKR_TILE + (uint64_t)wave * VGX_WAVE;
		if (T0 >= totalTris) { continue; } // the last tile's empty waves; nothing below synchronises the workgroup
		const WaveOwners o = wave_owners(A.cand_prefix, numCand, totalTris, T0, lane); // every candidate has a triangle: P is strictly ascending
		// the lanes of one candidate are consecutive: the last lane of every segment publishes for it
		// (a lane past the total searched for T0 and would join its candidate: it gets a segment of its own)
		const int k = o.live ? o.k : -1;
		const int kPrev = __shfl_up(k, 1);
		const uint64_t heads = wave_ballot(lane == 0 || k != kPrev);
		const int head = seg_head(heads, lane);
		const bool segLast = lane == VGX_WAVE - 1 || ((heads >> (lane + 1)) & 1ull) != 0ull;
		uint32_t m = 0;
		uint64_t cand = 0ull;
		VgxPickrTri Tri;
		bool ok = false, transparent = false;
		if (o.live) {
			m = A.cand_mesh[o.c0 + (uint64_t)o.k];
			const uint32_t t = (uint32_t)(T0 + (uint64_t)lane - o.first);
			const vgx_mesh me = A.meshes[m];
			const uint16_t* ip = A.idx + me.first_index + 3ull * t;
			const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
			if (vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) {
				const float2* pp = (const float2*)A.pos + me.first_vertex;
				const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
				vgx_pickr_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), &Tri);
				ok = Tri.sign != 0;
				if (ok) {
					cand = A.cand[m];
					if (anyAlpha) {
						const uint32_t* cp = A.color + me.first_vertex;
						transparent = vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2]);
					}
				}
			}
		}
		// the union of the wave's candidate words, in scalar registers
		const uint32_t ulo = wave_uniform_u32(wave_reduce((uint32_t)cand, [](uint32_t x, uint32_t y) { return x | y; }));
		const uint32_t uhi = wave_uniform_u32(wave_reduce((uint32_t)(cand >> 32), [](uint32_t x, uint32_t y) { return x | y; }));
		uint64_t todo = ((uint64_t)uhi << 32) | ulo;
		uint64_t mine = 0ull;
		while (todo) {
			const uint32_t q = (uint32_t)__builtin_ctzll(todo);
			todo &= todo - 1ull;
			const vgx_pick_rect_query Q = s_q[q];
			const bool hit = ok && ((cand >> q) & 1ull) != 0ull && !((Q.flags & VGX_PICK_SKIP_TRANSPARENT) && transparent) && vgx_pickr_touch(Tri, Q);
			mine |= hit ? 1ull << q : 0ull;
		}
		if (!wave_ballot(mine != 0ull)) { continue; }
		const uint64_t seg = seg_incl_or(mine, head, lane);
		if (o.live && segLast && seg) { atomicOr((unsigned long long*)(A.touch + m), (unsigned long long)seg); }
	}
}

// A lane past the frame's last mesh takes part in the shuffles with neutral words
__global__ __launch_bounds__(256) void k_pickr_runs(VgxPickrArgs A)
{
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint64_t byDraw = query_flag_mask(A, VGX_PICK_RECT_BY_DRAW, lane);
	if (!byDraw) { return; }
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = m < A.num_meshes;
	const uint32_t run = live ? A.run_of[m] : 0xFFFFFFFFu;
	const uint64_t touch = live ? A.touch[m] & byDraw : 0ull;
	const uint64_t both = byDraw & query_flag_mask(A, VGX_PICK_RECT_WINDOW, lane); // only these queries ever look at a run's `inside`
	const uint64_t outside = live && both ? ~A.inside[m] & both : 0ull;
	const uint32_t rPrev = (uint32_t)__shfl_up((int)run, 1);
	const uint64_t heads = wave_ballot(lane == 0 || run != rPrev);
	const int head = seg_head(heads, lane);
	const bool segLast = lane == VGX_WAVE - 1 || ((heads >> (lane + 1)) & 1ull) != 0ull;
	if (!wave_ballot((touch | outside) != 0ull)) { return; }
	const uint64_t t = seg_incl_or(touch, head, lane), o = seg_incl_or(outside, head, lane);
	if (live && segLast) {
		if (t) { atomicOr((unsigned long long*)(A.run_touch + run), (unsigned long long)t); }
		if (o) { atomicAnd((unsigned long long*)(A.run_inside + run), (unsigned long long)~o); }
	}
}

__global__ __launch_bounds__(256) void k_pickr_select(VgxPickrArgs A)
{
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint64_t window = query_flag_mask(A, VGX_PICK_RECT_WINDOW, lane), byDraw = query_flag_mask(A, VGX_PICK_RECT_BY_DRAW, lane);
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t block = m >> 6; // uniform over the wave
	if (block * VGX_WAVE >= A.num_meshes) { return; }
	uint64_t entry = 0ull, top = 0ull;
	if (m < A.num_meshes) {
		const uint64_t touch = A.touch[m], inside = window ? A.inside[m] : ~0ull; // without a window query the plane was not written
		uint64_t runTouch = 0ull, runInside = 0ull;
		bool runHead = false;
		if (byDraw) {
			const uint32_t run = A.run_of[m];
			runTouch = A.run_touch[run]; runInside = A.run_inside[run];
			runHead = A.run_first[run] == (uint32_t)m;
		}
		entry = vgx_pickr_entry_word(touch, inside, runTouch, runInside, runHead, window, byDraw);
		top = vgx_pickr_top_word(touch, inside, runTouch, runInside, window, byDraw);
		A.cand[m] = entry; // the top word lives on in block_top alone
	}
	uint32_t myCount = 0u, myTop = 0u;
	if (wave_ballot((entry | top) != 0ull)) {
		for (uint32_t q = 0; q < A.nqueries; ++q) {
			const uint64_t e = wave_ballot(((entry >> q) & 1ull) != 0ull), t = wave_ballot(((top >> q) & 1ull) != 0ull);
			if ((uint32_t)lane == q) {
				myCount = (uint32_t)__popcll(e);
				myTop = t ? (uint32_t)(block * VGX_WAVE) + (uint32_t)(63 - __clzll((long long)t)) + 1u : 0u;
			}
		}
	}
	A.block_count[block * VGX_WAVE + (uint64_t)lane] = myCount;
	A.block_top[block * VGX_WAVE + (uint64_t)lane] = myTop;
}

__global__ __launch_bounds__(256) void k_pickr_finish(VgxPickrArgs A)
{
	__shared__ uint32_t s_w[4];
	const uint32_t q = blockIdx.x, tid = threadIdx.x;
	const int lane = tid & (VGX_WAVE - 1), wave = tid >> 6;
	const vgx_pick_rect_query Q = A.queries[q];
	const uint64_t numBlocks = (A.num_meshes + VGX_WAVE - 1) / VGX_WAVE;
	uint32_t carry = 0u, best = 0u;
	// a thread takes VGX_PICKR_PER consecutive blocks a step: their loads are in flight together, and a frame of 4.35 M meshes is 34 steps
	// of two barriers, not 266 (the walk is latency bound: one workgroup, every step waits for its loads)
	for (uint64_t base = 0; base < numBlocks; base += 256 * VGX_PICKR_PER) {
		const uint64_t b0 = base + (uint64_t)tid * VGX_PICKR_PER;
		uint32_t c[VGX_PICKR_PER], sum = 0u;
#pragma unroll
		for (int k = 0; k < VGX_PICKR_PER; ++k) {
			const bool in = b0 + k < numBlocks;
			c[k] = in ? A.block_count[(b0 + k) * VGX_WAVE + q] : 0u;
			const uint32_t t = in ? A.block_top[(b0 + k) * VGX_WAVE + q] : 0u;
			best = t > best ? t : best;
			sum += c[k];
		}
		const uint32_t incl = wave_incl_scan_u32(sum, lane);
		if (lane == VGX_WAVE - 1) { s_w[wave] = incl; }
		__syncthreads();
		uint32_t before = carry, total = carry;
		for (int w = 0; w < 4; ++w) { const uint32_t s = s_w[w]; before += w < wave ? s : 0u; total += s; }
		__syncthreads();
		uint32_t excl = before + incl - sum;
#pragma unroll
		for (int k = 0; k < VGX_PICKR_PER; ++k) {
			if (b0 + k < numBlocks) { A.block_count[(b0 + k) * VGX_WAVE + q] = excl; }
			excl += c[k];
		}
		carry = total;
	}
	best = block_max_u32(best, s_w);
	if (tid == 0 && A.count) { A.count[q] = carry; }
	if (!A.top) { return; }
	uint32_t tri = 0u;
	if (best) { // uniform over the workgroup
		const vgx_mesh me = A.meshes[best - 1u];
		const uint16_t* ip = A.idx + me.first_index;
		const float2* pp = (const float2*)A.pos + me.first_vertex;
		const uint32_t* cp = A.color + me.first_vertex;
		const bool skips = (Q.flags & VGX_PICK_SKIP_TRANSPARENT) != 0u;
		const uint32_t tris = vgx_pick_mesh_triangles(me);
		for (uint32_t t = tid; t < tris; t += 256) {
			const uint32_t i0 = ip[3ull * t], i1 = ip[3ull * t + 1], i2 = ip[3ull * t + 2];
			if (!vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) { continue; }
			if (skips && vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2])) { continue; }
			const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
			VgxPickrTri Tri;
			vgx_pickr_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), &Tri);
			if (vgx_pickr_touch(Tri, Q)) { tri = t + 1u; }
		}
		tri = block_max_u32(tri, s_w);
	}
	if (tid == 0) { A.top[q] = vgx_pickr_record(best, tri, A.meshes); }
}

__global__ __launch_bounds__(256) void k_pickr_list(VgxPickrArgs A)
{
	__shared__ vgx_pick_rect_query s_q[VGX_PICK_RECT_MAX_QUERIES];
	if (threadIdx.x < A.nqueries) { s_q[threadIdx.x] = A.queries[threadIdx.x]; }
	__syncthreads();
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t block = m >> 6; // uniform over the wave
	const uint64_t entry = m < A.num_meshes ? A.cand[m] : 0ull;
	if (!wave_ballot(entry != 0ull)) { return; }
	for (uint32_t q = 0; q < A.nqueries; ++q) {
		const bool mineSet = ((entry >> q) & 1ull) != 0ull;
		const uint64_t e = wave_ballot(mineSet);
		if (!e) { continue; }
		const uint32_t first = A.block_count[block * VGX_WAVE + q]; // the entries of the blocks before: uniform
		if (first >= A.list_cap) { continue; }
		const uint32_t rank = first + (uint32_t)__popcll(e & lanemask_lt(lane));
		if (mineSet && rank < A.list_cap) { A.list[(uint64_t)q * A.list_cap + rank] = vgx_pickr_entry_value(s_q[q], (uint32_t)m); }
	}
}

} // namespace

void vgx_launch_pick_rect(const VgxPickrArgs& a, void* partial, uint32_t grid, hipStream_t s)
{
	const unsigned tb = (unsigned)((a.num_meshes + 255) / 256);
	if (a.num_meshes) { hipLaunchKernelGGL(k_pickr_meshes, dim3(tb), dim3(256), 0, s, a); }
	OpPickrCand op;
	op.candTris = a.cand_tris; op.numMeshes = a.num_meshes; op.candMesh = a.cand_mesh; op.candPrefix = a.cand_prefix;
	op.runOf = a.run_of; op.runFirst = a.run_first; op.totals = a.totals;
	vgx_device_scan_small(op, (Sum3*)partial, s, a.num_meshes); // up to 1024 meshes one workgroup of 256: at 1024 threads the operator spills 200 bytes a lane
	if (a.num_meshes) {
		hipLaunchKernelGGL(k_pickr_tris, dim3(grid), dim3(256), 0, s, a);
		hipLaunchKernelGGL(k_pickr_runs, dim3(tb), dim3(256), 0, s, a);
		hipLaunchKernelGGL(k_pickr_select, dim3(tb), dim3(256), 0, s, a);
	}
	hipLaunchKernelGGL(k_pickr_finish, dim3(a.nqueries), dim3(256), 0, s, a); // without meshes too: every count 0, every top "none"
	if (a.list && a.list_cap && a.num_meshes) { hipLaunchKernelGGL(k_pickr_list, dim3(tb), dim3(256), 0, s, a); }
}
