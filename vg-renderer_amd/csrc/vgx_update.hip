// vgx_update.hip -- where the instances of a submitted frame live, and rewriting the slices of a few of them, on gfx950.
//
// vgx_cache_layout: the instance scan of vgx_cache_submit (vgx_scan.h over vgx_cache_range_counts, vgx_update.h) storing one 32-byte
//   vgx_cache_slot per instance instead of three prefix arrays in context scratch.
//
// vgx_cache_update: a listed instance is one whole drawing (41 k vertices in 435 meshes) or a one-draw instance of 4 .. 100 vertices,
//   and the list holds one entry or a hundred thousand, so the work is spread by OUTPUT VERTEX, not by instance:
//   scan OpUpdateList  one item per listed entry: the checks of vgx_update_classify, exclusive sums of the vertices and meshes of
//                      the entries that pass (the others count nothing and are never walked), the status from the ORed flag word
//   k_update_pos       a wave owns a contiguous range of the "dirty vertex" space (a multiple of 256 vertices), finds its first
//                      listed entry by search and walks on, as k_cache_copy_flat does: cached position -> v2xform -> the frame.
//                      8 B read (the cached drawing stays in L2) + 8 B written per vertex
//   k_update_meshes    a wave owns a contiguous range of the "dirty mesh" space and takes one mesh at a time, the records handed
//                      round 64 at a time: the instance's colour into the non-AA meshes (4 B written per vertex of those), and, when
//                      the caller keeps a vgx_mesh_bounds table, the mesh's box. The box is reduced over the order-preserving integer
//                      images (vgx_bounds.h) of the SAME v2xform of the cached positions -- the bytes k_update_pos stores, so nothing
//                      of the frame is read back -- and stored plainly by the one wave that owns the mesh: no empty-box reset, no
//                      atomics, no decode pass.
//   Duplicates in the list are walked twice and store the same bytes twice: positions, colours and boxes are functions of (cache,
//   inst[d], slots[d]) alone. No kernel both resets and combines a value, so two copies of an instance cannot race to a different
//   result.
// Bounds of every store: vgx_update_classify admits an entry only if its slice [slots[d], slots[d+1]) has exactly the range's vertex
// and mesh counts and ends inside the frame's totals; a mesh's vertex span is clipped to its slice (vgx_update_mesh_span).
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_bounds.h"
#include "vgx_update.h"

namespace {

// (both scans: vgx_device_scan_small, vgx_scan.h)
// ---- vgx_cache_layout ---------------------------------------------------------------------------------------------------
struct OpCacheLayout
{
	vgx_cache_desc cache;
	const vgx_cache_instance* inst;
	uint64_t ninst;
	vgx_cache_slot* slots;
	uint32_t* status; // the caller's dev_status (already VGX_OK) or null
	__device__ uint64_t size() const { return ninst; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		VgxRangeCounts n = { 0, 0, 0 };
		if (!vgx_cache_range_counts(cache, inst[i], &n) && status) { *status = (uint32_t)VGX_E_INVALID_ARG; } // every writer stores the same word
		r.a = n.meshes; r.b = n.vertices; r.c = n.indices;
		return r;
	}
	__device__ void put(uint64_t i, uint64_t m, uint64_t v, uint64_t x, uint64_t c) const
	{
		uint64_t* p = (uint64_t*)(slots + i);
		p[0] = m; p[1] = v; p[2] = x; p[3] = c;
	}
	__device__ void store(uint64_t i, Sum3 e) const { put(i, e.a, e.b, e.c, inst[i].first_mesh); }
	__device__ void finish(Sum3 t) const { put(ninst, t.a, t.b, t.c, 0); }
};

// ---- vgx_cache_update ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t update_list_size(const VgxUpdateArgs& A)
{
	if (!A.dev_ndirty) { return A.ndirty; }
	const uint64_t n = *A.dev_ndirty;
	return n < A.ndirty ? n : A.ndirty;
}

struct OpUpdateList
{
	VgxUpdateArgs A;
	__device__ uint64_t size() const { return update_list_size(A); }
	__device__ Sum3 load(uint64_t j) const
	{
		Sum3 r = sum3_zero();
		VgxRangeCounts n;
		const uint32_t bad = vgx_update_classify(A.cache, A.inst, A.ninst, A.slots, A.dirty[j], A.frame_vertices, A.frame_meshes, &n);
		if (bad) { atomicOr(A.flags, bad); } // rare; an OR does not depend on the order, nor on how often the scan loads an item
		r.a = n.vertices; r.b = n.meshes;
		return r;
	}
	__device__ void store(uint64_t j, Sum3 e) const { A.vert_prefix[j] = e.a; A.mesh_prefix[j] = e.b; }
	__device__ void finish(Sum3 t) const
	{
		const uint64_t n = size();
		A.vert_prefix[n] = t.a; A.mesh_prefix[n] = t.b;
		// every load of the scan lies in front of this call (an earlier kernel, or the block barrier of the single-workgroup form)
		if (A.status) { *A.status = (uint32_t)vgx_update_status(__hip_atomic_load(A.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
	}
};

__global__ __launch_bounds__(VGX_WAVE) void k_update_pos(VgxUpdateArgs A)
{
	const int lane = threadIdx.x;
	const uint64_t nlist = update_list_size(A);
	const uint64_t* prefix = A.vert_prefix;
	const uint64_t total = prefix[nlist];
	// ranges are multiples of 256 vertices so that the 4x-unrolled loop below mostly runs full
	uint64_t per = (total + gridDim.x - 1) / gridDim.x;
	per = (per + 255) / 256 * 256;
	const uint64_t o0 = (uint64_t)blockIdx.x * per;
	const uint64_t o1 = o0 + per < total ? o0 + per : total;
	if (o0 >= o1) { return; }
	uint64_t j = find_owner_u64(prefix, 0, nlist, o0); // the listed entry that owns dirty vertex o0 (skips entries that count nothing)
	uint64_t o = o0;
	while (o < o1) {
		const uint64_t jb = prefix[j], je = prefix[j + 1];
		if (je <= o) { ++j; continue; }
		const uint64_t d = A.dirty[j];
		const vgx_cache_instance in = A.inst[d];
		const uint64_t end = je < o1 ? je : o1;
		const float2* sp = (const float2*)A.cache.pos + vgx_cache_first_vertex(A.cache, in.first_mesh) + (o - jb);
		float2* dp = (float2*)A.pos + A.slots[d].first_vertex + (o - jb);
		const uint64_t n = end - o;
		uint64_t k = lane;
		for (; k + 3 * VGX_WAVE < n; k += 4 * VGX_WAVE) { // four independent 512-byte wave loads in flight
			const float2 q0 = sp[k], q1 = sp[k + VGX_WAVE], q2 = sp[k + 2 * VGX_WAVE], q3 = sp[k + 3 * VGX_WAVE];
			const V2 r0 = v2xform(v2(q0.x, q0.y), in.mtx), r1 = v2xform(v2(q1.x, q1.y), in.mtx);
			const V2 r2 = v2xform(v2(q2.x, q2.y), in.mtx), r3 = v2xform(v2(q3.x, q3.y), in.mtx);
			dp[k] = make_float2(r0.x, r0.y); dp[k + VGX_WAVE] = make_float2(r1.x, r1.y);
			dp[k + 2 * VGX_WAVE] = make_float2(r2.x, r2.y); dp[k + 3 * VGX_WAVE] = make_float2(r3.x, r3.y);
		}
		for (; k < n; k += VGX_WAVE) {
			const float2 q = sp[k];
			const V2 r = v2xform(v2(q.x, q.y), in.mtx);
			dp[k] = make_float2(r.x, r.y);
		}
		o = end;
	}
}

__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

template<int BOUNDS>
__global__ __launch_bounds__(VGX_WAVE) void k_update_meshes(VgxUpdateArgs A)
{
	const int lane = threadIdx.x;
	const uint64_t nlist = update_list_size(A);
	const uint64_t* prefix = A.mesh_prefix;
	const uint64_t total = prefix[nlist];
	const uint64_t per = (total + gridDim.x - 1) / gridDim.x;
	const uint64_t q0 = (uint64_t)blockIdx.x * per;
	const uint64_t q1 = q0 + per < total ? q0 + per : total;
	if (q0 >= q1) { return; }
	uint64_t j = find_owner_u64(prefix, 0, nlist, q0);
	uint64_t q = q0;
	while (q < q1) {
		const uint64_t jb = prefix[j], je = prefix[j + 1];
		if (je <= q) { ++j; continue; }
		const uint64_t d = A.dirty[j];
		const vgx_cache_instance in = A.inst[d];
		const vgx_cache_slot s0 = A.slots[d];
		const uint64_t sliceVertices = A.slots[d + 1].first_vertex - s0.first_vertex;
		const uint64_t rangeFirst = vgx_cache_first_vertex(A.cache, in.first_mesh);
		const uint64_t end = je < q1 ? je : q1;
		// meshes [k0, k1) of the instance's range; 64 records at a time, one per lane, handed round by readlane
		const uint64_t k1 = end - jb;
		for (uint64_t k0 = q - jb; k0 < k1; k0 += VGX_WAVE) {
			const uint64_t left = k1 - k0;
			const int cnt = left < (uint64_t)VGX_WAVE ? (int)left : VGX_WAVE;
			uint64_t offL = 0; uint32_t nvL = 0, uniL = 0;
			if (lane < cnt) {
				const vgx_mesh src = A.cache.meshes[in.first_mesh + k0 + (uint64_t)lane];
				nvL = vgx_update_mesh_span(src, rangeFirst, sliceVertices, &offL);
				uniL = vgx_mesh_takes_instance_colour(src.subpath_kind) ? 1u : 0u;
			}
			for (int t = 0; t < cnt; ++t) {
				const uint32_t nv = wave_bcast_u32(nvL, t);
				const bool uni = wave_bcast_u32(uniL, t) != 0u;
				if (!BOUNDS && !uni) { continue; }
				const uint64_t off = wave_bcast_u64(offL, t);
				if (uni) {
					uint32_t* dc = A.color + s0.first_vertex + off;
					for (uint32_t v = lane; v < nv; v += VGX_WAVE) { dc[v] = in.color; }
				}
				if (BOUNDS) {
					uint32_t lox = VGX_ORD_POS_INF, loy = VGX_ORD_POS_INF, hix = VGX_ORD_NEG_INF, hiy = VGX_ORD_NEG_INF;
					const float2* sp = (const float2*)A.cache.pos + rangeFirst + off;
					for (uint32_t v = lane; v < nv; v += VGX_WAVE) {
						const float2 c = sp[v];
						const V2 r = v2xform(v2(c.x, c.y), in.mtx); // what k_update_pos stores for this vertex
						const uint32_t x = vgx_ord_from_float(r.x), y = vgx_ord_from_float(r.y);
						lox = umin32(lox, x); loy = umin32(loy, y); hix = umax32(hix, x); hiy = umax32(hiy, y);
					}
#pragma unroll
					for (int sh = 32; sh >= 1; sh >>= 1) {
						lox = umin32(lox, (uint32_t)__shfl_xor((int)lox, sh)); loy = umin32(loy, (uint32_t)__shfl_xor((int)loy, sh));
						hix = umax32(hix, (uint32_t)__shfl_xor((int)hix, sh)); hiy = umax32(hiy, (uint32_t)__shfl_xor((int)hiy, sh));
					}
					if (lane == 0) { // the mesh is this wave's alone (a duplicate of the entry stores the same bytes)
						((float4*)A.mesh_bounds)[s0.first_mesh + k0 + (uint64_t)t] =
							make_float4(vgx_float_from_ord(lox), vgx_float_from_ord(loy), vgx_float_from_ord(hix), vgx_float_from_ord(hiy));
					}
				}
			}
		}
		q = end;
	}
}

// waves of a kernel that spreads at most `bound` items (a bound the host knows), `perWave` of them to a wave at least
unsigned update_grid(uint64_t bound, uint64_t perWave)
{
	const uint64_t want = (bound + perWave - 1) / perWave;
	return (unsigned)(want < 1 ? 1 : (want > 32768 ? 32768 : want));
}

} // namespace

void vgx_launch_cache_layout(const vgx_cache_desc& cache, const vgx_cache_instance* inst, uint64_t ninst, vgx_cache_slot* slots, uint32_t* status,
                             void* partial, hipStream_t s)
{
	OpCacheLayout op;
	op.cache = cache; op.inst = inst; op.ninst = ninst; op.slots = slots; op.status = status;
	vgx_device_scan_small(op, (Sum3*)partial, s, ninst);
}

void vgx_launch_cache_update(const VgxUpdateArgs& a, void* partial, hipStream_t s)
{
	OpUpdateList op;
	op.A = a;
	vgx_device_scan_small(op, (Sum3*)partial, s, a.ndirty);
	if (!a.ndirty) { return; }
	// The totals stay on the device. The host knows bounds: every listed entry has at most the cache's vertices / meshes. Waves
	// without a range exit at once.
	const uint64_t big = ~0ull;
	const uint64_t vb = a.cache.num_vertices && a.ndirty > big / a.cache.num_vertices ? big : a.ndirty * a.cache.num_vertices;
	const uint64_t mb = a.cache.num_meshes && a.ndirty > big / a.cache.num_meshes ? big : a.ndirty * a.cache.num_meshes;
	if (vb) { hipLaunchKernelGGL(k_update_pos, dim3(update_grid(vb, 256)), dim3(VGX_WAVE), 0, s, a); }
	if (mb) {
		if (a.mesh_bounds) { hipLaunchKernelGGL(k_update_meshes<1>, dim3(update_grid(mb, 1)), dim3(VGX_WAVE), 0, s, a); }
		else { hipLaunchKernelGGL(k_update_meshes<0>, dim3(update_grid(mb, 1)), dim3(VGX_WAVE), 0, s, a); }
	}
}
