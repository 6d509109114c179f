// vgx_bounds.hip -- per-mesh bounding boxes of a mesh stream and view culling of shape-cache instances on gfx950.
//
// vgx_mesh_bounds: meshes run from 4 to 65 535 vertices, so the work is spread by VERTEX, not by mesh.
//   k_bounds_init    bounds[m] <- the empty box, as order-preserving uint32 images (vgx_bounds.h)
//   k_bounds_flat    a wave owns a contiguous range of the vertex stream (a multiple of 256 vertices, as k_cache_copy_flat does)
//                    and walks the meshes that intersect it: whole 8-byte vertices per lane (512 B per wave instruction), min / max
//                    as integers on the images, reduced across the wave per mesh. A mesh that lies wholly inside the range is
//                    stored plainly; one that crosses a range boundary is combined with atomicMin / atomicMax on the images --
//                    order independent and bitwise reproducible, one set of four per wave and crossing (no contention to speak of)
//   k_bounds_decode  images -> floats, in place
// The caller's `bounds` array is the only table: no scratch, no host synchronisation, nothing of the context is touched.
//
// vgx_cache_cull:
//   k_cache_cull     one lane per instance (vgx_bounds.h: range union -> corners through v2xform -> cull rule)
//   scan OpCullKept  (vgx_scan.h) the dense ascending list of the kept instances, skipped when the caller wants neither list nor count
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_bounds.h"

namespace {

struct OrdBox { uint32_t minx, miny, maxx, maxy; };

__device__ __forceinline__ OrdBox ord_empty() { OrdBox b; b.minx = VGX_ORD_POS_INF; b.miny = VGX_ORD_POS_INF; b.maxx = VGX_ORD_NEG_INF; b.maxy = VGX_ORD_NEG_INF; return b; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ void ord_add(OrdBox& b, float2 q)
{
	const uint32_t x = vgx_ord_from_float(q.x), y = vgx_ord_from_float(q.y);
	b.minx = umin32(b.minx, x); b.miny = umin32(b.miny, y); b.maxx = umax32(b.maxx, x); b.maxy = umax32(b.maxy, y);
}
__device__ __forceinline__ OrdBox ord_wave_reduce(OrdBox b)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		b.minx = umin32(b.minx, (uint32_t)__shfl_xor((int)b.minx, d)); b.miny = umin32(b.miny, (uint32_t)__shfl_xor((int)b.miny, d));
		b.maxx = umax32(b.maxx, (uint32_t)__shfl_xor((int)b.maxx, d)); b.maxy = umax32(b.maxy, (uint32_t)__shfl_xor((int)b.maxy, d));
	}
	return b;
}

__global__ __launch_bounds__(256) void k_bounds_init(uint4* table, uint64_t numMeshes)
{
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (m < numMeshes) { table[m] = make_uint4(VGX_ORD_POS_INF, VGX_ORD_POS_INF, VGX_ORD_NEG_INF, VGX_ORD_NEG_INF); }
}

__global__ __launch_bounds__(256) void k_bounds_decode(uint4* table, uint64_t numMeshes)
{
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= numMeshes) { return; }
	const uint4 o = table[m];
	float4 r;
	r.x = vgx_float_from_ord(o.x); r.y = vgx_float_from_ord(o.y); r.z = vgx_float_from_ord(o.z); r.w = vgx_float_from_ord(o.w);
	((float4*)table)[m] = r;
}

// Precondition (include/vgx.h): the mesh table is ascending in first_vertex. Whatever the table holds, only vertices inside a mesh's own range are read.
__global__ __launch_bounds__(VGX_WAVE) void k_bounds_flat(const float2* pos, const vgx_mesh* meshes, uint64_t numMeshes, uint32_t* table)
{
	const int lane = threadIdx.x;
	const uint64_t base = meshes[0].first_vertex;
	const vgx_mesh last = meshes[numMeshes - 1];
	const uint64_t stop = last.first_vertex + last.num_vertices;
	if (stop <= base) { return; }
	const uint64_t total = stop - base;
	// ranges are multiples of 256 vertices so that the 4x-unrolled loop below mostly runs full
	uint64_t per = (total + gridDim.x - 1) / gridDim.x;
	per = (per + 255) / 256 * 256;
	const uint64_t r0 = (uint64_t)blockIdx.x * per;
	if (r0 >= total) { return; }
	const uint64_t o0 = base + r0;
	const uint64_t o1 = r0 + per < total ? o0 + per : stop;
	// the last mesh that starts at or before o0 (0-vertex meshes in front of it share its start and keep the empty box)
	uint64_t m = 0;
	{
		uint64_t hi = numMeshes;
		while (hi - m > 1) {
			const uint64_t mid = (m + hi) >> 1;
			if (meshes[mid].first_vertex <= o0) { m = mid; } else { hi = mid; }
		}
	}
	// 64 mesh records at a time, one per lane, handed round by readlane: no dependent record load per mesh
	while (m < numMeshes) {
		const uint64_t mk = m + (uint64_t)lane;
		uint64_t fvL = ~0ull; uint32_t nvL = 0;
		if (mk < numMeshes) { fvL = meshes[mk].first_vertex; nvL = meshes[mk].num_vertices; }
		const uint64_t left = numMeshes - m;
		const int cnt = left < (uint64_t)VGX_WAVE ? (int)left : VGX_WAVE;
		bool done = false;
		for (int k = 0; k < cnt; ++k) {
			const uint64_t fv = wave_bcast_u64(fvL, k);
			const uint32_t nv = wave_bcast_u32(nvL, k);
			if (fv >= o1) { done = true; break; }
			const uint64_t fe = fv + nv;
			const uint64_t a = fv > o0 ? fv : o0;
			const uint64_t b = fe < o1 ? fe : o1;
			if (a >= b) { continue; } // ends in front of the range, or has no vertices
			OrdBox box = ord_empty();
			const float2* p = pos + a;
			const uint64_t n = b - a;
			uint64_t j = lane;
			for (; j + 3 * VGX_WAVE < n; j += 4 * VGX_WAVE) { // four independent 512-byte wave loads in flight
				const float2 q0 = p[j], q1 = p[j + VGX_WAVE], q2 = p[j + 2 * VGX_WAVE], q3 = p[j + 3 * VGX_WAVE];
				ord_add(box, q0); ord_add(box, q1); ord_add(box, q2); ord_add(box, q3);
			}
			for (; j < n; j += VGX_WAVE) { ord_add(box, p[j]); }
			box = ord_wave_reduce(box);
			if (lane == 0) {
				uint32_t* t = table + 4 * (m + (uint64_t)k);
				if (fv >= o0 && fe <= o1) { // wholly this wave's: nobody else touches the entry
					*(uint4*)t = make_uint4(box.minx, box.miny, box.maxx, box.maxy);
				} else {
					atomicMin(t + 0, box.minx); atomicMin(t + 1, box.miny); atomicMax(t + 2, box.maxx); atomicMax(t + 3, box.maxy);
				}
			}
		}
		if (done) { break; }
		m += (uint64_t)cnt;
	}
}

// ---- vgx_cache_cull ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cache_cull(VgxCullArgs A)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.ninst) { return; }
	vgx_cache_instance in = A.inst[i];
	const uint32_t view = A.inst_view ? A.inst_view[i] : 0u;
	const bool valid = vgx_cull_valid(in, A.cache_meshes, view, A.nviews);
	const VgxBox L = vgx_box_union_range(A.mesh_bounds, in.first_mesh, valid ? in.num_meshes : 0u);
	VgxBox B = vgx_box_empty();
	bool keep = false;
	if (valid) { keep = vgx_cull_decide(L, in.mtx, A.views + 4 * (uint64_t)view, &B); }
	else if (A.status) { *A.status = (uint32_t)VGX_E_INVALID_ARG; } // every writer stores the same word
	if (!keep) { in.num_meshes = 0; }
	if (!keep || A.out_inst != A.inst) { A.out_inst[i] = in; } // in place, a kept record stays as it is
	if (A.out_bounds) { *(float4*)(A.out_bounds + 4 * i) = make_float4(B.minx, B.miny, B.maxx, B.maxy); }
	if (A.flags) { A.flags[i] = keep ? 1u : 0u; }
}

struct OpCullKept // order-preserving compaction: kept[rank among the kept] = i
{
	const uint8_t* flags;
	uint64_t ninst;
	uint32_t* kept;
	uint64_t* numKept;
	__device__ uint64_t size() const { return ninst; }
	__device__ Sum3 load(uint64_t i) const { Sum3 r = sum3_zero(); r.a = flags[i]; return r; }
	__device__ void store(uint64_t i, Sum3 e) const { if (kept && flags[i]) { kept[e.a] = (uint32_t)i; } }
	__device__ void finish(Sum3 t) const { if (numKept) { *numKept = t.a; } }
};

} // namespace

void vgx_launch_mesh_bounds(const float* pos, const vgx_mesh* meshes, uint64_t numMeshes, float* bounds, hipStream_t s)
{
	const unsigned tb = (unsigned)((numMeshes + 255) / 256);
	hipLaunchKernelGGL(k_bounds_init, dim3(tb), dim3(256), 0, s, (uint4*)bounds, numMeshes);
	// the vertex count lives in the table (device memory): the grid follows the mesh count -- meshes have at least 4 vertices, so
	// 256 .. 32768 waves leave every wave a range of 256 vertices or more at frame size, and waves without a range exit at once
	const uint64_t g = numMeshes < 256 ? 256 : (numMeshes > 32768 ? 32768 : numMeshes);
	hipLaunchKernelGGL(k_bounds_flat, dim3((unsigned)g), dim3(VGX_WAVE), 0, s, (const float2*)pos, meshes, numMeshes, (uint32_t*)bounds);
	hipLaunchKernelGGL(k_bounds_decode, dim3(tb), dim3(256), 0, s, (uint4*)bounds, numMeshes);
}

void vgx_launch_cache_cull(const VgxCullArgs& a, uint32_t* kept, uint64_t* numKept, void* partial, hipStream_t s)
{
	if (a.ninst) {
		hipLaunchKernelGGL(k_cache_cull, dim3((unsigned)((a.ninst + 255) / 256)), dim3(256), 0, s, a);
	}
	if (kept || numKept) {
		OpCullKept op;
		op.flags = a.flags; op.ninst = a.ninst; op.kept = kept; op.numKept = numKept;
		vgx_device_scan(op, (Sum3*)partial, s, a.ninst);
	}
}
