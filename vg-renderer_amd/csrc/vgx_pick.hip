// vgx_pick.hip -- hit testing of points against a mesh stream on gfx950 (include/vgx.h: vgx_pick; the arithmetic: vgx_pick.h).
//
// Meshes run from 4 to 65 535 vertices and a point lies in very few boxes, so the box stage is spread by MESH and the triangle stage by
// TRIANGLE of the meshes that are left:
//   k_pick_meshes   one lane per mesh, the queries staged once per workgroup in LDS (4 KB at most): a mesh is a candidate iff it has a
//                   triangle and some query with mesh_end > m lies in its box; writes the mesh's triangle count, 0 for a non-candidate.
//                   Its first workgroup resets the key table: the call cleans up after the one before it
//   scan OpPickCand (vgx_scan.h) the dense ascending candidate list and the exclusive prefix of the candidates' triangle counts in one
//                   pass; the totals stay on the device
//   k_pick_tris     fixed grid, grid-stride over tiles of 256 entries of the candidate-triangle prefix. A wave finds the candidate of its
//                   first triangle by binary search and holds the 64 prefix entries from there one per lane: every candidate has a
//                   triangle, so its 64 triangles lie in those. A lane loads three uint16 indices, gathers three positions (and three
//                   colours when some query asks for the transparency rule), then runs the queries from LDS in a wave-uniform loop:
//                   mesh_end, the triangle's box, the binary64 predicate. Lanes are in ascending (mesh, triangle) order, so the highest
//                   lane that hits holds the wave's largest key: no reduction, ONE 64-bit atomicMax per wave and query with a hit
//   k_pick_finish   one lane per query: key -> vgx_pick_hit
// No host round trip, no count comes back. A maximum is order independent, so the result is the same on every run.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_pick.h"

namespace {

#define VGX_PICK_TILE 256

__global__ __launch_bounds__(256) void k_pick_meshes(VgxPickArgs A)
{
	__shared__ vgx_pick_query s_q[VGX_PICK_MAX_QUERIES];
	if (threadIdx.x < A.nqueries) { s_q[threadIdx.x] = A.queries[threadIdx.x]; }
	if (blockIdx.x == 0 && threadIdx.x < VGX_PICK_MAX_QUERIES) { A.keys[threadIdx.x] = 0ull; }
	__syncthreads();
	const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= A.num_meshes) { return; }
	const uint32_t tris = vgx_pick_mesh_triangles(A.meshes[m]);
	const float4 box = ((const float4*)A.mesh_bounds)[m];
	bool cand = false;
	if (tris) {
		for (uint32_t q = 0; q < A.nqueries; ++q) {
			const vgx_pick_query Q = s_q[q];
			cand = cand || ((uint64_t)Q.mesh_end > m && vgx_pick_in_box(Q.x, Q.y, box.x, box.y, box.z, box.w));
		}
	}
	A.cand_tris[m] = cand ? tris : 0u;
}

struct OpPickCand // order-preserving compaction of the candidates, with the prefix of their triangle counts riding along
{
	const uint32_t* candTris;
	uint64_t numMeshes;
	uint32_t* candMesh;
	uint64_t* candPrefix; // [numCand + 1]
	uint64_t* totals;     // numCand, total triangles
	__device__ uint64_t size() const { return numMeshes; }
	__device__ Sum3 load(uint64_t i) const { Sum3 r = sum3_zero(); const uint32_t t = candTris[i]; r.a = t ? 1u : 0u; r.b = t; return r; }
	__device__ void store(uint64_t i, Sum3 e) const { if (candTris[i]) { candMesh[e.a] = (uint32_t)i; candPrefix[e.a] = e.b; } }
	__device__ void finish(Sum3 t) const { totals[0] = t.a; totals[1] = t.b; candPrefix[t.a] = t.b; }
};

__global__ __launch_bounds__(256) void k_pick_tris(VgxPickArgs A)
{
	__shared__ vgx_pick_query s_q[VGX_PICK_MAX_QUERIES];
	bool wantAlpha = false;
	if (threadIdx.x < A.nqueries) {
		const vgx_pick_query Q = A.queries[threadIdx.x];
		s_q[threadIdx.x] = Q;
		wantAlpha = (Q.flags & VGX_PICK_SKIP_TRANSPARENT) != 0;
	}
	const bool anyAlpha = __syncthreads_or(wantAlpha ? 1 : 0) != 0;
	const uint64_t numCand = A.totals[0], totalTris = A.totals[1];
	const uint64_t numTiles = (totalTris + VGX_PICK_TILE - 1) / VGX_PICK_TILE;
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	for (uint64_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
		const uint64_t T0 = tile * VGX_PICK_TILE + (uint64_t)wave * VGX_WAVE;
		if (T0 >= totalTris) { continue; } // the last tile's empty waves; nothing below synchronises the workgroup
		// the candidate that owns T0 (P[0] = 0 <= T0 < P[numCand] = totalTris; P is strictly ascending), then 64 entries from there
		const uint64_t c0 = find_owner_u64(A.cand_prefix, 0, numCand, T0);
		const uint64_t ck = c0 + (uint64_t)lane;
		const uint64_t w = ck <= numCand ? A.cand_prefix[ck] : ~0ull;
		const uint64_t T = T0 + (uint64_t)lane;
		const bool live = T < totalTris;
		uint64_t first = 0;
		const int k = window_owner(w, live ? T : T0, &first);
		uint32_t m = 0, t = 0;
		V2 a = v2(0.0f, 0.0f), b = a, c = a;
		bool ok = false, transparent = false;
		if (live) {
			m = A.cand_mesh[c0 + (uint64_t)k];
			t = (uint32_t)(T - first);
			const vgx_mesh me = A.meshes[m];
			const uint16_t* ip = A.idx + me.first_index + 3ull * t;
			const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
			ok = vgx_pick_tri_valid(i0, i1, i2, me.num_vertices);
			if (ok) {
				const float2* pp = (const float2*)A.pos + me.first_vertex;
				const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
				a = v2(p0.x, p0.y); b = v2(p1.x, p1.y); c = v2(p2.x, p2.y);
				if (anyAlpha) {
					const uint32_t* cp = A.color + me.first_vertex;
					transparent = vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2]);
				}
			}
		}
		if (!wave_ballot(ok)) { continue; }
		const uint64_t key = vgx_pick_key(m, t);
		for (uint32_t q = 0; q < A.nqueries; ++q) {
			const vgx_pick_query Q = s_q[q];
			const bool hit = ok && Q.mesh_end > m && !((Q.flags & VGX_PICK_SKIP_TRANSPARENT) && transparent) && vgx_pick_tri(a, b, c, Q.x, Q.y);
			const uint64_t hits = wave_ballot(hit);
			// keys ascend with the lane: the highest hit lane holds the wave's maximum
			if (hits && lane == 63 - __clzll((long long)hits)) { atomicMax((unsigned long long*)(A.keys + q), (unsigned long long)key); }
		}
	}
}

__global__ __launch_bounds__(VGX_PICK_MAX_QUERIES) void k_pick_finish(VgxPickArgs A)
{
	const uint32_t q = threadIdx.x;
	if (q < A.nqueries) { A.hits[q] = vgx_pick_decode(A.keys[q], A.meshes); }
}

} // namespace

void vgx_launch_pick(const VgxPickArgs& a, void* partial, uint32_t grid, hipStream_t s)
{
	// at least one workgroup even without meshes: it resets the key table
	const uint64_t tb = a.num_meshes ? (a.num_meshes + 255) / 256 : 1;
	hipLaunchKernelGGL(k_pick_meshes, dim3((unsigned)tb), dim3(256), 0, s, a);
	OpPickCand op;
	op.candTris = a.cand_tris; op.numMeshes = a.num_meshes; op.candMesh = a.cand_mesh; op.candPrefix = a.cand_prefix; op.totals = a.totals;
	vgx_device_scan(op, (Sum3*)partial, s, a.num_meshes);
	if (a.nqueries) {
		if (a.num_meshes) { hipLaunchKernelGGL(k_pick_tris, dim3(grid), dim3(256), 0, s, a); }
		hipLaunchKernelGGL(k_pick_finish, dim3(1), dim3(VGX_PICK_MAX_QUERIES), 0, s, a);
	}
}
