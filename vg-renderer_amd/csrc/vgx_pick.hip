// vgx_pick.hip -- hit testing of points against a mesh stream on gfx950 (include/vgx.h: vgx_pick; the arithmetic: vgx_pick.h).
//
// Meshes run from 4 to 65 535 vertices and a point lies in very few boxes, so the box stage is spread by MESH and the triangle stage by
// TRIANGLE of the meshes that are left:
//   k_pick_meshes   one lane per mesh, the queries staged once per workgroup in LDS (4 KB at most): a mesh is a candidate iff it has a
//                   triangle and some query with mesh_end > m lies in its box; writes the mesh's triangle count, 0 for a non-candidate.
//                   Its first workgroup resets the key table: the call cleans up after the one before it
//   scan OpPickCand (vgx_scan.h) the dense ascending candidate list and the exclusive prefix of the candidates' triangle counts in one
//                   pass; the totals stay on the device
//   k_pick_tris     fixed grid, grid-stride over tiles of 256 entries of the candidate-triangle prefix; a wave finds the owners of its 64
//                   triangles by wave_owners (vgx_wave.h). A lane loads three uint16 indices, gathers three positions (and three
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
		const WaveOwners o = wave_owners(A.cand_prefix, numCand, totalTris, T0, lane); // every candidate has a triangle: P is strictly ascending
		uint32_t m = 0, t = 0;
		V2 a = v2(0.0f, 0.0f), b = a, c = a;
		bool ok = false, transparent = false;
		if (o.live) {
			m = A.cand_mesh[o.c0 + (uint64_t)o.k];
			t = (uint32_t)(T0 + (uint64_t)lane - o.first);
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

// ---- vgx_pick_frame: hit testing under scissors, clip regions and contour fills (include/vgx.h; the arithmetic: vgx_pick.h) -----------
// Whether mesh m is a hit depends on the stamp, and the stamp on which clip meshes below m cover the point: one maximum no longer
// answers. Coverage is decided per (candidate, query) first, into one bit each, and a last stage walks every query's bits in mesh order:
//   k_pickf_meshes    one lane per mesh of the range, the queries' points staged once per workgroup in LDS (6 KB): the mesh's state under
//                     its draw (vgx_pickf_mesh_state) and whether it is a candidate -- it has an element, and some point lies in its
//                     box and in its draw's scissor. Not filtered by mesh_end: a clip mesh below a hit counts whatever the query asks for
//   scan OpPickfCand  (vgx_scan.h) the dense ascending candidate list, the triangle candidates with the exclusive prefix of their
//                     triangle counts, the contour candidates, the candidates' covered rows zeroed, and the count of meshes with
//                     draw >= num_draws: dev_status is decided there, in one reduction
//   k_pickf_tris      k_pick_tris's traversal with the raster's coverage rule, set up once per lane. Per query and wave ONE atomicOr
//                     per candidate with a covering lane
//   k_pickf_contours  one wave per (contour candidate, 64 queries): a lane is a query, the mesh's edges are set up 64 at a time, one per
//                     lane, and broadcast from LDS; each lane sums its own W in an int32 -- no reduction, no atomics, and integer
//                     addition gives the same W in any order. The wave owns its two words of the candidate's row: plain stores
//   k_pickf_resolve   one workgroup per query over the candidates in ascending chunks of 256: "the last covered clip mesh so far"
//                     (stamper_before_me, vgx_wave.h), its draw is the S a lane tests against; the answer is the highest passing
//                     lane. The same workgroup then finds the largest covering triangle of the winner and writes the record
// No host round trip, no count comes back, every table is sized by the range. Bits are ORed and maxima taken: the same result every run.
namespace {

#define VGX_PICKF_CAND    0x100u // beside the mode in VgxPickfMesh::mode: the mesh is a candidate
#define VGX_PICKF_CONTOUR 0x200u // ... and of kind VGX_MESH_CONTOURS

struct PickfQuery : VgxPickStagedPoint { uint32_t mesh_end, flags; }; // 24 bytes

__device__ __forceinline__ PickfQuery pickf_query(const vgx_pick_query Q)
{
	PickfQuery P;
	P.mesh_end = Q.mesh_end;
	P.flags = vgx_pick_stage_point(Q.x, Q.y, Q.flags, true, &P);
	return P;
}

__global__ __launch_bounds__(256) void k_pickf_meshes(VgxPickfArgs A)
{
	__shared__ PickfQuery s_q[VGX_PICK_MAX_QUERIES];
	if (threadIdx.x < A.nqueries) { s_q[threadIdx.x] = pickf_query(A.queries[threadIdx.x]); }
	__syncthreads();
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= A.nrange) { return; }
	const uint64_t m = A.mesh_begin + r;
	const vgx_mesh me = A.meshes[m];
	VgxPickfMesh st;
	if (me.draw >= A.num_draws) {
		st.mode = VGX_RF_INVALID; st.f = st.n = st.elems = 0u; st.rect[0] = st.rect[1] = st.rect[2] = st.rect[3] = 0u;
	} else {
		vgx_pickf_mesh_state(me, A.draws[me.draw].state_key, A.draw_state[me.draw], &st);
		const float4 b4 = ((const float4*)A.mesh_bounds)[m];
		const float box[4] = { b4.x, b4.y, b4.z, b4.w };
		bool cand = false;
		if (st.elems) {
			for (uint32_t q = 0; q < A.nqueries; ++q) {
				const PickfQuery Q = s_q[q];
				cand = cand || ((Q.flags & VGX_PICK_STAGED_VALID) && vgx_pickf_in_scissor(st.rect, Q.X, Q.Y) && vgx_pickf_in_box(box, (double)Q.x, (double)Q.y));
			}
		}
		if (cand) { st.mode |= VGX_PICKF_CAND | (vgx_raster_kind_is_contours(me.subpath_kind) ? VGX_PICKF_CONTOUR : 0u); }
	}
	A.mesh_state[r] = st;
}

struct OpPickfCand // order-preserving compaction of the candidates and of their two kinds; the triangle prefix and the status ride along
{
	const VgxPickfMesh* meshState;
	uint64_t nrange;
	uint32_t* candMesh; uint32_t* triCand; uint64_t* triPrefix; uint32_t* conCand; uint32_t* cover;
	uint64_t* totals;
	uint32_t* status;
	__device__ uint64_t size() const { return nrange; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t mode = meshState[i].mode;
		if (mode & VGX_PICKF_CAND) {
			r.a = 1u;
			if (mode & VGX_PICKF_CONTOUR) { r.c = 1u; } else { r.b = meshState[i].elems; }
		}
		r.d = mode == VGX_RF_INVALID ? 1u : 0u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		const uint32_t mode = meshState[i].mode;
		if (!(mode & VGX_PICKF_CAND)) { return; }
		candMesh[e.a] = (uint32_t)i;
		uint4* row = (uint4*)(cover + 8u * e.a);
		row[0] = make_uint4(0u, 0u, 0u, 0u); row[1] = make_uint4(0u, 0u, 0u, 0u);
		if (mode & VGX_PICKF_CONTOUR) { conCand[e.c] = (uint32_t)e.a; }
		else { triCand[e.a - e.c] = (uint32_t)e.a; triPrefix[e.a - e.c] = e.b; }
	}
	__device__ void finish(Sum3 t) const
	{
		totals[0] = t.a; totals[1] = t.b; totals[2] = t.c; totals[3] = t.d;
		triPrefix[t.a - t.c] = t.b;
		if (status) { *status = t.d ? (uint32_t)VGX_E_INVALID_ARG : (uint32_t)VGX_OK; }
	}
};

__global__ __launch_bounds__(256) void k_pickf_tris(VgxPickfArgs A)
{
	__shared__ PickfQuery s_q[VGX_PICK_MAX_QUERIES];
	bool wantAlpha = false;
	if (threadIdx.x < A.nqueries) {
		const vgx_pick_query Q = A.queries[threadIdx.x];
		s_q[threadIdx.x] = pickf_query(Q);
		wantAlpha = (Q.flags & VGX_PICK_SKIP_TRANSPARENT) != 0;
	}
	const bool anyAlpha = __syncthreads_or(wantAlpha ? 1 : 0) != 0;
	const uint64_t numTri = A.totals[0] - A.totals[2], totalTris = A.totals[1];
	const uint64_t numTiles = (totalTris + VGX_PICK_TILE - 1) / VGX_PICK_TILE;
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	for (uint64_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
		const uint64_t T0 = tile * VGX_PICK_TILE + (uint64_t)wave * VGX_WAVE;
		if (T0 >= totalTris) { continue; } // the last tile's empty waves; nothing below synchronises the workgroup
		const WaveOwners o = wave_owners(A.tri_prefix, numTri, totalTris, T0, lane); // every triangle candidate has a triangle: P is strictly ascending
		// the lanes of one candidate are consecutive: my candidate's lanes as a mask, for "one atomic per candidate"
		const int kPrev = __shfl_up(o.k, 1);
		const uint64_t heads = wave_ballot(lane == 0 || o.k != kPrev);
		const uint64_t segBelow = lanemask_ge(seg_head(heads, lane)) & lanemask_lt(lane); // my candidate's lanes below me
		uint32_t c = 0, mode = 0;
		uint32_t rect[4] = { 0u, 0u, 0u, 0u };
		float box[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		VgxRasterTri Tri;
		bool ok = false, transparent = false;
		if (o.live) {
			c = A.tri_cand[o.c0 + (uint64_t)o.k];
			const uint32_t r = A.cand_mesh[c];
			const uint32_t t = (uint32_t)(T0 + (uint64_t)lane - o.first);
			const uint64_t m = A.mesh_begin + r;
			const vgx_mesh me = A.meshes[m];
			const uint16_t* ip = A.idx + me.first_index + 3ull * t;
			const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
			if (vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) {
				const float2* pp = (const float2*)A.pos + me.first_vertex;
				const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
				ok = vgx_raster_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), 0u, 0u, 0u, &Tri);
				if (ok) {
					const uint4* sp = (const uint4*)(A.mesh_state + r);
					const uint4 s0 = sp[0], s1 = sp[1];
					mode = s0.x & 0xFFu;
					rect[0] = s1.x; rect[1] = s1.y; rect[2] = s1.z; rect[3] = s1.w;
					const float4 b4 = ((const float4*)A.mesh_bounds)[m];
					box[0] = b4.x; box[1] = b4.y; box[2] = b4.z; box[3] = b4.w;
					if (anyAlpha) {
						const uint32_t* cp = A.color + me.first_vertex;
						transparent = vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2]);
					}
				}
			}
		}
		if (!wave_ballot(ok)) { continue; }
		for (uint32_t q = 0; q < A.nqueries; ++q) {
			const PickfQuery Q = s_q[q];
			if (!(Q.flags & VGX_PICK_STAGED_VALID)) { continue; }
			const double px = (double)Q.x, py = (double)Q.y;
			double E[3], S;
			const bool hit = ok && !(transparent && vgx_pickf_skips(mode, Q.flags)) && vgx_pickf_in_scissor(rect, Q.X, Q.Y) && vgx_pickf_in_box(box, px, py)
			              && vgx_raster_cover(Tri, px, py, E, &S);
			const uint64_t hits = wave_ballot(hit);
			if (hit && !(hits & segBelow)) { atomicOr(A.cover + 8ull * c + (q >> 5), 1u << (q & 31u)); }
		}
	}
}

struct PickfEdge { VgxRasterEdge e; float uy, vy; uint32_t flags, valid; }; // 40 bytes: what vgx_raster_contour_winding reads of a VgxRasterTri

__global__ __launch_bounds__(VGX_WAVE) void k_pickf_contours(VgxPickfArgs A)
{
	__shared__ PickfEdge s_e[VGX_WAVE];
	const uint64_t numCon = A.totals[2];
	const uint32_t groups = (A.nqueries + VGX_WAVE - 1) / VGX_WAVE;
	const int lane = threadIdx.x;
	for (uint64_t item = blockIdx.x; item < numCon * groups; item += gridDim.x) { // uniform over the wave = the workgroup
		const uint32_t g = (uint32_t)(item % groups);
		const uint32_t c = A.con_cand[item / groups];
		const uint32_t r = A.cand_mesh[c];
		const uint64_t m = A.mesh_begin + r;
		const vgx_mesh me = A.meshes[m];
		const VgxPickfMesh st = A.mesh_state[r];
		const float4 b4 = ((const float4*)A.mesh_bounds)[m];
		const float box[4] = { b4.x, b4.y, b4.z, b4.w };
		const uint32_t q = g * VGX_WAVE + (uint32_t)lane;
		double px = 0.0, py = 0.0;
		bool elig = false;
		if (q < A.nqueries) {
			const vgx_pick_query Q = A.queries[q];
			int32_t X, Y;
			elig = vgx_pickf_point(Q.x, Q.y, &px, &py, &X, &Y) && vgx_pickf_in_scissor(st.rect, X, Y) && vgx_pickf_in_box(box, px, py)
			    && !(vgx_pickf_skips(st.mode & 0xFFu, Q.flags) && (A.color[me.first_vertex] >> 24) == 0u);
		}
		const uint16_t* ip = A.idx + me.first_index;
		const float2* pp = (const float2*)A.pos + me.first_vertex;
		int32_t W = 0;
		for (uint32_t base = 0; base < st.elems; base += VGX_WAVE) {
			const uint32_t e = base + (uint32_t)lane;
			PickfEdge rec;
			rec.valid = 0u; rec.flags = 0u; rec.uy = rec.vy = 0.0f; rec.e.lox = rec.e.loy = 0.0f; rec.e.dx = rec.e.dy = 0.0;
			if (e < st.elems) {
				const uint32_t i0 = ip[2ull * e], i1 = ip[2ull * e + 1];
				if (i0 < me.num_vertices && i1 < me.num_vertices) {
					const float2 u = pp[i0], v = pp[i1];
					VgxRasterTri T;
					if (vgx_raster_contour_edge(v2(u.x, u.y), v2(v.x, v.y), &T)) { rec.e = T.e[0]; rec.flags = T.flags; rec.uy = T.miny; rec.vy = T.maxy; rec.valid = 1u; }
				}
			}
			s_e[lane] = rec;
			__syncthreads();
			const uint32_t cnt = st.elems - base < VGX_WAVE ? st.elems - base : VGX_WAVE;
			for (uint32_t k = 0; k < cnt; ++k) {
				const PickfEdge R = s_e[k];
				if (!R.valid) { continue; }
				VgxRasterTri T;
				T.e[0] = R.e; T.flags = R.flags; T.miny = R.uy; T.maxy = R.vy;
				W += vgx_raster_contour_winding(T, px, py);
			}
			__syncthreads();
		}
		const uint64_t mask = wave_ballot(elig && vgx_raster_contour_covered(W, me.subpath_kind, box, px, py));
		if (lane == 0) { A.cover[8ull * c + 2u * g] = (uint32_t)mask; A.cover[8ull * c + 2u * g + 1u] = (uint32_t)(mask >> 32); }
	}
}

__global__ __launch_bounds__(256) void k_pickf_resolve(VgxPickfArgs A)
{
	__shared__ uint32_t s_w[4];
	const uint32_t q = blockIdx.x, tid = threadIdx.x;
	const vgx_pick_query Q = A.queries[q];
	double px, py;
	int32_t X, Y;
	const bool point = vgx_pickf_point(Q.x, Q.y, &px, &py, &X, &Y);
	const uint64_t numCand = point && A.totals[3] == 0 ? A.totals[0] : 0; // a mesh with draw >= num_draws: every hit is "none"
	uint32_t carry = 0, best = 0; // candidate numbers + 1: the last covered clip mesh of the chunks before, my highest hit
	for (uint64_t base = 0; base < numCand; base += 256) {
		const uint64_t c = base + tid;
		bool covered = c < numCand && ((A.cover[8ull * c + (q >> 5)] >> (q & 31u)) & 1u) != 0u;
		if (!__syncthreads_or(covered ? 1 : 0)) { continue; }
		uint32_t r = 0, mode = VGX_RF_NOTHING, f = 0, n = 0;
		if (covered) {
			r = A.cand_mesh[c];
			const uint4 s0 = *(const uint4*)(A.mesh_state + r);
			mode = s0.x & 0xFFu; f = s0.y; n = s0.z;
		}
		const uint32_t stamper = stamper_before_me(covered && mode == VGX_RF_STAMP ? (uint32_t)c + 1u : 0u, &carry, s_w);
		if (covered && mode != VGX_RF_STAMP) {
			const uint32_t S = stamper ? A.mesh_state[A.cand_mesh[stamper - 1u]].f : VGX_RASTER_STAMP_NONE;
			if (vgx_pickf_hit(mode, f, n, S, A.mesh_begin + r, Q.mesh_end)) { best = (uint32_t)c + 1u; }
		}
	}
	best = block_max_u32(best, s_w);
	uint32_t mesh = VGX_PICK_NONE, top = 0;
	if (best) { // uniform over the workgroup
		const uint32_t r = A.cand_mesh[best - 1u];
		const VgxPickfMesh st = A.mesh_state[r];
		mesh = (uint32_t)(A.mesh_begin + r);
		if (!(st.mode & VGX_PICKF_CONTOUR)) {
			const vgx_mesh me = A.meshes[mesh];
			const uint16_t* ip = A.idx + me.first_index;
			const float2* pp = (const float2*)A.pos + me.first_vertex;
			const uint32_t* cp = A.color + me.first_vertex;
			const bool skips = vgx_pickf_skips(st.mode & 0xFFu, Q.flags);
			for (uint32_t t = tid; t < st.elems; t += 256) {
				const uint32_t i0 = ip[3ull * t], i1 = ip[3ull * t + 1], i2 = ip[3ull * t + 2];
				if (!vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) { continue; }
				if (skips && vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2])) { continue; }
				const float2 p0 = pp[i0], p1 = pp[i1], p2 = pp[i2];
				if (vgx_pickf_tri(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), px, py)) { top = t + 1u; }
			}
		}
		top = block_max_u32(top, s_w);
	}
	if (tid == 0) { A.hits[q] = vgx_pickf_record(mesh, top - 1u, A.meshes); } // top == 0: a contour mesh, or no hit: 0xFFFFFFFF
}

} // namespace

void vgx_launch_pick_frame(const VgxPickfArgs& a, void* partial, uint32_t grid, hipStream_t s)
{
	if (a.nrange) { hipLaunchKernelGGL(k_pickf_meshes, dim3((unsigned)((a.nrange + 255) / 256)), dim3(256), 0, s, a); }
	OpPickfCand op;
	op.meshState = a.mesh_state; op.nrange = a.nrange; op.candMesh = a.cand_mesh; op.triCand = a.tri_cand; op.triPrefix = a.tri_prefix;
	op.conCand = a.con_cand; op.cover = a.cover; op.totals = a.totals; op.status = a.status;
	vgx_device_scan(op, (Sum3*)partial, s, a.nrange); // an empty range too: it leaves the totals and the status
	if (!a.nqueries) { return; }
	if (a.nrange) {
		hipLaunchKernelGGL(k_pickf_tris, dim3(grid), dim3(256), 0, s, a);
		hipLaunchKernelGGL(k_pickf_contours, dim3(grid), dim3(VGX_WAVE), 0, s, a);
	}
	hipLaunchKernelGGL(k_pickf_resolve, dim3(a.nqueries), dim3(256), 0, s, a);
}
