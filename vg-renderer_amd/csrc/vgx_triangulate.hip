// vgx_triangulate.hip -- vgx_concave_triangulate (include/vgx.h): concave fills that are one simple ring become triangles by ear
// clipping on the device; every other concave draw gets vgx_concave_contours' meshes (vgx_concave_lane.h) at its place.
//
// Placement needs the routes, and a route needs the whole clipping (STALLED is known last), so the call has four steps:
//   scan 1      per draw what can be said without geometry (no mesh / MULTI / TOO_LONG / "the ring decides") and the ring's vertex count;
//               the prefix over the deciding rings is their place in the triangle scratch
//   k_tri_decide  one workgroup per deciding draw: the ring into LDS (position + two 16-bit links per vertex), non-finite test, the
//               orientation's vertex by a block reduction, the O(V^2) edge-pair test spread over the threads, then ONE wave walks the
//               clipping loop in the rule's sequential order -- a candidate's containment test is spread over the lanes, "any inside" is
//               a ballot -- and leaves ring-local triangles in scratch
//   scan 2      routes -> sizes, offsets and mesh records, the capacities checked (VGX_E_NOSPACE with the exact need)
//   k_tri_emit  one workgroup per mesh-making draw writes the streams: a triangulated draw by tri_emit_vertex / tri_emit_index, a refused
//               one by contours_emit_vertex
// Nothing in the result goes through an atomic (the sticky status word aside, as everywhere): the bytes are the same every run.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_scan_ops.h"
#include "vgx_triangulate_lane.h"

namespace {

#define VGX_TRI_THREADS 256

struct OpTriClasses // scan 1
{
	VgxTriArgs A;
	__device__ uint64_t size() const { return A.ndraws; }
	__device__ uint32_t cls(uint64_t i, uint64_t* V) const
	{
		int made;
		const uint32_t c = tri_draw_class(A.draws[i], A.draw_info[i], A.subpaths, V, &made);
		if (made < 0) { set_status(A.totals, VGX_E_INVALID_ARG); }
		return c;
	}
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		uint64_t V;
		if (cls(i, &V) == VGX_TRI_ROUTE_TRIANGLES) { r.a = V; }
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		uint64_t V;
		const uint32_t c = cls(i, &V);
		A.route[i] = c; A.ring_vertices[i] = V; A.cand_prefix[i] = e.a;
		if (A.draw_route && c != VGX_TRI_ROUTE_TRIANGLES) { A.draw_route[i] = c; } // a deciding draw's word is k_tri_decide's
	}
	__device__ void finish(Sum3 t) const { A.cand_prefix[A.ndraws] = t.a; A.ring_vertices[A.ndraws] = 0; }
};

struct OpTriPlaces // scan 2
{
	VgxTriArgs A;
	__device__ uint64_t size() const { return A.ndraws; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t route = A.route[i];
		if (route == 0u) { return r; }
		uint32_t nm; bool big;
		tri_draw_sizes(A.draws[i], route, A.ring_vertices[i], &r.a, &r.b, &nm, &big);
		r.c = nm;
		if (big) { set_status(A.totals, VGX_E_MESH_TOO_LARGE); } // uint16 indices
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		A.vertex_prefix[i] = e.a; A.index_prefix[i] = e.b;
		const uint32_t route = A.route[i];
		if (route == 0u || !A.meshes) { return; }
		vgx_mesh m[2];
		const uint32_t n = tri_draw_meshes(A.draws[i], (uint32_t)i, route, A.ring_vertices[i], e.a, e.b, m);
		for (uint32_t k = 0; k < n; ++k) { if (e.c + k < A.cap_meshes) { A.meshes[e.c + k] = m[k]; } }
	}
	__device__ void finish(Sum3 t) const
	{
		A.vertex_prefix[A.ndraws] = t.a; A.index_prefix[A.ndraws] = t.b;
		A.totals->sizes.num_meshes = t.c;
		A.totals->sizes.num_vertices = t.a;
		A.totals->sizes.num_indices = t.b;
		if (t.a > A.cap_vertices || t.b > A.cap_indices || t.c > A.cap_meshes) { set_status(A.totals, VGX_E_NOSPACE); }
	}
};

__device__ __forceinline__ V2 lds_pos(const float2* p, uint32_t i)
{
	const float2 t = p[i];
	return v2(t.x, t.y);
}

// One workgroup per deciding draw. LDS: 12 bytes per ring vertex (48 KiB at the cap of 4096: three workgroups per CU)
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_decide(VgxTriArgs A)
{
	__shared__ float2 s_pos[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint16_t s_prev[VGX_TRIANGULATE_MAX_VERTICES], s_next[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint32_t s_min[VGX_TRI_THREADS];
	const uint32_t tid = threadIdx.x;
	for (uint64_t di = blockIdx.x; di < A.ndraws; di += gridDim.x) {
		if (A.route[di] != VGX_TRI_ROUTE_TRIANGLES) { continue; } // block-uniform
		__syncthreads(); // the previous ring's readers are done
		const vgx_draw d = A.draws[di];
		const vgx_subpath sp = A.subpaths[A.draw_info[di].first_subpath];
		const uint32_t V = sp.num_vertices; // 3 .. VGX_TRIANGULATE_MAX_VERTICES (tri_draw_class)
		const float* v = A.poly + 2 * sp.first_vertex;
		uint32_t route = VGX_TRI_ROUTE_TRIANGLES;

		// the ring, its links, the non-finite test, and this thread's smallest vertex by (x, y, index)
		bool bad = false;
		uint32_t k = 0xFFFFFFFFu;
		V2 pk = v2(0.0f, 0.0f);
		for (uint32_t j = tid; j < V; j += VGX_TRI_THREADS) {
			const V2 p = tri_ring_vertex(v, V, d, j);
			s_pos[j] = make_float2(p.x, p.y);
			s_prev[j] = (uint16_t)(j ? j - 1 : V - 1); s_next[j] = (uint16_t)(j + 1 < V ? j + 1 : 0);
			bad = bad || !tri_finite(p);
			if (k == 0xFFFFFFFFu || tri_before(p, j, pk, k)) { k = j; pk = p; }
		}
		s_min[tid] = k;
		if (__syncthreads_or(bad ? 1 : 0)) { route = VGX_TRI_REFUSED_NONFINITE; }

		double s = 0.0;
		if (route == VGX_TRI_ROUTE_TRIANGLES) {
			k = s_min[0]; // every thread folds the same candidates in the same order (broadcast reads)
			const uint32_t cands = V < VGX_TRI_THREADS ? V : VGX_TRI_THREADS;
			for (uint32_t t = 1; t < cands; ++t) {
				const uint32_t j = s_min[t];
				if (tri_before(lds_pos(s_pos, j), j, lds_pos(s_pos, k), k)) { k = j; }
			}
			s = (double)tri_sign(tri_edge(lds_pos(s_pos, s_prev[k]), lds_pos(s_pos, k), lds_pos(s_pos, s_next[k])));
			if (s == 0.0) { route = VGX_TRI_REFUSED_DEGENERATE; }
		}

		if (route == VGX_TRI_ROUTE_TRIANGLES) { // edge i against the edges i + 2 ..: the j of one i spread over the threads
			bool meet = false;
			for (uint32_t i = 0; i + 2 < V; ++i) {
				const V2 u1 = lds_pos(s_pos, i), v1 = lds_pos(s_pos, i + 1);
				for (uint32_t j = i + 2 + tid; j < V; j += VGX_TRI_THREADS) {
					if (i == 0 && j == V - 1) { continue; } // the closing edge shares vertex 0
					meet = meet || tri_edges_meet(u1, v1, lds_pos(s_pos, j), lds_pos(s_pos, j + 1 < V ? j + 1 : 0));
				}
			}
			if (__syncthreads_or(meet ? 1 : 0)) { route = VGX_TRI_REFUSED_NOT_SIMPLE; }
		}

		if (tid < 64) { // one wave, every lane with the same cursor; a link is stored by all lanes alike, so each reads back its own store
			const uint32_t lane = tid;
			const uint64_t first = 3 * A.cand_prefix[di];
			const bool keep = first + 3 * (uint64_t)V <= A.cap_tri; // beyond it the call ends with VGX_E_NOSPACE: the route is still needed
			uint16_t* tri = A.tri + first;
			if (route == VGX_TRI_ROUTE_TRIANGLES) {
				uint32_t b = 0, size = V, misses = 0, nt = 0;
				while (size > 3) {
					const uint32_t a = s_prev[b], c = s_next[b];
					const V2 pa = lds_pos(s_pos, a), pb = lds_pos(s_pos, b), pc = lds_pos(s_pos, c);
					const double t = s * tri_edge(pa, pb, pc);
					bool ear = t == 0.0;
					if (t > 0.0) {
						ear = true;
						for (uint32_t base = 0; base < V && ear; base += 64) {
							const uint32_t p = base + lane;
							bool inside = false;
							if (p < V && p != a && p != b && p != c && s_prev[p] != VGX_TRI_UNLINKED) { inside = tri_blocks(pa, pb, pc, lds_pos(s_pos, p), s); }
							ear = wave_ballot(inside) == 0ull;
						}
					}
					if (ear) {
						if (lane == 0 && keep) { tri[nt] = (uint16_t)a; tri[nt + 1] = (uint16_t)b; tri[nt + 2] = (uint16_t)c; }
						nt += 3;
						s_next[a] = (uint16_t)c; s_prev[c] = (uint16_t)a; s_prev[b] = VGX_TRI_UNLINKED;
						b = s_next[c]; --size; misses = 0;
					} else {
						b = c;
						if (++misses > size) { route = VGX_TRI_REFUSED_STALLED; break; }
					}
				}
				if (route == VGX_TRI_ROUTE_TRIANGLES && lane == 0 && keep) { tri[nt] = s_prev[b]; tri[nt + 1] = (uint16_t)b; tri[nt + 2] = s_next[b]; }
			}
			if (lane == 0) {
				A.route[di] = route;
				if (A.draw_route) { A.draw_route[di] = route; }
			}
		}
	}
}

// One workgroup per mesh-making draw. The sizes were checked against the capacities by scan 2: any status but VGX_OK and nothing is written
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_emit(VgxTriArgs A)
{
	if (A.totals->status != VGX_OK) { return; }
	for (uint64_t di = blockIdx.x; di < A.ndraws; di += gridDim.x) {
		const uint32_t route = A.route[di];
		if (route == 0u) { continue; }
		const vgx_draw d = A.draws[di];
		const vgx_draw_info info = A.draw_info[di];
		const vgx_subpath* sp = A.subpaths + info.first_subpath;
		const uint64_t V = A.ring_vertices[di], fv = A.vertex_prefix[di], fi = A.index_prefix[di];
		if (route == VGX_TRI_ROUTE_TRIANGLES) {
			const uint16_t* tri = A.tri + 3 * A.cand_prefix[di];
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) { tri_emit_vertex(A.poly, sp, d, c, V, fv, fi, A.pos, A.color, A.idx); }
			for (uint64_t k = threadIdx.x; k < 3 * (V - 2); k += VGX_TRI_THREADS) { tri_emit_index(d, tri, k, V, fi, A.idx); }
		} else {
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) {
				contours_emit_vertex(A.poly, sp, info.num_subpaths, d, c, V, fv, fi, A.pos, A.color, A.idx);
			}
		}
	}
}

} // namespace

void vgx_launch_concave_triangulate(const VgxTriArgs& a, void* partial, hipStream_t s)
{
	OpTriClasses classes; classes.A = a;
	vgx_device_scan(classes, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_decide, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a);
	}
	OpTriPlaces places; places.A = a;
	vgx_device_scan(places, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_emit, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a);
	}
}
