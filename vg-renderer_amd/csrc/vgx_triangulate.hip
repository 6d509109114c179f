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
// vgx_concave_triangulate_rings (further down) is the same four steps with kernels of its own for draws of one outer ring with holes,
// vgx_concave_triangulate_nested (below it) for draws of several outlines and islands in holes.
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

// ---- vgx_concave_triangulate_rings: the same four steps for draws of one outer ring with holes ------------------------------------------
// The scans carry H = num_subpaths - 1 per draw (it is in the draw's info): a deciding draw takes V + 2 H slots of triangle scratch and,
// triangulated, 3 (V + 2 H - 2) indices. k_tri_decide and k_tri_emit above are not launched by this entry and not touched by it.
struct OpTriRingsClasses : OpTriClasses // scan 1
{
	__device__ uint32_t cls(uint64_t i, uint64_t* V, uint32_t* H) const
	{
		int made;
		const uint32_t c = tri_rings_draw_class(A.draws[i], A.draw_info[i], A.subpaths, V, H, &made);
		if (made < 0) { set_status(A.totals, VGX_E_INVALID_ARG); }
		return c;
	}
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		uint64_t V; uint32_t H;
		if (cls(i, &V, &H) == VGX_TRI_ROUTE_TRIANGLES) { r.a = V + 2ull * H; }
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		uint64_t V; uint32_t H;
		const uint32_t c = cls(i, &V, &H);
		A.route[i] = c; A.ring_vertices[i] = V; A.cand_prefix[i] = e.a;
		if (A.draw_route && c != VGX_TRI_ROUTE_TRIANGLES) { A.draw_route[i] = c; } // a deciding draw's word is k_tri_decide_rings'
	}
};

struct OpTriRingsPlaces : OpTriPlaces // scan 2
{
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t route = A.route[i];
		if (route == 0u) { return r; }
		uint32_t nm; bool big;
		tri_rings_draw_sizes(A.draws[i], route, A.ring_vertices[i], A.draw_info[i].num_subpaths - 1u, &r.a, &r.b, &nm, &big);
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
		const uint32_t n = tri_rings_draw_meshes(A.draws[i], (uint32_t)i, route, A.ring_vertices[i], A.draw_info[i].num_subpaths - 1u, e.a, e.b, m);
		for (uint32_t k = 0; k < n; ++k) { if (e.c + k < A.cap_meshes) { A.meshes[e.c + k] = m[k]; } }
	}
};

#define VGX_TRI_NONE 0xFFFFFFFFu

// the smallest (or greatest) vertex by (x, y, index) over the wave, on every lane; i == VGX_TRI_NONE: this lane has none
__device__ __forceinline__ uint32_t wave_extreme_vertex(V2 p, uint32_t i, bool greatest)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const V2 o = v2(__shfl_xor(p.x, d), __shfl_xor(p.y, d));
		const uint32_t oi = (uint32_t)__shfl_xor((int)i, d);
		const bool take = oi != VGX_TRI_NONE && (i == VGX_TRI_NONE || (greatest ? tri_before(p, i, o, oi) : tri_before(o, oi, p, i)));
		if (take) { p = o; i = oi; }
	}
	return i;
}

// the smallest key (d2, slot) over the workgroup, on every thread; slot == VGX_TRI_NONE: this thread has none. Two barriers
__device__ __forceinline__ void block_min_key(double* d2, uint32_t* slot, double* s_d, uint32_t* s_s)
{
	double k = *d2; uint32_t x = *slot;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const double ok = __shfl_xor(k, d);
		const uint32_t ox = (uint32_t)__shfl_xor((int)x, d);
		if (ox != VGX_TRI_NONE && (x == VGX_TRI_NONE || tri_key_less(ok, ox, k, x))) { k = ok; x = ox; }
	}
	if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = k; s_s[threadIdx.x >> 6] = x; }
	__syncthreads();
	k = s_d[0]; x = s_s[0];
	for (int w = 1; w < VGX_TRI_THREADS / 64; ++w) {
		const double ok = s_d[w]; const uint32_t ox = s_s[w];
		if (ox != VGX_TRI_NONE && (x == VGX_TRI_NONE || tri_key_less(ok, ox, k, x))) { k = ok; x = ox; }
	}
	__syncthreads();
	*d2 = k; *slot = x;
}

// One workgroup per deciding draw. LDS by the compiler's report: 61 776 bytes -- 8 bytes of position per vertex, a 16-bit slot -> vertex
// map and two 16-bit links per slot at the cap of 4096 slots (56 KiB), three small per-ring tables and the reduction's words -- so two
// workgroups per CU (160 KiB) whatever the draws hold. `route` is block-uniform throughout: every change comes out of a barrier
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_decide_rings(VgxTriArgs A)
{
	__shared__ float2 s_pos[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint16_t s_vert[VGX_TRIANGULATE_MAX_VERTICES], s_prev[VGX_TRIANGULATE_MAX_VERTICES], s_next[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint16_t s_mh[VGX_TRI_MAX_RINGS], s_lo[VGX_TRI_MAX_RINGS]; // per ring its greatest and its smallest vertex; s_lo later: the holes in processing order
	__shared__ int8_t s_sgn[VGX_TRI_MAX_RINGS];
	__shared__ double s_rd[VGX_TRI_THREADS / 64];
	__shared__ uint32_t s_rs[VGX_TRI_THREADS / 64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	for (uint64_t di = blockIdx.x; di < A.ndraws; di += gridDim.x) {
		if (A.route[di] != VGX_TRI_ROUTE_TRIANGLES) { continue; } // block-uniform
		__syncthreads(); // the previous draw's readers are done
		const vgx_draw d = A.draws[di];
		const vgx_draw_info info = A.draw_info[di];
		const vgx_subpath* sp = A.subpaths + info.first_subpath;
		const uint32_t S = info.num_subpaths, H = S - 1u;
		const uint32_t V = (uint32_t)A.ring_vertices[di], N = V + 2u * H; // N <= VGX_TRIANGULATE_MAX_VERTICES, S <= VGX_TRI_MAX_RINGS (tri_rings_draw_class)
		const uint64_t base0 = sp[0].first_vertex;
		const bool evenOdd = (d.fill_flags & VGX_FILL_EVEN_ODD) != 0u;
		uint32_t route = VGX_TRI_ROUTE_TRIANGLES;

		// the rings by vertex, their links, the non-finite test
		bool bad = false;
		for (uint32_t j = tid; j < V; j += VGX_TRI_THREADS) {
			const uint32_t r = tri_ring_of(sp, S, j);
			const uint32_t first = (uint32_t)(sp[r].first_vertex - base0), n = sp[r].num_vertices, jl = j - first;
			const V2 p = tri_ring_vertex(A.poly + 2 * sp[r].first_vertex, n, d, jl);
			s_pos[j] = make_float2(p.x, p.y);
			s_prev[j] = (uint16_t)(jl ? j - 1 : first + n - 1); s_next[j] = (uint16_t)(jl + 1 < n ? j + 1 : first);
			s_vert[j] = VGX_TRI_UNLINKED;
			bad = bad || !tri_finite(p);
		}
		if (__syncthreads_or(bad ? 1 : 0)) { route = VGX_TRI_REFUSED_NONFINITE; }

		// per ring, a wave each: its smallest and greatest vertex and its orientation
		if (route == VGX_TRI_ROUTE_TRIANGLES) {
			for (uint32_t r = wave; r < S; r += VGX_TRI_THREADS / 64) {
				const uint32_t first = (uint32_t)(sp[r].first_vertex - base0), n = sp[r].num_vertices;
				uint32_t k = VGX_TRI_NONE, g = VGX_TRI_NONE;
				V2 pk = v2(0.0f, 0.0f), pg = pk;
				for (uint32_t j = first + lane; j < first + n; j += 64) {
					const V2 p = lds_pos(s_pos, j);
					if (k == VGX_TRI_NONE || tri_before(p, j, pk, k)) { k = j; pk = p; }
					if (g == VGX_TRI_NONE || tri_before(pg, g, p, j)) { g = j; pg = p; }
				}
				k = wave_extreme_vertex(pk, k, false); g = wave_extreme_vertex(pg, g, true);
				if (lane == 0) {
					s_lo[r] = (uint16_t)k; s_mh[r] = (uint16_t)g;
					s_sgn[r] = (int8_t)tri_sign(tri_edge(lds_pos(s_pos, s_prev[k]), lds_pos(s_pos, k), lds_pos(s_pos, s_next[k])));
				}
			}
			__syncthreads();
			bool flat = false;
			for (uint32_t r = tid; r < S; r += VGX_TRI_THREADS) { flat = flat || s_sgn[r] == 0; }
			if (__syncthreads_or(flat ? 1 : 0)) { route = VGX_TRI_REFUSED_DEGENERATE; }
		}

		if (route == VGX_TRI_ROUTE_TRIANGLES) { // every edge against every later edge of the draw: the j of one i spread over the threads
			bool meet = false;
			for (uint32_t i = 0; i + 1 < V; ++i) {
				const uint32_t ni = s_next[i];
				const V2 u1 = lds_pos(s_pos, i), v1 = lds_pos(s_pos, ni);
				for (uint32_t j = i + 1 + tid; j < V; j += VGX_TRI_THREADS) {
					const uint32_t nj = s_next[j];
					if (ni == j || nj == i) { continue; } // a common vertex index
					meet = meet || tri_edges_meet(u1, v1, lds_pos(s_pos, j), lds_pos(s_pos, nj));
				}
			}
			if (__syncthreads_or(meet ? 1 : 0)) { route = VGX_TRI_REFUSED_NOT_SIMPLE; }
		}

		uint32_t o = 0;
		double s = 0.0;
		if (route == VGX_TRI_ROUTE_TRIANGLES) { // the outer ring; per hole, a wave each: its orientation and inside(m_h, r) of every other ring r
			uint32_t k = s_lo[0]; // every thread folds the same ring minima in the same order (broadcast reads)
			for (uint32_t r = 1; r < S; ++r) {
				const uint32_t j = s_lo[r];
				if (tri_before(lds_pos(s_pos, j), j, lds_pos(s_pos, k), k)) { k = j; }
			}
			o = tri_ring_of(sp, S, k);
			s = (double)s_sgn[o];
			bool wrong = false;
			for (uint32_t h = wave; h < S; h += VGX_TRI_THREADS / 64) {
				if (h == o) { continue; }
				if (!evenOdd && s_sgn[h] != -s_sgn[o]) { wrong = true; }
				const V2 m = lds_pos(s_pos, s_mh[h]);
				for (uint32_t r = 0; r < S && !wrong; ++r) {
					if (r == h) { continue; }
					const uint32_t first = (uint32_t)(sp[r].first_vertex - base0), n = sp[r].num_vertices;
					bool in = false;
					for (uint32_t j = first + lane; j < first + n; j += 64) { in = in != tri_inside_edge(lds_pos(s_pos, j), lds_pos(s_pos, s_next[j]), m); }
					const bool inside = (__popcll(wave_ballot(in)) & 1) != 0;
					if (inside != (r == o)) { wrong = true; }
				}
			}
			if (__syncthreads_or(wrong ? 1 : 0)) { route = VGX_TRI_REFUSED_NESTING; }
		}

		if (route == VGX_TRI_ROUTE_TRIANGLES) { // the holes in descending order of their bridge vertex (s_lo); the merged ring starts as ring o
			for (uint32_t h = tid; h < S; h += VGX_TRI_THREADS) {
				if (h == o) { continue; }
				const uint32_t mine = s_mh[h];
				const V2 pm = lds_pos(s_pos, mine);
				uint32_t rank = 0;
				for (uint32_t g = 0; g < S; ++g) {
					const uint32_t other = s_mh[g];
					if (g != o && g != h && tri_before(pm, mine, lds_pos(s_pos, other), other)) { ++rank; }
				}
				s_lo[rank] = (uint16_t)h;
			}
			const uint32_t first = (uint32_t)(sp[o].first_vertex - base0), n = sp[o].num_vertices;
			for (uint32_t j = first + tid; j < first + n; j += VGX_TRI_THREADS) { s_vert[j] = (uint16_t)j; }
			__syncthreads();
		}

		for (uint32_t jh = 0; jh < H && route == VGX_TRI_ROUTE_TRIANGLES; ++jh) { // one bridge per trip
			const uint32_t h = s_lo[jh], M = s_mh[h], slots = V + 2u * jh;
			const V2 pm = lds_pos(s_pos, M);
			double rejected = -1.0; // the last rejected key; d2 >= 0
			uint32_t rejectedSlot = 0, q = VGX_TRI_NONE;
			for (;;) {
				double best = 0.0;
				uint32_t bestSlot = VGX_TRI_NONE;
				for (uint32_t x = tid; x < slots; x += VGX_TRI_THREADS) {
					const uint32_t vx = s_vert[x];
					if (vx == VGX_TRI_UNLINKED) { continue; }
					const V2 px = lds_pos(s_pos, vx);
					if (!tri_after(px, pm) || !tri_cone(lds_pos(s_pos, s_vert[s_prev[x]]), px, lds_pos(s_pos, s_vert[s_next[x]]), pm, s)) { continue; }
					const double dd = tri_d2(pm, px);
					if (!tri_key_less(rejected, rejectedSlot, dd, x)) { continue; }
					if (bestSlot == VGX_TRI_NONE || tri_key_less(dd, x, best, bestSlot)) { best = dd; bestSlot = x; }
				}
				block_min_key(&best, &bestSlot, s_rd, s_rs);
				if (bestSlot == VGX_TRI_NONE) { break; }
				const uint32_t vq = s_vert[bestSlot];
				const V2 pq = lds_pos(s_pos, vq);
				bool hidden = false; // every ring's edges and the earlier bridges are the links of the slots so far
				for (uint32_t x = tid; x < slots; x += VGX_TRI_THREADS) {
					const uint32_t y = s_next[x];
					const uint32_t u = x < V ? x : s_vert[x], w = y < V ? y : s_vert[y];
					if (u == M || w == M || u == vq || w == vq) { continue; }
					hidden = hidden || tri_edges_meet(pm, pq, lds_pos(s_pos, u), lds_pos(s_pos, w));
				}
				if (!__syncthreads_or(hidden ? 1 : 0)) { q = bestSlot; break; }
				rejected = best; rejectedSlot = bestSlot;
			}
			if (q == VGX_TRI_NONE) { route = VGX_TRI_REFUSED_NO_BRIDGE; break; }
			const uint32_t first = (uint32_t)(sp[h].first_vertex - base0), n = sp[h].num_vertices;
			const bool backwards = s_sgn[h] == s_sgn[o];
			for (uint32_t j = first + tid; j < first + n; j += VGX_TRI_THREADS) {
				if (backwards) { const uint16_t t = s_prev[j]; s_prev[j] = s_next[j]; s_next[j] = t; }
				s_vert[j] = (uint16_t)j;
			}
			__syncthreads();
			if (tid == 0) { // q -> M -> the hole -> second copy of M -> second copy of q -> old next q
				const uint32_t a = slots, b = slots + 1u, qn = s_next[q], last = s_prev[M];
				s_vert[a] = (uint16_t)M; s_vert[b] = s_vert[q];
				s_next[q] = (uint16_t)M; s_prev[M] = (uint16_t)q;
				s_next[last] = (uint16_t)a; s_prev[a] = (uint16_t)last;
				s_next[a] = (uint16_t)b; s_prev[b] = (uint16_t)a;
				s_next[b] = (uint16_t)qn; s_prev[qn] = (uint16_t)b;
			}
			__syncthreads();
		}

		if (tid < 64) { // one wave, every lane with the same cursor, over the N slots
			const uint64_t first = 3 * A.cand_prefix[di];
			const bool keep = first + 3 * (uint64_t)N <= A.cap_tri; // beyond it the call ends with VGX_E_NOSPACE: the route is still needed
			uint16_t* tri = A.tri + first;
			if (route == VGX_TRI_ROUTE_TRIANGLES) {
				uint32_t b = 0, size = N, misses = 0, nt = 0;
				while (size > 3) {
					const uint32_t a = s_prev[b], c = s_next[b];
					const uint32_t va = s_vert[a], vb = s_vert[b], vc = s_vert[c];
					const V2 pa = lds_pos(s_pos, va), pb = lds_pos(s_pos, vb), pc = lds_pos(s_pos, vc);
					const double t = s * tri_edge(pa, pb, pc);
					bool ear = t == 0.0;
					if (t > 0.0) {
						ear = true;
						for (uint32_t base = 0; base < N && ear; base += 64) {
							const uint32_t p = base + lane;
							bool inside = false;
							if (p < N && p != a && p != b && p != c && s_prev[p] != VGX_TRI_UNLINKED) { inside = tri_blocks_slot(pa, pb, pc, lds_pos(s_pos, s_vert[p]), s); }
							ear = wave_ballot(inside) == 0ull;
						}
					}
					if (ear) {
						if (lane == 0 && keep) { tri[nt] = (uint16_t)va; tri[nt + 1] = (uint16_t)vb; tri[nt + 2] = (uint16_t)vc; }
						nt += 3;
						s_next[a] = (uint16_t)c; s_prev[c] = (uint16_t)a; s_prev[b] = VGX_TRI_UNLINKED;
						b = s_next[c]; --size; misses = 0;
					} else {
						b = c;
						if (++misses > size) { route = VGX_TRI_REFUSED_STALLED; break; }
					}
				}
				if (route == VGX_TRI_ROUTE_TRIANGLES && lane == 0 && keep) { tri[nt] = s_vert[s_prev[b]]; tri[nt + 1] = s_vert[b]; tri[nt + 2] = s_vert[s_next[b]]; }
			}
			if (lane == 0) {
				A.route[di] = route;
				if (A.draw_route) { A.draw_route[di] = route; }
			}
		}
	}
}

// k_tri_emit for the rings entry: a triangulated draw holds all its sub-paths' vertices and 3 (V + 2 H - 2) triangle indices
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_emit_rings(VgxTriArgs A)
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
			const uint64_t ni = 3 * (V + 2ull * (info.num_subpaths - 1u) - 2);
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) { (void)contours_emit_vertex_data(A.poly, sp, info.num_subpaths, d, c, V, fv, fi, A.pos, A.color, A.idx); }
			for (uint64_t k = threadIdx.x; k < ni; k += VGX_TRI_THREADS) { tri_emit_index(d, tri, k, V, fi, A.idx); }
		} else {
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) {
				contours_emit_vertex(A.poly, sp, info.num_subpaths, d, c, V, fv, fi, A.pos, A.color, A.idx);
			}
		}
	}
}

// ---- vgx_concave_triangulate_nested: the same four steps for draws of several outlines and islands in holes ---------------------------
// Scan 1 is the rings entry's (V + 2 (S - 1) slots of triangle scratch per deciding draw bound any grouping). A triangulated draw has
// 3 (V + 2 S - 4 G) indices, so k_tri_decide_nested leaves G per draw in `groups` for scan 2 and the emit kernel. The kernels above are
// not launched by this entry and not touched by it.
struct OpTriNestedPlaces : OpTriPlaces // scan 2
{
	const uint32_t* groups;
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t route = A.route[i];
		if (route == 0u) { return r; }
		uint32_t nm; bool big;
		tri_nested_draw_sizes(A.draws[i], route, A.ring_vertices[i], A.draw_info[i].num_subpaths, groups[i], &r.a, &r.b, &nm, &big);
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
		const uint32_t n = tri_nested_draw_meshes(A.draws[i], (uint32_t)i, route, A.ring_vertices[i], A.draw_info[i].num_subpaths, groups[i], e.a, e.b, m);
		for (uint32_t k = 0; k < n; ++k) { if (e.c + k < A.cap_meshes) { A.meshes[e.c + k] = m[k]; } }
	}
};

// v, which every lane of the wave holds alike, as a value the compiler knows to be uniform
__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// does slot p (still linked, not a, b or c) keep (a, b, c) from being an ear of its group? amend: the group has holes
__device__ __forceinline__ bool nested_slot_blocks(const float2* s_pos, const uint16_t* s_vert, const uint16_t* s_prev, uint32_t p, uint32_t a, uint32_t b, uint32_t c,
                                                   V2 pa, V2 pb, V2 pc, double s, bool amend)
{
	if (p == a || p == b || p == c || s_prev[p] == VGX_TRI_UNLINKED) { return false; }
	const V2 pp = lds_pos(s_pos, s_vert[p]);
	return amend ? tri_blocks_slot(pa, pb, pc, pp, s) : tri_blocks(pa, pb, pc, pp, s);
}

// One workgroup per deciding draw. LDS by the compiler's report: k_tri_decide_rings' tables, a 16-bit ring per
// vertex and five more 16-bit tables per ring -- below 80 KiB, so two workgroups per CU as there. The tables per ring r: s_first (its
// first vertex; [S] = V), s_mh, s_sgn, s_depth, s_out (the outer ring of its group); per outer ring o: s_H (its holes), s_B (the holes of
// the groups before it), s_T (the triangles of the groups before it); s_lo[s_B[o] + j] = the j-th processed hole of group o.
// `route` and `limit` are block-uniform throughout: every change comes out of a barrier.
// Classification is one THREAD per ring r (a thread takes ceil(S / 256) rings): inside(m_r, r') over every other ring in turn, twice
// (depth, then parent), behind the y-range pre-test that is exact by the definition of inside. Without the pre-test a thread would walk
// up to ceil(S / 256) * V edges per pass, as much as the edge-pair test above it at 819 rings; with it only the rings whose y-range holds
// m_r.y are walked. With many small rings (text) every thread is busy; with few long rings few threads are, for at most V edges each.
// Clipping: wave w clips the groups whose outer ring is w, w + 4, .. (a static assignment: no counter, no atomic). A group's slots,
// links and triangles belong to it alone and its triangles have their place (s_T) in advance, so no barrier is needed inside the phase.
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_decide_nested(VgxTriArgs A, uint32_t* groups)
{
	__shared__ float2 s_pos[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint16_t s_vert[VGX_TRIANGULATE_MAX_VERTICES], s_prev[VGX_TRIANGULATE_MAX_VERTICES], s_next[VGX_TRIANGULATE_MAX_VERTICES], s_ring[VGX_TRIANGULATE_MAX_VERTICES];
	__shared__ uint16_t s_first[VGX_TRI_MAX_RINGS + 1], s_mh[VGX_TRI_MAX_RINGS], s_lo[VGX_TRI_MAX_RINGS], s_depth[VGX_TRI_MAX_RINGS], s_out[VGX_TRI_MAX_RINGS];
	__shared__ uint16_t s_H[VGX_TRI_MAX_RINGS], s_B[VGX_TRI_MAX_RINGS], s_T[VGX_TRI_MAX_RINGS];
	__shared__ int8_t s_sgn[VGX_TRI_MAX_RINGS];
	__shared__ double s_rd[VGX_TRI_THREADS / 64];
	__shared__ uint32_t s_rs[VGX_TRI_THREADS / 64];
	__shared__ uint32_t s_stalled, s_groups; // did a group stall; G
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	for (uint64_t di = blockIdx.x; di < A.ndraws; di += gridDim.x) {
		if (A.route[di] != VGX_TRI_ROUTE_TRIANGLES) { continue; } // block-uniform
		__syncthreads(); // the previous draw's readers are done
		const vgx_draw d = A.draws[di];
		const vgx_draw_info info = A.draw_info[di];
		const vgx_subpath* sp = A.subpaths + info.first_subpath;
		const uint32_t S = info.num_subpaths;
		const uint32_t V = (uint32_t)A.ring_vertices[di], N = V + 2u * (S - 1u); // N <= VGX_TRIANGULATE_MAX_VERTICES, S <= VGX_TRI_MAX_RINGS (tri_rings_draw_class)
		const uint64_t base0 = sp[0].first_vertex;
		const bool evenOdd = (d.fill_flags & VGX_FILL_EVEN_ODD) != 0u;
		uint32_t route = VGX_TRI_ROUTE_TRIANGLES;

		// the rings by vertex, their links, the non-finite test
		bool bad = false;
		for (uint32_t j = tid; j < V; j += VGX_TRI_THREADS) {
			const uint32_t r = tri_ring_of(sp, S, j);
			const uint32_t first = (uint32_t)(sp[r].first_vertex - base0), n = sp[r].num_vertices, jl = j - first;
			const V2 p = tri_ring_vertex(A.poly + 2 * sp[r].first_vertex, n, d, jl);
			s_pos[j] = make_float2(p.x, p.y);
			s_prev[j] = (uint16_t)(jl ? j - 1 : first + n - 1); s_next[j] = (uint16_t)(jl + 1 < n ? j + 1 : first);
			s_vert[j] = VGX_TRI_UNLINKED; s_ring[j] = (uint16_t)r;
			bad = bad || !tri_finite(p);
		}
		for (uint32_t r = tid; r <= S; r += VGX_TRI_THREADS) { s_first[r] = (uint16_t)(r < S ? (uint32_t)(sp[r].first_vertex - base0) : V); }
		if (tid == 0) { s_stalled = 0u; s_groups = 0u; }
		if (__syncthreads_or(bad ? 1 : 0)) { route = VGX_TRI_REFUSED_NONFINITE; }

		// per ring, a wave each: its greatest vertex and its orientation
		if (route == VGX_TRI_ROUTE_TRIANGLES) {
			for (uint32_t r = wave; r < S; r += VGX_TRI_THREADS / 64) {
				const uint32_t first = s_first[r], end = s_first[r + 1];
				uint32_t k = VGX_TRI_NONE, g = VGX_TRI_NONE;
				V2 pk = v2(0.0f, 0.0f), pg = pk;
				for (uint32_t j = first + lane; j < end; j += 64) {
					const V2 p = lds_pos(s_pos, j);
					if (k == VGX_TRI_NONE || tri_before(p, j, pk, k)) { k = j; pk = p; }
					if (g == VGX_TRI_NONE || tri_before(pg, g, p, j)) { g = j; pg = p; }
				}
				k = wave_extreme_vertex(pk, k, false); g = wave_extreme_vertex(pg, g, true);
				if (lane == 0) {
					s_mh[r] = (uint16_t)g;
					s_sgn[r] = (int8_t)tri_sign(tri_edge(lds_pos(s_pos, s_prev[k]), lds_pos(s_pos, k), lds_pos(s_pos, s_next[k])));
				}
			}
			__syncthreads();
			bool flat = false;
			for (uint32_t r = tid; r < S; r += VGX_TRI_THREADS) { flat = flat || s_sgn[r] == 0; }
			if (__syncthreads_or(flat ? 1 : 0)) { route = VGX_TRI_REFUSED_DEGENERATE; }
		}

		if (route == VGX_TRI_ROUTE_TRIANGLES) { // every edge against every later edge of the draw: the j of one i spread over the threads
			bool meet = false;
			for (uint32_t i = 0; i + 1 < V; ++i) {
				const uint32_t ni = s_next[i];
				const V2 u1 = lds_pos(s_pos, i), v1 = lds_pos(s_pos, ni);
				for (uint32_t j = i + 1 + tid; j < V; j += VGX_TRI_THREADS) {
					const uint32_t nj = s_next[j];
					if (ni == j || nj == i) { continue; } // a common vertex index
					meet = meet || tri_edges_meet(u1, v1, lds_pos(s_pos, j), lds_pos(s_pos, nj));
				}
			}
			if (__syncthreads_or(meet ? 1 : 0)) { route = VGX_TRI_REFUSED_NOT_SIMPLE; }
		}

		if (route == VGX_TRI_ROUTE_TRIANGLES) { // depth(r) = the rings m_r is inside of
			// The pre-test: per ring the vertices of its least and its greatest y (in s_B and s_T, which nothing uses before the groups
			// are counted). An edge u -> v counts for inside(p, .) only when (u.y <= p.y) != (v.y <= p.y). With p.y < the ring's least y
			// both sides are false for every edge, with p.y >= its greatest y both are true: no edge counts, inside is false, and the
			// ring need not be walked. Exact by the definition, so it changes no answer
			for (uint32_t r = tid; r < S; r += VGX_TRI_THREADS) {
				uint32_t lo = s_first[r], hi = lo;
				for (uint32_t j = lo + 1u, e = s_first[r + 1]; j < e; ++j) {
					const float y = s_pos[j].y;
					if (y < s_pos[lo].y) { lo = j; }
					if (y > s_pos[hi].y) { hi = j; }
				}
				s_B[r] = (uint16_t)lo; s_T[r] = (uint16_t)hi;
			}
			__syncthreads();
			for (uint32_t r = tid; r < S; r += VGX_TRI_THREADS) {
				const V2 m = lds_pos(s_pos, s_mh[r]);
				uint32_t n = 0;
				for (uint32_t q = 0; q < S; ++q) {
					if (q == r || m.y < s_pos[s_B[q]].y || m.y >= s_pos[s_T[q]].y) { continue; }
					bool in = false;
					for (uint32_t j = s_first[q], e = s_first[q + 1]; j < e; ++j) { in = in != tri_inside_edge(lds_pos(s_pos, j), lds_pos(s_pos, s_next[j]), m); }
					n += in ? 1u : 0u;
				}
				s_depth[r] = (uint16_t)n;
			}
			__syncthreads();
			bool wrong = false; // the parent: the one ring of depth - 1 that m_r is inside of; only rings of that depth are walked again
			for (uint32_t r = tid; r < S; r += VGX_TRI_THREADS) {
				const V2 m = lds_pos(s_pos, s_mh[r]);
				const uint32_t depth = s_depth[r];
				uint32_t parents = 0, parent = r;
				for (uint32_t q = 0; q < S && depth > 0u; ++q) {
					if (q == r || s_depth[q] + 1u != depth || m.y < s_pos[s_B[q]].y || m.y >= s_pos[s_T[q]].y) { continue; }
					bool in = false;
					for (uint32_t j = s_first[q], e = s_first[q + 1]; j < e; ++j) { in = in != tri_inside_edge(lds_pos(s_pos, j), lds_pos(s_pos, s_next[j]), m); }
					if (in) { ++parents; parent = q; }
				}
				const bool hole = tri_nested_is_hole(depth);
				if (depth > 0u && parents != 1u) { wrong = true; }
				if (hole && !tri_nested_hole_fits(s_sgn[r], s_sgn[parent], evenOdd)) { wrong = true; }
				s_out[r] = (uint16_t)(hole ? parent : r);
			}
			if (__syncthreads_or(wrong ? 1 : 0)) { route = VGX_TRI_REFUSED_NESTING; }
		}

		uint32_t limit = S; // the first group that finds no bridge: the groups from it on decide nothing any more
		if (route == VGX_TRI_ROUTE_TRIANGLES) {
			// per outer ring its holes and its triangles, then the exclusive prefixes in ring order (at most 819 entries: one thread)
			for (uint32_t o = tid; o < S; o += VGX_TRI_THREADS) {
				uint32_t Hg = 0, Vg = 0;
				if (s_out[o] == o) {
					for (uint32_t r = 0; r < S; ++r) { if (s_out[r] == o) { Vg += (uint32_t)s_first[r + 1] - s_first[r]; Hg += r != o ? 1u : 0u; } }
				}
				s_H[o] = (uint16_t)Hg; s_T[o] = (uint16_t)(Vg ? tri_nested_group_triangles(Vg, Hg) : 0u);
			}
			__syncthreads();
			if (tid == 0) {
				uint32_t G = 0, B = 0, T = 0;
				for (uint32_t o = 0; o < S; ++o) {
					if (s_out[o] != o) { continue; }
					const uint32_t t = s_T[o];
					s_B[o] = (uint16_t)B; s_T[o] = (uint16_t)T;
					++G; B += s_H[o]; T += t;
				}
				s_groups = G;
			}
			__syncthreads();
			// a group's holes in descending order of their bridge vertex (s_lo); every outer ring is a merged ring to start with
			for (uint32_t h = tid; h < S; h += VGX_TRI_THREADS) {
				const uint32_t o = s_out[h];
				if (o == h) { continue; }
				const uint32_t mine = s_mh[h];
				const V2 pm = lds_pos(s_pos, mine);
				uint32_t rank = 0;
				for (uint32_t g = 0; g < S; ++g) {
					const uint32_t other = s_mh[g];
					if (g != o && g != h && s_out[g] == o && tri_before(pm, mine, lds_pos(s_pos, other), other)) { ++rank; }
				}
				s_lo[s_B[o] + rank] = (uint16_t)h;
			}
			for (uint32_t j = tid; j < V; j += VGX_TRI_THREADS) {
				const uint32_t r = s_ring[j];
				if (s_out[r] == r) { s_vert[j] = (uint16_t)j; }
			}
			__syncthreads();

			// bridges: group after group by the block-wide search, over the group's slots alone
			for (uint32_t o = 0; o < S && limit == S; ++o) {
				if (s_out[o] != o) { continue; }
				const uint32_t Hg = s_H[o], slot0 = V + 2u * s_B[o];
				const double s = (double)s_sgn[o];
				for (uint32_t jh = 0; jh < Hg; ++jh) { // one bridge per trip
					const uint32_t h = s_lo[s_B[o] + jh], M = s_mh[h], slots = V + 2u * jh; // its vertex slots among the V, then its bridge slots from slot0
					const V2 pm = lds_pos(s_pos, M);
					double rejected = -1.0; // the last rejected key; d2 >= 0
					uint32_t rejectedSlot = 0, q = VGX_TRI_NONE;
					for (;;) {
						double best = 0.0;
						uint32_t bestSlot = VGX_TRI_NONE;
						for (uint32_t i = tid; i < slots; i += VGX_TRI_THREADS) {
							const uint32_t x = i < V ? i : i - V + slot0;
							const uint32_t vx = s_vert[x];
							if (vx == VGX_TRI_UNLINKED || (x < V && s_out[s_ring[x]] != o)) { continue; }
							const V2 px = lds_pos(s_pos, vx);
							if (!tri_after(px, pm) || !tri_cone(lds_pos(s_pos, s_vert[s_prev[x]]), px, lds_pos(s_pos, s_vert[s_next[x]]), pm, s)) { continue; }
							const double dd = tri_d2(pm, px);
							if (!tri_key_less(rejected, rejectedSlot, dd, x)) { continue; }
							if (bestSlot == VGX_TRI_NONE || tri_key_less(dd, x, best, bestSlot)) { best = dd; bestSlot = x; }
						}
						block_min_key(&best, &bestSlot, s_rd, s_rs);
						if (bestSlot == VGX_TRI_NONE) { break; }
						const uint32_t vq = s_vert[bestSlot];
						const V2 pq = lds_pos(s_pos, vq);
						bool hidden = false; // the group's rings' edges and its earlier bridges are the links of its slots so far
						for (uint32_t i = tid; i < slots; i += VGX_TRI_THREADS) {
							const uint32_t x = i < V ? i : i - V + slot0;
							if (x < V && s_out[s_ring[x]] != o) { continue; }
							const uint32_t y = s_next[x];
							const uint32_t u = x < V ? x : s_vert[x], w = y < V ? y : s_vert[y];
							if (u == M || w == M || u == vq || w == vq) { continue; }
							hidden = hidden || tri_edges_meet(pm, pq, lds_pos(s_pos, u), lds_pos(s_pos, w));
						}
						if (!__syncthreads_or(hidden ? 1 : 0)) { q = bestSlot; break; }
						rejected = best; rejectedSlot = bestSlot;
					}
					if (q == VGX_TRI_NONE) { limit = o; break; }
					const uint32_t first = s_first[h], end = s_first[h + 1];
					const bool backwards = s_sgn[h] == s_sgn[o];
					for (uint32_t j = first + tid; j < end; j += VGX_TRI_THREADS) {
						if (backwards) { const uint16_t t = s_prev[j]; s_prev[j] = s_next[j]; s_next[j] = t; }
						s_vert[j] = (uint16_t)j;
					}
					__syncthreads();
					if (tid == 0) { // q -> M -> the hole -> second copy of M -> second copy of q -> old next q
						const uint32_t a = slot0 + 2u * jh, b = a + 1u, qn = s_next[q], last = s_prev[M];
						s_vert[a] = (uint16_t)M; s_vert[b] = s_vert[q];
						s_next[q] = (uint16_t)M; s_prev[M] = (uint16_t)q;
						s_next[last] = (uint16_t)a; s_prev[a] = (uint16_t)last;
						s_next[a] = (uint16_t)b; s_prev[b] = (uint16_t)a;
						s_next[b] = (uint16_t)qn; s_prev[qn] = (uint16_t)b;
					}
					__syncthreads();
				}
			}

			// clipping: every wave clips whole groups below `limit`, wave w the outer rings o = w, w + 4, ..; every lane with the same
			// cursor; a link is stored by all lanes alike. Everything that steers a loop here is made wave-uniform FOR THE COMPILER
			// (readfirstlane, ballot): left as values loaded per lane, the loops are built as lane-divergent ones, and the ballots
			// inside them must never run with a part of the wave
			const uint64_t first = 3 * A.cand_prefix[di];
			const bool keep = first + 3 * (uint64_t)N <= A.cap_tri; // beyond it the call ends with VGX_E_NOSPACE: the route is still needed
			for (uint32_t o = wave_uniform(wave); o < limit; o += VGX_TRI_THREADS / 64) {
				if (wave_uniform(s_out[o]) == o) {
					const uint32_t Hg = wave_uniform(s_H[o]), B = wave_uniform(s_B[o]), bridge0 = V + 2u * B, bridge1 = bridge0 + 2u * Hg;
					const double s = (double)s_sgn[o];
					const bool amend = Hg != 0u; // a group of one ring: vgx_concave_triangulate's loop
					uint32_t b = s_first[o], size = (uint32_t)s_first[o + 1] - s_first[o];
					for (uint32_t j = 0; j < Hg; ++j) { // the group's slots and the lowest of them (broadcast reads)
						const uint32_t h = s_lo[B + j], f = s_first[h];
						size += (uint32_t)s_first[h + 1] - f + 2u;
						b = f < b ? f : b;
					}
					size = wave_uniform(size);
					const bool wide = Hg + 1u > (V + 63u) / 64u; // more rings than the draw has 64-vertex strides: walk those and filter by group
					uint16_t* tri = A.tri + first + 3u * s_T[o];
					uint32_t misses = 0, nt = 0;
					bool stalled = false;
					while (size > 3 && !stalled) {
						const uint32_t a = s_prev[b], c = s_next[b];
						const uint32_t va = s_vert[a], vb = s_vert[b], vc = s_vert[c];
						const V2 pa = lds_pos(s_pos, va), pb = lds_pos(s_pos, vb), pc = lds_pos(s_pos, vc);
						const double t = s * tri_edge(pa, pb, pc);
						bool ear = wave_ballot(t == 0.0) != 0ull; // every lane holds the same t
						if (wave_ballot(t > 0.0) != 0ull) {
							ear = true;
							if (wide) {
								for (uint32_t base = 0; base < V && ear; base += 64) {
									const uint32_t p = base + lane;
									const bool inside = p < V && s_out[s_ring[p]] == o && nested_slot_blocks(s_pos, s_vert, s_prev, p, a, b, c, pa, pb, pc, s, amend);
									ear = wave_ballot(inside) == 0ull;
								}
							} else {
								for (uint32_t k = 0; k <= Hg && ear; ++k) { // the group's ring ranges
									const uint32_t r = k ? wave_uniform(s_lo[B + k - 1u]) : o, end = wave_uniform(s_first[r + 1]);
									for (uint32_t base = wave_uniform(s_first[r]); base < end && ear; base += 64) {
										const uint32_t p = base + lane;
										const bool inside = p < end && nested_slot_blocks(s_pos, s_vert, s_prev, p, a, b, c, pa, pb, pc, s, amend);
										ear = wave_ballot(inside) == 0ull;
									}
								}
							}
							for (uint32_t base = bridge0; base < bridge1 && ear; base += 64) { // and its bridge slots
								const uint32_t p = base + lane;
								const bool inside = p < bridge1 && nested_slot_blocks(s_pos, s_vert, s_prev, p, a, b, c, pa, pb, pc, s, amend);
								ear = wave_ballot(inside) == 0ull;
							}
						}
						if (ear) {
							if (lane == 0 && keep) { tri[nt] = (uint16_t)va; tri[nt + 1] = (uint16_t)vb; tri[nt + 2] = (uint16_t)vc; }
							nt += 3;
							s_next[a] = (uint16_t)c; s_prev[c] = (uint16_t)a; s_prev[b] = VGX_TRI_UNLINKED;
							b = s_next[c]; --size; misses = 0;
						} else {
							b = c;
							stalled = ++misses > size;
						}
					}
					if (stalled) {
						s_stalled = 1u; // by every lane alike
					} else if (lane == 0 && keep) {
						tri[nt] = s_vert[s_prev[b]]; tri[nt + 1] = s_vert[b]; tri[nt + 2] = s_vert[s_next[b]];
					}
				}
			}
			__syncthreads();
			if (s_stalled) { route = VGX_TRI_REFUSED_STALLED; } else if (limit != S) { route = VGX_TRI_REFUSED_NO_BRIDGE; }
		}

		if (tid == 0) {
			A.route[di] = route;
			groups[di] = route == VGX_TRI_ROUTE_TRIANGLES ? s_groups : 0u;
			if (A.draw_route) { A.draw_route[di] = route; }
		}
	}
}

// k_tri_emit for the nested entry: a triangulated draw holds all its sub-paths' vertices and 3 (V + 2 S - 4 G) triangle indices
__global__ __launch_bounds__(VGX_TRI_THREADS) void k_tri_emit_nested(VgxTriArgs A, const uint32_t* groups)
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
			const uint64_t ni = 3 * (V + 2ull * info.num_subpaths - 4ull * groups[di]);
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) { (void)contours_emit_vertex_data(A.poly, sp, info.num_subpaths, d, c, V, fv, fi, A.pos, A.color, A.idx); }
			for (uint64_t k = threadIdx.x; k < ni; k += VGX_TRI_THREADS) { tri_emit_index(d, tri, k, V, fi, A.idx); }
		} else {
			for (uint64_t c = threadIdx.x; c < V; c += VGX_TRI_THREADS) {
				contours_emit_vertex(A.poly, sp, info.num_subpaths, d, c, V, fv, fi, A.pos, A.color, A.idx);
			}
		}
	}
}

} // namespace

void vgx_launch_concave_triangulate_nested(const VgxTriArgs& a, uint32_t* groups, void* partial, hipStream_t s)
{
	OpTriRingsClasses classes; classes.A = a;
	vgx_device_scan(classes, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_decide_nested, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a, groups);
	}
	OpTriNestedPlaces places; places.A = a; places.groups = groups;
	vgx_device_scan(places, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_emit_nested, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a, (const uint32_t*)groups);
	}
}

void vgx_launch_concave_triangulate_rings(const VgxTriArgs& a, void* partial, hipStream_t s)
{
	OpTriRingsClasses classes; classes.A = a;
	vgx_device_scan(classes, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_decide_rings, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a);
	}
	OpTriRingsPlaces places; places.A = a;
	vgx_device_scan(places, (Sum3*)partial, s, a.ndraws);
	if (a.ndraws) {
		const uint32_t blocks = (uint32_t)(a.ndraws < 4096u ? a.ndraws : 4096u);
		hipLaunchKernelGGL(k_tri_emit_rings, dim3(blocks), dim3(VGX_TRI_THREADS), 0, s, a);
	}
}

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
