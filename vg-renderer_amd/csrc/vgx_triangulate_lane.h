// vgx_triangulate_lane.h -- the arithmetic of vgx_concave_triangulate (include/vgx.h) for ONE ring: host + device. The predicates below
// are what a lane of vgx_triangulate.hip evaluates; tri_ring_route runs the rule vertex after vertex on the host (libvgx_hosttest.so:
// vgxt_concave_triangulate), so that the CPU suite pins every route and every index without a GPU. What a refused draw holds is
// vgx_concave_lane.h's, called from both sides. Below them, the same for vgx_concave_triangulate_rings -- one outer ring with holes:
// nesting, cone, bridge distance, the clipping amendment -- and its host walk tri_rings_route (vgxt_concave_triangulate_rings). Last,
// vgx_concave_triangulate_nested -- several outlines, islands in holes: groups by containment depth -- and tri_nested_route.
//
// Every decision is a sign of the canonical edge value of vgx_raster.h -- the rasteriser's own function, not a restatement of it --, so
// "the triangles' windings sum to the ring's" is a statement about one number computed in one place.
#ifndef VGX_TRIANGULATE_LANE_H
#define VGX_TRIANGULATE_LANE_H

#include "vgx_concave_lane.h"
#include "vgx_raster.h"

#define VGX_TRI_UNLINKED 0xFFFFu // prev[] of a clipped vertex; VGX_TRIANGULATE_MAX_VERTICES stays below it
static_assert(VGX_TRIANGULATE_MAX_VERTICES < VGX_TRI_UNLINKED, "ring links are 16 bits wide");

// c(a, b, p) of the header
VGX_HD double tri_edge(V2 a, V2 b, V2 p)
{
	VgxRasterEdge e;
	const uint32_t f = vgx_raster_edge(a, b, true, 0, &e);
	return vgx_raster_edge_value(e, f, 0, (double)p.x, (double)p.y);
}

VGX_HD bool tri_finite(V2 p)
{
	union { float f; uint32_t u; } x, y;
	x.f = p.x; y.f = p.y;
	return (x.u & 0x7F800000u) != 0x7F800000u && (y.u & 0x7F800000u) != 0x7F800000u;
}

// vertex j of the ring of a single-sub-path draw: the polyline vertex, with AA the vertex vgx_concave_move gives
VGX_HD V2 tri_ring_vertex(const float* v, uint32_t n, const vgx_draw& d, uint32_t j)
{
	return (d.fill_flags & VGX_FILL_AA) ? contour_vertex(v, n, j, d.fringe).in : ldc(v, j);
}

// What can be said of draw d without its geometry: 0 (no mesh), MULTI, TOO_LONG, or VGX_TRI_ROUTE_TRIANGLES = "the ring decides".
// *made = contours_draw_counts' return, *V its vertex count
VGX_HD uint32_t tri_draw_class(const vgx_draw& d, const vgx_draw_info& di, const vgx_subpath* subs, uint64_t* V, int* made)
{
	*made = contours_draw_counts(d, di, subs, V);
	if (*made <= 0) { return 0u; }
	if (di.num_subpaths > 1u) { return VGX_TRI_REFUSED_MULTI; }
	if (*V > VGX_TRIANGULATE_MAX_VERTICES) { return VGX_TRI_REFUSED_TOO_LONG; }
	return VGX_TRI_ROUTE_TRIANGLES;
}

// (x, y, index) order of the orientation's vertex k
VGX_HD bool tri_before(V2 p, uint32_t i, V2 q, uint32_t j)
{
	return p.x < q.x || (p.x == q.x && (p.y < q.y || (p.y == q.y && i < j)));
}

VGX_HD int tri_sign(double e) { return e > 0.0 ? 1 : (e < 0.0 ? -1 : 0); }

VGX_HD bool tri_in_box(V2 p, V2 a, V2 b)
{
	const float x0 = a.x < b.x ? a.x : b.x, x1 = a.x < b.x ? b.x : a.x, y0 = a.y < b.y ? a.y : b.y, y1 = a.y < b.y ? b.y : a.y;
	return p.x >= x0 && p.x <= x1 && p.y >= y0 && p.y <= y1;
}

// do the edges u1 -> v1 and u2 -> v2 (no vertex index in common) meet?
VGX_HD bool tri_edges_meet(V2 u1, V2 v1, V2 u2, V2 v2)
{
	const int a = tri_sign(tri_edge(u1, v1, u2)), b = tri_sign(tri_edge(u1, v1, v2));
	const int c = tri_sign(tri_edge(u2, v2, u1)), d = tri_sign(tri_edge(u2, v2, v1));
	if (a * b < 0 && c * d < 0) { return true; }
	return (a == 0 && tri_in_box(u2, u1, v1)) || (b == 0 && tri_in_box(v2, u1, v1)) || (c == 0 && tri_in_box(u1, u2, v2)) || (d == 0 && tri_in_box(v1, u2, v2));
}

// does p keep (a, b, c) from being an ear of a ring of orientation s?
VGX_HD bool tri_blocks(V2 a, V2 b, V2 c, V2 p, double s)
{
	return s * tri_edge(a, b, p) >= 0.0 && s * tri_edge(b, c, p) >= 0.0 && s * tri_edge(c, a, p) >= 0.0;
}

// mesh record(s) of a draw of V ring vertices under `route`, first mesh at (firstVertex, firstIndex); the sizes it adds. A refused
// draw: contours_draw_meshes'
VGX_HD void tri_draw_sizes(const vgx_draw& d, uint32_t route, uint64_t V, uint64_t* nv, uint64_t* ni, uint32_t* nm, bool* tooLarge)
{
	const bool aa = (d.fill_flags & VGX_FILL_AA) != 0u;
	if (route == VGX_TRI_ROUTE_TRIANGLES) {
		*nv = aa ? 3 * V : V; *ni = (aa ? 6 * V : 0u) + 3 * (V - 2); *nm = 1u;
		*tooLarge = *nv > 65536u;
	} else {
		*nv = aa ? 3 * V : V; *ni = aa ? 8 * V : 2 * V; *nm = aa ? 2u : 1u;
		*tooLarge = (aa ? 2 * V : V) > 65536u; // vgx_concave_contours' rule: per mesh
	}
}

VGX_HD uint32_t tri_draw_meshes(const vgx_draw& d, uint32_t drawIndex, uint32_t route, uint64_t V, uint64_t firstVertex, uint64_t firstIndex, vgx_mesh* m)
{
	if (route != VGX_TRI_ROUTE_TRIANGLES) { return contours_draw_meshes(d, drawIndex, V, firstVertex, firstIndex, m); }
	uint64_t nv, ni; uint32_t nm; bool big;
	tri_draw_sizes(d, route, V, &nv, &ni, &nm, &big);
	m[0].first_vertex = firstVertex; m[0].first_index = firstIndex; m[0].num_vertices = (uint32_t)nv; m[0].num_indices = (uint32_t)ni;
	m[0].draw = drawIndex; m[0].subpath_kind = (uint32_t)VGX_MESH_CONCAVE_FILL_AA << 28;
	return 1u;
}

// Vertex c of a triangulated draw: its vertex (with AA: its fringe pair, the segment's six indices and the moved vertex behind the fringe)
VGX_HD void tri_emit_vertex(const float* poly, const vgx_subpath* sp, const vgx_draw& d, uint64_t c, uint64_t V, uint64_t firstVertex, uint64_t firstIndex,
                            float* pos, uint32_t* color, uint16_t* idx)
{
	(void)contours_emit_vertex_data(poly, sp, 1u, d, c, V, firstVertex, firstIndex, pos, color, idx);
}

// Index k (< 3 (V - 2)) of a triangulated draw from the clipping's ring-local triangles
VGX_HD void tri_emit_index(const vgx_draw& d, const uint16_t* tri, uint64_t k, uint64_t V, uint64_t firstIndex, uint16_t* idx)
{
	const bool aa = (d.fill_flags & VGX_FILL_AA) != 0u;
	idx[firstIndex + (aa ? 6 * V : 0u) + k] = (uint16_t)(tri[k] + (aa ? 2 * V : 0u));
}

// ---- vgx_concave_triangulate_rings: one outer ring with holes, bridged into one ring of SLOTS (include/vgx.h) ---------------------------
// A draw of S sub-paths has V vertices (numbered in sub-path order), H = S - 1 holes and N = V + 2 H slots. Slot i < V is vertex i;
// slots V + 2 j and V + 2 j + 1 are the second copies of the bridge ends of the j-th processed hole. vert[] is the slot -> vertex map;
// while the bridges are built, vert[i] of a vertex slot that is not yet in the merged ring holds VGX_TRI_UNLINKED.
#define VGX_TRI_MAX_RINGS ((VGX_TRIANGULATE_MAX_VERTICES + 2u) / 5u) // 3 S + 2 (S - 1) <= the cap

// 0 (no mesh), TOO_LONG, or VGX_TRI_ROUTE_TRIANGLES = "the rings decide"; *V the vertex count, *H the holes. Never MULTI
VGX_HD uint32_t tri_rings_draw_class(const vgx_draw& d, const vgx_draw_info& di, const vgx_subpath* subs, uint64_t* V, uint32_t* H, int* made)
{
	*made = contours_draw_counts(d, di, subs, V);
	*H = 0u;
	if (*made <= 0) { return 0u; }
	*H = di.num_subpaths - 1u;
	if (*V + 2ull * *H > VGX_TRIANGULATE_MAX_VERTICES) { return VGX_TRI_REFUSED_TOO_LONG; }
	return VGX_TRI_ROUTE_TRIANGLES;
}

VGX_HD void tri_rings_draw_sizes(const vgx_draw& d, uint32_t route, uint64_t V, uint32_t H, uint64_t* nv, uint64_t* ni, uint32_t* nm, bool* tooLarge)
{
	tri_draw_sizes(d, route, V, nv, ni, nm, tooLarge);
	if (route == VGX_TRI_ROUTE_TRIANGLES) { *ni += 6ull * H; } // 3 (V + 2 H - 2) triangle indices
}

VGX_HD uint32_t tri_rings_draw_meshes(const vgx_draw& d, uint32_t drawIndex, uint32_t route, uint64_t V, uint32_t H, uint64_t firstVertex, uint64_t firstIndex, vgx_mesh* m)
{
	const uint32_t n = tri_draw_meshes(d, drawIndex, route, V, firstVertex, firstIndex, m);
	if (route == VGX_TRI_ROUTE_TRIANGLES) { m[0].num_indices += 6u * H; }
	return n;
}

// the sub-path of draw-local vertex c among the draw's nsub: the last that starts at or before c
VGX_HD uint32_t tri_ring_of(const vgx_subpath* sp, uint32_t nsub, uint32_t c)
{
	uint32_t lo = 0, hi = nsub;
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if (sp[mid].first_vertex - sp[0].first_vertex <= c) { lo = mid; } else { hi = mid; }
	}
	return lo;
}

// draw-local vertex c of the rings: the polyline vertex, with AA the vertex vgx_concave_move gives for its contour
VGX_HD V2 tri_rings_vertex(const float* poly, const vgx_subpath* sp, uint32_t nsub, const vgx_draw& d, uint32_t c)
{
	const uint32_t r = tri_ring_of(sp, nsub, c);
	return tri_ring_vertex(poly + 2 * sp[r].first_vertex, sp[r].num_vertices, d, c - (uint32_t)(sp[r].first_vertex - sp[0].first_vertex));
}

// is p after m in (x, then y), strictly? (a bridge goes forwards)
VGX_HD bool tri_after(V2 p, V2 m) { return p.x > m.x || (p.x == m.x && p.y > m.y); }

VGX_HD bool tri_same_place(V2 p, V2 q) { return p.x == q.x && p.y == q.y; }

// does the edge u -> v count for inside(p, .)?
VGX_HD bool tri_inside_edge(V2 u, V2 v, V2 p)
{
	if ((u.y <= p.y) == (v.y <= p.y)) { return false; }
	return tri_sign(tri_edge(u, v, p)) == (v.y > u.y ? 1 : -1);
}

// does the corner a -> q -> n of a ring of orientation s see m?
VGX_HD bool tri_cone(V2 a, V2 q, V2 n, V2 m, double s)
{
	const double t = s * tri_edge(a, q, n), e1 = s * tri_edge(a, q, m), e2 = s * tri_edge(q, n, m);
	return t > 0.0 ? (e1 > 0.0 && e2 > 0.0) : (e1 > 0.0 || e2 > 0.0);
}

VGX_HD double tri_d2(V2 m, V2 q)
{
	const double dx = (double)q.x - (double)m.x, dy = (double)q.y - (double)m.y;
	return dx * dx + dy * dy;
}

VGX_HD bool tri_key_less(double d, uint32_t slot, double d0, uint32_t slot0) { return d < d0 || (d == d0 && slot < slot0); }

// does p keep (a, b, c) from being an ear, under the amendment: a slot at the place of a, b or c does not
VGX_HD bool tri_blocks_slot(V2 a, V2 b, V2 c, V2 p, double s)
{
	if (tri_same_place(p, a) || tri_same_place(p, b) || tri_same_place(p, c)) { return false; }
	return tri_blocks(a, b, c, p, s);
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the pieces the host walks of the rings entry and of the nested entry (further down) share -------------------------------------
// The rings' links, per ring its orientation and its greatest vertex, the draw's smallest vertex (*lowest), and the refusals that need
// no nesting: NONFINITE, DEGENERATE, NOT_SIMPLE over the whole draw. VGX_TRI_ROUTE_TRIANGLES: none of them. vert[] is left UNLINKED
static inline uint32_t tri_rings_prepare(const V2* pos, uint32_t V, const vgx_subpath* sp, uint32_t S, uint16_t* vert, uint16_t* prev, uint16_t* next, int8_t* sgn, uint16_t* mh,
                                         uint32_t* lowest)
{
	for (uint32_t j = 0; j < V; ++j) { if (!tri_finite(pos[j])) { return VGX_TRI_REFUSED_NONFINITE; } }
	*lowest = 0;
	for (uint32_t r = 0; r < S; ++r) {
		const uint32_t first = (uint32_t)(sp[r].first_vertex - sp[0].first_vertex), n = sp[r].num_vertices;
		uint32_t k = first, g = first;
		for (uint32_t j = first; j < first + n; ++j) {
			prev[j] = (uint16_t)(j > first ? j - 1 : first + n - 1); next[j] = (uint16_t)(j + 1 < first + n ? j + 1 : first);
			vert[j] = VGX_TRI_UNLINKED;
			if (tri_before(pos[j], j, pos[k], k)) { k = j; }
			if (tri_before(pos[g], g, pos[j], j)) { g = j; }
		}
		sgn[r] = (int8_t)tri_sign(tri_edge(pos[prev[k]], pos[k], pos[next[k]]));
		mh[r] = (uint16_t)g;
		if (tri_before(pos[k], k, pos[*lowest], *lowest)) { *lowest = k; }
	}
	for (uint32_t r = 0; r < S; ++r) { if (sgn[r] == 0) { return VGX_TRI_REFUSED_DEGENERATE; } }
	for (uint32_t i = 0; i + 1 < V; ++i) {
		for (uint32_t j = i + 1; j < V; ++j) {
			if (next[i] == j || next[j] == i) { continue; } // a common vertex index
			if (tri_edges_meet(pos[i], pos[next[i]], pos[j], pos[next[j]])) { return VGX_TRI_REFUSED_NOT_SIMPLE; }
		}
	}
	return VGX_TRI_ROUTE_TRIANGLES;
}

// inside(p, ring of n vertices from `first`), by the ring's own vertex order
static inline bool tri_inside_ring(const V2* pos, uint32_t first, uint32_t n, V2 p)
{
	bool in = false;
	for (uint32_t j = first; j < first + n; ++j) { in = in != tri_inside_edge(pos[j], pos[j + 1 < first + n ? j + 1 : first], p); }
	return in;
}

// One bridge: hole h (bridge vertex M = mh[h]) of the ring merged so far around outer ring o of orientation so, as the j-th processed
// hole of its group. The group's slots so far are its vertex slots among the V -- those of the rings r with outer[r] == o; outer == null:
// every ring (the rings entry) -- and the 2 j bridge slots from slot0. Searches, and on success splices with the new slots slot0 + 2 j
// and slot0 + 2 j + 1. *tried: the candidates the search tried. false: no bridge
static inline bool tri_bridge_hole(const V2* pos, uint32_t V, const vgx_subpath* sp, uint32_t S, const uint16_t* outer, uint32_t o, int so, uint32_t h, int sh, uint32_t M,
                                   uint32_t j, uint32_t slot0, uint16_t* vert, uint16_t* prev, uint16_t* next, uint32_t* tried)
{
	const double s = (double)so;
	const uint32_t slots = V + 2u * j;
	const V2 pm = pos[M];
	double rejected = -1.0; uint32_t rejectedSlot = 0; // the last rejected key; d2 >= 0
	uint32_t q = 0xFFFFFFFFu;
	*tried = 0;
	for (;;) {
		double best = 0.0; uint32_t bestSlot = 0xFFFFFFFFu;
		for (uint32_t i = 0; i < slots; ++i) {
			const uint32_t x = i < V ? i : i - V + slot0;
			if (vert[x] == VGX_TRI_UNLINKED || (outer && x < V && outer[tri_ring_of(sp, S, x)] != o)) { continue; }
			const V2 px = pos[vert[x]];
			if (!tri_after(px, pm) || !tri_cone(pos[vert[prev[x]]], px, pos[vert[next[x]]], pm, s)) { continue; }
			const double d = tri_d2(pm, px);
			if (!tri_key_less(rejected, rejectedSlot, d, x)) { continue; }
			if (bestSlot == 0xFFFFFFFFu || tri_key_less(d, x, best, bestSlot)) { best = d; bestSlot = x; }
		}
		if (bestSlot == 0xFFFFFFFFu) { break; }
		++*tried;
		const uint32_t vq = vert[bestSlot];
		bool hidden = false;
		for (uint32_t i = 0; i < slots && !hidden; ++i) { // the rings' edges and the earlier bridges are the links of the slots so far
			const uint32_t x = i < V ? i : i - V + slot0;
			if (outer && x < V && outer[tri_ring_of(sp, S, x)] != o) { continue; }
			const uint32_t u = x < V ? x : vert[x], y = next[x], w = y < V ? y : vert[y];
			if (u == M || w == M || u == vq || w == vq) { continue; }
			hidden = tri_edges_meet(pm, pos[vq], pos[u], pos[w]);
		}
		if (!hidden) { q = bestSlot; break; }
		rejected = best; rejectedSlot = bestSlot;
	}
	if (q == 0xFFFFFFFFu) { return false; }
	const uint32_t first = (uint32_t)(sp[h].first_vertex - sp[0].first_vertex), A = slot0 + 2u * j, B = A + 1u;
	for (uint32_t k = first; k < first + sp[h].num_vertices; ++k) {
		if (sh == so) { const uint16_t t = prev[k]; prev[k] = next[k]; next[k] = t; } // traversed backwards
		vert[k] = (uint16_t)k;
	}
	const uint32_t qn = next[q], last = prev[M];
	vert[A] = (uint16_t)M; vert[B] = vert[q];
	next[q] = (uint16_t)M; prev[M] = (uint16_t)q;
	next[last] = (uint16_t)A; prev[A] = (uint16_t)last;
	next[A] = (uint16_t)B; prev[B] = (uint16_t)A;
	next[B] = (uint16_t)qn; prev[qn] = (uint16_t)B;
	return true;
}

// The clipping loop over one ring of `size` linked slots from cursor b; amend: a slot at the place of a, b or c does not block. Appends
// vertex triples at tri[*nt ..]. false: STALLED
static inline bool tri_clip_slots(const V2* pos, const uint16_t* vert, uint16_t* prev, uint16_t* next, double s, uint32_t b, uint32_t size, bool amend, uint16_t* tri,
                                  uint32_t* nt)
{
	uint32_t misses = 0;
	while (size > 3) {
		const uint32_t a = prev[b], c = next[b];
		const V2 pa = pos[vert[a]], pb = pos[vert[b]], pc = pos[vert[c]];
		const double t = s * tri_edge(pa, pb, pc);
		bool ear = t == 0.0;
		if (t > 0.0) {
			ear = true;
			for (uint32_t p = next[c]; p != a && ear; p = next[p]) { ear = amend ? !tri_blocks_slot(pa, pb, pc, pos[vert[p]], s) : !tri_blocks(pa, pb, pc, pos[vert[p]], s); }
		}
		if (ear) {
			tri[(*nt)++] = vert[a]; tri[(*nt)++] = vert[b]; tri[(*nt)++] = vert[c];
			next[a] = (uint16_t)c; prev[c] = (uint16_t)a; prev[b] = VGX_TRI_UNLINKED;
			b = next[c]; --size; misses = 0;
		} else {
			b = c;
			if (++misses > size) { return false; }
		}
	}
	tri[(*nt)++] = vert[prev[b]]; tri[(*nt)++] = vert[b]; tri[(*nt)++] = vert[next[b]];
	return true;
}

// The rule on the host for a draw of S >= 1 rings, step after step. pos[0 .. V): the rings' vertices (with AA the moved ones); sp: the
// draw's S sub-paths. vert / prev / next: N = V + 2 (S - 1) entries each; sgn, mh: S entries; tri receives 3 (N - 2) draw-local VERTEX
// indices when the route is VGX_TRI_ROUTE_TRIANGLES. trips (may be null): per processed hole the candidates its search tried
static inline uint32_t tri_rings_route(const V2* pos, uint32_t V, const vgx_subpath* sp, uint32_t S, bool evenOdd, uint16_t* vert, uint16_t* prev, uint16_t* next,
                                       int8_t* sgn, uint16_t* mh, uint16_t* tri, uint32_t* trips)
{
	const uint32_t H = S - 1u, N = V + 2u * H;
	uint32_t lowest;
	const uint32_t early = tri_rings_prepare(pos, V, sp, S, vert, prev, next, sgn, mh, &lowest);
	if (early != VGX_TRI_ROUTE_TRIANGLES) { return early; }
	const uint32_t o = tri_ring_of(sp, S, lowest);
	for (uint32_t h = 0; h < S; ++h) {
		if (h == o) { continue; }
		if (!evenOdd && sgn[h] != -sgn[o]) { return VGX_TRI_REFUSED_NESTING; }
		for (uint32_t r = 0; r < S; ++r) {
			if (r == h) { continue; }
			if (tri_inside_ring(pos, (uint32_t)(sp[r].first_vertex - sp[0].first_vertex), sp[r].num_vertices, pos[mh[h]]) != (r == o)) { return VGX_TRI_REFUSED_NESTING; }
		}
	}
	{
		const uint32_t first = (uint32_t)(sp[o].first_vertex - sp[0].first_vertex);
		for (uint32_t j = first; j < first + sp[o].num_vertices; ++j) { vert[j] = (uint16_t)j; }
	}
	uint32_t lastHole = 0xFFFFFFFFu; // holes in descending order of their bridge vertex
	for (uint32_t jh = 0; jh < H; ++jh) {
		uint32_t h = 0xFFFFFFFFu;
		for (uint32_t r = 0; r < S; ++r) {
			if (r == o) { continue; }
			if (lastHole != 0xFFFFFFFFu && !tri_before(pos[mh[r]], mh[r], pos[mh[lastHole]], mh[lastHole])) { continue; }
			if (h == 0xFFFFFFFFu || tri_before(pos[mh[h]], mh[h], pos[mh[r]], mh[r])) { h = r; }
		}
		lastHole = h;
		uint32_t tried;
		const bool found = tri_bridge_hole(pos, V, sp, S, nullptr, o, sgn[o], h, sgn[h], mh[h], jh, V, vert, prev, next, &tried);
		if (trips) { trips[jh] = tried; }
		if (!found) { return VGX_TRI_REFUSED_NO_BRIDGE; }
	}
	uint32_t nt = 0;
	return tri_clip_slots(pos, vert, prev, next, (double)sgn[o], 0u, N, true, tri, &nt) ? VGX_TRI_ROUTE_TRIANGLES : VGX_TRI_REFUSED_STALLED;
}

// The rule on the host, vertex after vertex: the route of the ring pos[0 .. V) (3 <= V <= VGX_TRIANGULATE_MAX_VERTICES) and, when it is
// VGX_TRI_ROUTE_TRIANGLES, its 3 (V - 2) ring-local indices in tri. prev / next: V links each
static inline uint32_t tri_ring_route(const V2* pos, uint32_t V, uint16_t* prev, uint16_t* next, uint16_t* tri)
{
	uint32_t k = 0;
	for (uint32_t j = 0; j < V; ++j) {
		if (!tri_finite(pos[j])) { return VGX_TRI_REFUSED_NONFINITE; }
		if (tri_before(pos[j], j, pos[k], k)) { k = j; }
		prev[j] = (uint16_t)(j ? j - 1 : V - 1); next[j] = (uint16_t)(j + 1 < V ? j + 1 : 0);
	}
	const int sg = tri_sign(tri_edge(pos[prev[k]], pos[k], pos[next[k]]));
	if (sg == 0) { return VGX_TRI_REFUSED_DEGENERATE; }
	const double s = (double)sg;
	for (uint32_t i = 0; i + 2 < V; ++i) {
		for (uint32_t j = i + 2; j < V; ++j) {
			if (i == 0 && j == V - 1) { continue; } // the closing edge shares vertex 0
			if (tri_edges_meet(pos[i], pos[i + 1], pos[j], pos[next[j]])) { return VGX_TRI_REFUSED_NOT_SIMPLE; }
		}
	}
	uint32_t b = 0, size = V, misses = 0, nt = 0;
	while (size > 3) {
		const uint32_t a = prev[b], c = next[b];
		const double t = s * tri_edge(pos[a], pos[b], pos[c]);
		bool ear = t == 0.0;
		if (t > 0.0) {
			ear = true;
			for (uint32_t p = next[c]; p != a && ear; p = next[p]) { ear = !tri_blocks(pos[a], pos[b], pos[c], pos[p], s); }
		}
		if (ear) {
			tri[nt++] = (uint16_t)a; tri[nt++] = (uint16_t)b; tri[nt++] = (uint16_t)c;
			next[a] = (uint16_t)c; prev[c] = (uint16_t)a; prev[b] = VGX_TRI_UNLINKED;
			b = next[c]; --size; misses = 0;
		} else {
			b = c;
			if (++misses > size) { return VGX_TRI_REFUSED_STALLED; }
		}
	}
	tri[nt++] = prev[b]; tri[nt++] = (uint16_t)b; tri[nt++] = next[b];
	return VGX_TRI_ROUTE_TRIANGLES;
}
#endif

// ---- vgx_concave_triangulate_nested: several outlines, islands in holes (include/vgx.h) ---------------------------------------------------
// The rings are classified by containment depth and cut into GROUPS of one even-depth ring (the group's outer ring) plus the odd-depth
// rings directly inside it (its holes); every group goes through the slots, bridges and clipping above with "the draw" read as "the
// group". A group is named by its outer ring; groups are numbered ascending by that sub-path index. Per ring r the tables hold
// outer[r] = the outer ring of r's group (r itself for an even depth); per outer ring o: holes[o] = H_g, before[o] = B_g (the holes of the
// groups before it) and first_tri[o] = the triangles of the groups before it.
VGX_HD bool tri_nested_is_hole(uint32_t depth) { return (depth & 1u) != 0u; }

// triangles of a group of Vg vertices and Hg holes
VGX_HD uint32_t tri_nested_group_triangles(uint32_t Vg, uint32_t Hg) { return Vg + 2u * Hg - 2u; }

// does orientation sh of a hole fit its parent's sp?
VGX_HD bool tri_nested_hole_fits(int sh, int sp, bool evenOdd) { return evenOdd || sh == -sp; }

// 3 (V + 2 S - 4 G) triangle indices: tri_draw_sizes' 3 (V - 2) and the difference
VGX_HD void tri_nested_draw_sizes(const vgx_draw& d, uint32_t route, uint64_t V, uint32_t S, uint32_t G, uint64_t* nv, uint64_t* ni, uint32_t* nm, bool* tooLarge)
{
	tri_draw_sizes(d, route, V, nv, ni, nm, tooLarge);
	if (route == VGX_TRI_ROUTE_TRIANGLES) { *ni = *ni + 6ull * S + 6ull - 12ull * G; }
}

VGX_HD uint32_t tri_nested_draw_meshes(const vgx_draw& d, uint32_t drawIndex, uint32_t route, uint64_t V, uint32_t S, uint32_t G, uint64_t firstVertex, uint64_t firstIndex, vgx_mesh* m)
{
	const uint32_t n = tri_draw_meshes(d, drawIndex, route, V, firstVertex, firstIndex, m);
	if (route == VGX_TRI_ROUTE_TRIANGLES) { m[0].num_indices = m[0].num_indices + 6u * S + 6u - 12u * G; }
	return n;
}

#ifndef __HIP_DEVICE_COMPILE__
// The rule on the host for a draw of S >= 1 rings, from the pieces of tri_rings_route. pos, sp, vert / prev / next, sgn, mh, tri, trips:
// as there (trips per processed hole B_g + j). tab: 6 S entries (depth, outer, holes, before, first_tri, order). *groups receives G
// when the route is VGX_TRI_ROUTE_TRIANGLES
static inline uint32_t tri_nested_route(const V2* pos, uint32_t V, const vgx_subpath* sp, uint32_t S, bool evenOdd, uint16_t* vert, uint16_t* prev, uint16_t* next,
                                        int8_t* sgn, uint16_t* mh, uint16_t* tab, uint16_t* tri, uint32_t* groups, uint32_t* trips)
{
	uint16_t* depth = tab, * outer = tab + S, * holes = tab + 2 * S, * before = tab + 3 * S, * firstTri = tab + 4 * S, * order = tab + 5 * S;
	uint32_t lowest;
	const uint32_t early = tri_rings_prepare(pos, V, sp, S, vert, prev, next, sgn, mh, &lowest);
	if (early != VGX_TRI_ROUTE_TRIANGLES) { return early; }
	// depth, parent, groups
	for (uint32_t r = 0; r < S; ++r) {
		uint32_t n = 0;
		for (uint32_t q = 0; q < S; ++q) {
			if (q != r && tri_inside_ring(pos, (uint32_t)(sp[q].first_vertex - sp[0].first_vertex), sp[q].num_vertices, pos[mh[r]])) { ++n; }
		}
		depth[r] = (uint16_t)n;
	}
	for (uint32_t r = 0; r < S; ++r) {
		uint32_t parents = 0, parent = r;
		for (uint32_t q = 0; q < S && depth[r] > 0u; ++q) {
			if (q == r || depth[q] + 1u != depth[r]) { continue; }
			if (tri_inside_ring(pos, (uint32_t)(sp[q].first_vertex - sp[0].first_vertex), sp[q].num_vertices, pos[mh[r]])) { ++parents; parent = q; }
		}
		if (depth[r] > 0u && parents != 1u) { return VGX_TRI_REFUSED_NESTING; }
		const bool hole = tri_nested_is_hole(depth[r]);
		if (hole && !tri_nested_hole_fits(sgn[r], sgn[parent], evenOdd)) { return VGX_TRI_REFUSED_NESTING; }
		outer[r] = (uint16_t)(hole ? parent : r);
	}
	uint32_t G = 0, B = 0, T = 0;
	for (uint32_t o = 0; o < S; ++o) {
		if (outer[o] != o) { continue; }
		uint32_t Hg = 0, Vg = 0;
		for (uint32_t r = 0; r < S; ++r) { if (outer[r] == o) { Vg += sp[r].num_vertices; Hg += r != o; } }
		holes[o] = (uint16_t)Hg; before[o] = (uint16_t)B; firstTri[o] = (uint16_t)T;
		++G; B += Hg; T += tri_nested_group_triangles(Vg, Hg);
	}
	for (uint32_t h = 0; h < S; ++h) { // a group's holes in descending order of their bridge vertex
		const uint32_t o = outer[h];
		if (o == h) { continue; }
		uint32_t rank = 0;
		for (uint32_t g = 0; g < S; ++g) { if (g != h && g != o && outer[g] == o && tri_before(pos[mh[h]], mh[h], pos[mh[g]], mh[g])) { ++rank; } }
		order[before[o] + rank] = (uint16_t)h;
	}
	uint32_t limit = S; // the first group that finds no bridge: the groups from it on decide nothing any more
	for (uint32_t o = 0; o < S && limit == S; ++o) {
		if (outer[o] != o) { continue; }
		const uint32_t first = (uint32_t)(sp[o].first_vertex - sp[0].first_vertex);
		for (uint32_t j = first; j < first + sp[o].num_vertices; ++j) { vert[j] = (uint16_t)j; }
		for (uint32_t jh = 0; jh < holes[o] && limit == S; ++jh) {
			const uint32_t h = order[before[o] + jh];
			uint32_t tried;
			const bool found = tri_bridge_hole(pos, V, sp, S, outer, o, sgn[o], h, sgn[h], mh[h], jh, V + 2u * before[o], vert, prev, next, &tried);
			if (trips) { trips[before[o] + jh] = tried; }
			if (!found) { limit = o; }
		}
	}
	for (uint32_t o = 0; o < limit; ++o) { // group after group; the ear test walks the group's own ring
		if (outer[o] != o) { continue; }
		uint32_t b = (uint32_t)(sp[o].first_vertex - sp[0].first_vertex), size = 0, nt = 3u * firstTri[o];
		for (uint32_t r = 0; r < S; ++r) {
			if (outer[r] != o) { continue; }
			const uint32_t first = (uint32_t)(sp[r].first_vertex - sp[0].first_vertex);
			size += sp[r].num_vertices + (r != o ? 2u : 0u);
			if (first < b) { b = first; }
		}
		// a group of one ring: vgx_concave_triangulate's loop, with no amendment
		if (!tri_clip_slots(pos, vert, prev, next, (double)sgn[o], b, size, holes[o] != 0u, tri, &nt)) { return VGX_TRI_REFUSED_STALLED; }
	}
	if (limit != S) { return VGX_TRI_REFUSED_NO_BRIDGE; }
	*groups = G;
	return VGX_TRI_ROUTE_TRIANGLES;
}
#endif

#endif
