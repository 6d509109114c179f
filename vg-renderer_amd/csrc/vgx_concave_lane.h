// vgx_concave_lane.h -- the per-vertex arithmetic of strokerConcaveFillEndAA's fringe loop (reference src/stroker.cpp:887-973) for ONE
// contour vertex: host + device. The kernels of vgx_concave.hip run it one contour vertex per lane; the host backend of the per-call
// compat layer (host/vgx_host_backend.hip) runs the same functions vertex after vertex.
#ifndef VGX_CONCAVE_LANE_H
#define VGX_CONCAVE_LANE_H

#include "vgx_lane.h"

VGX_HD V2 ldc(const float* v, uint64_t i)
{
#ifdef __HIPCC__
	const float2 t = *(const float2*)(v + 2 * i);
	return v2(t.x, t.y);
#else // the plain C++ build of libvgx_hosttest.so has no float2
	return v2(v[2 * i], v[2 * i + 1]);
#endif
}

struct FringePair { V2 in, out; }; // p[inner], p[1 - inner]

// contour-wide constants: aa = fringe / 2 * sign(cross(d(last,0), d(0,1))), inner = sign < 0 ? 0 : 1 (stroker.cpp:895-898)
VGX_HD float contour_cross_sign(const float* v, uint32_t n)
{
	const V2 d01 = v2dir(ldc(v, n - 1), ldc(v, 0));
	return vgm_sign(v2cross(d01, v2dir(ldc(v, 0), ldc(v, n > 1 ? 1 : 0))));
}

VGX_HD FringePair fringe_of(V2 p1, V2 d01, V2 d12, float aa, bool innerIsSecond)
{
	const V2 vaa = v2mul(v2extrude(d01, d12), aa);
	const V2 p0 = v2sub(p1, vaa), pp1 = v2add(p1, vaa);
	FringePair r;
	r.in = innerIsSecond ? pp1 : p0;
	r.out = innerIsSecond ? p0 : pp1;
	return r;
}

// vertex j of a contour of n original vertices v[0..n): both fringe vertices (stroker.cpp:899-927)
VGX_HD FringePair contour_vertex(const float* v, uint32_t n, uint32_t j, float fringe)
{
	const float crossSign = contour_cross_sign(v, n);
	const float aa = fringe * 0.5f * crossSign;
	const bool innerIsSecond = !(crossSign < 0.0f);
	const V2 p1 = ldc(v, j);
	const V2 pPrev = ldc(v, j > 0 ? j - 1 : n - 1);
	const V2 d01 = v2dir(pPrev, p1); // iteration j's d01 = iteration j-1's d12 = dir(original v[j-1], original v[j]); j = 0: dir(v[n-1], v[0])
	V2 p2 = ldc(v, j + 1 < n ? j + 1 : 0);
	if (j + 1 == n && n > 1) { // the closing iteration reads vertex 0 AFTER iteration 0 moved it
		const V2 q0 = ldc(v, 0);
		const FringePair f0 = fringe_of(q0, v2dir(ldc(v, n - 1), q0), v2dir(q0, ldc(v, 1)), aa, innerIsSecond);
		p2 = f0.in;
	}
	return fringe_of(p1, d01, v2dir(p1, p2), aa, innerIsSecond);
}

// ---- vgx_concave_contours: a concave draw's own sub-paths as contour meshes (include/vgx.h) ------------------------------------------
// Does draw d make meshes, and from how many contour vertices? 1: yes, *V = the sum of its sub-paths' vertex counts. 0: no (another sort
// of draw, no sub-path, or a sub-path below 3 vertices: the reference's return, src/vg.cpp:3136-3138). -1: its sub-paths do not lie back
// to back in the polyline array, which vgx_flatten never writes: the call ends with VGX_E_INVALID_ARG
VGX_HD int contours_draw_counts(const vgx_draw& d, const vgx_draw_info& di, const vgx_subpath* subs, uint64_t* V)
{
	*V = 0;
	if (!(d.fill_flags & VGX_FILL_CONCAVE) || (d.fill_flags & VGX_FILL_ENABLE) || di.num_subpaths == 0u) { return 0; }
	const vgx_subpath* sp = subs + di.first_subpath;
	bool small = false;
	uint64_t v = 0;
	for (uint32_t k = 0; k < di.num_subpaths; ++k) {
		if (sp[k].first_vertex != sp[0].first_vertex + v) { return -1; }
		small = small || sp[k].num_vertices < 3u;
		v += sp[k].num_vertices;
	}
	if (small) { return 0; }
	*V = v;
	return 1;
}

// the records of a draw of V contour vertices whose first mesh starts at (firstVertex, firstIndex): 1 (no AA) or 2 (AA: fringe, interior)
VGX_HD uint32_t contours_draw_meshes(const vgx_draw& d, uint32_t drawIndex, uint64_t V, uint64_t firstVertex, uint64_t firstIndex, vgx_mesh* m)
{
	const uint32_t rule = (d.fill_flags & VGX_FILL_EVEN_ODD) ? VGX_CONTOUR_EVEN_ODD : 0u;
	uint32_t k = 0;
	if (d.fill_flags & VGX_FILL_AA) {
		m[k].first_vertex = firstVertex; m[k].first_index = firstIndex; m[k].num_vertices = (uint32_t)(2 * V); m[k].num_indices = (uint32_t)(6 * V);
		m[k].draw = drawIndex; m[k].subpath_kind = (uint32_t)VGX_MESH_CONCAVE_FILL_AA << 28;
		firstVertex += 2 * V; firstIndex += 6 * V;
		++k;
	}
	m[k].first_vertex = firstVertex; m[k].first_index = firstIndex; m[k].num_vertices = (uint32_t)V; m[k].num_indices = (uint32_t)(2 * V);
	m[k].draw = drawIndex; m[k].subpath_kind = ((uint32_t)VGX_MESH_CONTOURS << 28) | rule;
	return k + 1u;
}

// Contour vertex c (< V) of a mesh-making draw: everything the draw's meshes hold for it. sp = the draw's nsub sub-paths. Without AA the
// vertex and its outgoing edge; with AA the fringe pair and the six indices of its segment exactly as k_concave_fringe writes them, and
// behind the fringe the moved vertex (k_concave_move's) and its outgoing edge. Stores are one element wide: vgx_mesh_out's alignment.
// contours_emit_vertex_data writes all of it but the outgoing edge (vgx_concave_triangulate puts triangles there) and returns the
// vertex's place: `before` contour vertices of the draw lie in front of its sub-path, whose vertex j of n it is
struct ContourPlace { uint32_t before, j, n; };
VGX_HD ContourPlace contours_emit_vertex_data(const float* poly, const vgx_subpath* sp, uint32_t nsub, const vgx_draw& d, uint64_t c, uint64_t V,
                                              uint64_t firstVertex, uint64_t firstIndex, float* pos, uint32_t* color, uint16_t* idx)
{
	uint32_t lo = 0, hi = nsub; // the last sub-path that starts at or before c
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if (sp[mid].first_vertex - sp[0].first_vertex <= c) { lo = mid; } else { hi = mid; }
	}
	const uint32_t before = (uint32_t)(sp[lo].first_vertex - sp[0].first_vertex), n = sp[lo].num_vertices;
	const uint32_t j = (uint32_t)c - before;
	const float* v = poly + 2 * sp[lo].first_vertex;
	V2 p = ldc(v, j);
	if (d.fill_flags & VGX_FILL_AA) {
		const FringePair f = contour_vertex(v, n, j, d.fringe);
		const uint64_t gv = firstVertex + 2 * c;
		pos[2 * gv] = f.in.x; pos[2 * gv + 1] = f.in.y; pos[2 * gv + 2] = f.out.x; pos[2 * gv + 3] = f.out.y;
		color[gv] = d.fill_color; color[gv + 1] = d.fill_color & 0x00FFFFFFu;
		const uint32_t vb = 2 * before;
		const uint32_t id0 = vb + 2 * j, id1 = id0 + 1, id2 = (j + 1 < n) ? id0 + 2 : vb, id3 = id2 + 1;
		uint16_t* pi = idx + firstIndex + 6 * c;
		pi[0] = (uint16_t)id0; pi[1] = (uint16_t)id2; pi[2] = (uint16_t)id1;
		pi[3] = (uint16_t)id2; pi[4] = (uint16_t)id3; pi[5] = (uint16_t)id1;
		p = f.in;
		firstVertex += 2 * V;
	}
	pos[2 * (firstVertex + c)] = p.x; pos[2 * (firstVertex + c) + 1] = p.y;
	color[firstVertex + c] = d.fill_color;
	ContourPlace at;
	at.before = before; at.j = j; at.n = n;
	return at;
}

VGX_HD void contours_emit_vertex(const float* poly, const vgx_subpath* sp, uint32_t nsub, const vgx_draw& d, uint64_t c, uint64_t V,
                                 uint64_t firstVertex, uint64_t firstIndex, float* pos, uint32_t* color, uint16_t* idx)
{
	const ContourPlace at = contours_emit_vertex_data(poly, sp, nsub, d, c, V, firstVertex, firstIndex, pos, color, idx);
	if (d.fill_flags & VGX_FILL_AA) { firstIndex += 6 * V; }
	idx[firstIndex + 2 * c] = (uint16_t)(at.before + at.j);
	idx[firstIndex + 2 * c + 1] = (uint16_t)(at.j + 1 < at.n ? at.before + at.j + 1 : at.before);
}

#endif
