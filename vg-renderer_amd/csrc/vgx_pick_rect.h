// vgx_pick_rect.h -- the arithmetic of vgx_pick_rect for ONE triangle, ONE box, ONE query and ONE entry: host + device.
// The kernels of vgx_pick_rect.hip run it one mesh / one triangle per lane; libvgx_hosttest.so (vgx_hosttest.cpp: vgxt_pick_rect) runs the
// same functions query after query, mesh after mesh and triangle after triangle so that the CPU suite pins the arithmetic without a GPU.
//
// The specification is in include/vgx.h (vgx_pick_rect). What a triangle is, which triangles are considered and the key of a hit are
// vgx_pick.h's (vgx_pick_mesh_triangles, vgx_pick_tri_valid, vgx_pick_tri_transparent, vgx_pick_key): nothing of them is restated here.
// Compiled with -ffp-contract=off on both sides, as vgx_pick.h is.
#ifndef VGX_PICK_RECT_H
#define VGX_PICK_RECT_H

#include "vgx_pick.h"

// ---- the query -----------------------------------------------------------------------------------------------------------
// step 1, and the reserved word: a query that fails selects nothing. A NaN coordinate fails a compare
VGX_HD bool vgx_pickr_query_valid(const vgx_pick_rect_query& Q) { return Q.reserved == 0u && Q.x0 <= Q.x1 && Q.y0 <= Q.y1; }

// mesh m (< num_meshes: the caller's check) is in the query's range
VGX_HD bool vgx_pickr_in_range(const vgx_pick_rect_query& Q, uint64_t m) { return (uint64_t)Q.mesh_begin <= m && m < (uint64_t)Q.mesh_end; }

// ---- the two box rules, binary32 compares: false with a NaN on either side -------------------------------------------------
// step 2 for a triangle's box, and the prefilter for a mesh's: every indexed vertex lies in the mesh box, so a mesh whose box fails
// has no triangle that passes
VGX_HD bool vgx_pickr_box_overlap(const vgx_pick_rect_query& Q, float minx, float miny, float maxx, float maxy)
{
	return Q.x1 >= minx && Q.x0 <= maxx && Q.y1 >= miny && Q.y0 <= maxy;
}

// inside(m): the mesh's box lies in R. The empty box (+inf, +inf, -inf, -inf) passes for every valid R
VGX_HD bool vgx_pickr_box_inside(const vgx_pick_rect_query& Q, float minx, float miny, float maxx, float maxy)
{
	return minx >= Q.x0 && maxx <= Q.x1 && miny >= Q.y0 && maxy <= Q.y1;
}

// ---- rectangle touches triangle ----------------------------------------------------------------------------------------------
// What does not depend on the rectangle, set up once per triangle: its box, the sign of A, and of every edge u -> v the start and the
// two differences
struct VgxPickrTri
{
	float lox, loy, hix, hiy;
	double ux[3], uy[3], dx[3], dy[3];
	int sign; // +1: A > 0, -1: A < 0, 0: A == 0 or NaN -- the triangle touches nothing
};

VGX_HD void vgx_pickr_setup(V2 a, V2 b, V2 c, VgxPickrTri* T)
{
	T->lox = a.x < b.x ? (a.x < c.x ? a.x : c.x) : (b.x < c.x ? b.x : c.x);
	T->hix = a.x > b.x ? (a.x > c.x ? a.x : c.x) : (b.x > c.x ? b.x : c.x);
	T->loy = a.y < b.y ? (a.y < c.y ? a.y : c.y) : (b.y < c.y ? b.y : c.y);
	T->hiy = a.y > b.y ? (a.y > c.y ? a.y : c.y) : (b.y > c.y ? b.y : c.y);
	const double ax = a.x, ay = a.y, bx = b.x, by = b.y, cx = c.x, cy = c.y;
	const double A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
	T->sign = A > 0.0 ? 1 : (A < 0.0 ? -1 : 0);
	T->ux[0] = ax; T->uy[0] = ay; T->dx[0] = bx - ax; T->dy[0] = by - ay;
	T->ux[1] = bx; T->uy[1] = by; T->dx[1] = cx - bx; T->dy[1] = cy - by;
	T->ux[2] = cx; T->uy[2] = cy; T->dx[2] = ax - cx; T->dy[2] = ay - cy;
}

// e(p) of edge k
VGX_HD double vgx_pickr_edge(const VgxPickrTri& T, int k, double px, double py) { return T.dx[k] * (py - T.uy[k]) - T.dy[k] * (px - T.ux[k]); }

VGX_HD bool vgx_pickr_edge_sign(int sign, double e) { return sign > 0 ? e >= 0.0 : e <= 0.0; }

// step 4 as the header states it: some corner of R passes
VGX_HD bool vgx_pickr_edge_pass4(const VgxPickrTri& T, int k, double x0, double y0, double x1, double y1)
{
	return vgx_pickr_edge_sign(T.sign, vgx_pickr_edge(T, k, x0, y0)) || vgx_pickr_edge_sign(T.sign, vgx_pickr_edge(T, k, x1, y0))
	    || vgx_pickr_edge_sign(T.sign, vgx_pickr_edge(T, k, x1, y1)) || vgx_pickr_edge_sign(T.sign, vgx_pickr_edge(T, k, x0, y1));
}

// ... and as one corner: the product dx * (py - uy) is largest at y1 for dx >= 0 and at y0 below, the product dy * (px - ux) is
// smallest at x0 for dy >= 0 and at x1 below, each rounding is monotone, so that corner holds the largest e of the four; with A < 0
// the opposite corner holds the smallest. A NaN there (0 * inf) says nothing about the other three: all four are looked at then
VGX_HD bool vgx_pickr_edge_pass(const VgxPickrTri& T, int k, double x0, double y0, double x1, double y1)
{
	const bool pos = T.sign > 0;
	const double py = ((T.dx[k] >= 0.0) == pos) ? y1 : y0;
	const double px = ((T.dy[k] >= 0.0) == pos) ? x0 : x1;
	const double e = vgx_pickr_edge(T, k, px, py);
	if (e != e) { return vgx_pickr_edge_pass4(T, k, x0, y0, x1, y1); }
	return vgx_pickr_edge_sign(T.sign, e);
}

// steps 2 to 4 for a valid query (step 1: vgx_pickr_query_valid). fourCorners: the header's form of step 4 (the tests hold the two equal)
VGX_HD bool vgx_pickr_touch(const VgxPickrTri& T, const vgx_pick_rect_query& Q, bool fourCorners = false)
{
	if (!vgx_pickr_box_overlap(Q, T.lox, T.loy, T.hix, T.hiy) || T.sign == 0) { return false; }
	const double x0 = Q.x0, y0 = Q.y0, x1 = Q.x1, y1 = Q.y1;
	if (fourCorners) { return vgx_pickr_edge_pass4(T, 0, x0, y0, x1, y1) && vgx_pickr_edge_pass4(T, 1, x0, y0, x1, y1) && vgx_pickr_edge_pass4(T, 2, x0, y0, x1, y1); }
	return vgx_pickr_edge_pass(T, 0, x0, y0, x1, y1) && vgx_pickr_edge_pass(T, 1, x0, y0, x1, y1) && vgx_pickr_edge_pass(T, 2, x0, y0, x1, y1);
}

// ---- entries, one bit per query ----------------------------------------------------------------------------------------------
// window / byDraw: the queries with VGX_PICK_RECT_WINDOW / VGX_PICK_RECT_BY_DRAW. touch and inside of a mesh; runTouch = the OR of touch
// and runInside = the AND of inside over the mesh's run (a mesh outside a query's range has touch 0 and inside 1 there).
// The bits of a mesh or a run that is selected as an entry of its kind ...
VGX_HD uint64_t vgx_pickr_selected(uint64_t touch, uint64_t inside, uint64_t window) { return touch & (inside | ~window); }

// ... the queries that list an entry at mesh m: the mesh itself, or, at the first mesh of a run, the run
VGX_HD uint64_t vgx_pickr_entry_word(uint64_t touch, uint64_t inside, uint64_t runTouch, uint64_t runInside, bool runHead, uint64_t window, uint64_t byDraw)
{
	return (vgx_pickr_selected(touch, inside, window) & ~byDraw) | (runHead ? vgx_pickr_selected(runTouch, runInside, window) & byDraw : 0ull);
}

// ... and the queries for which mesh m has touch and belongs to a selected entry: out->top is the largest such mesh
VGX_HD uint64_t vgx_pickr_top_word(uint64_t touch, uint64_t inside, uint64_t runTouch, uint64_t runInside, uint64_t window, uint64_t byDraw)
{
	return (vgx_pickr_selected(touch, inside, window) & ~byDraw) | (touch & vgx_pickr_selected(runTouch, runInside, window) & byDraw);
}

// the value of the entry listed at mesh m: a run that began before the range is named by the range's first mesh
VGX_HD uint32_t vgx_pickr_entry_value(const vgx_pick_rect_query& Q, uint32_t m)
{
	return (Q.flags & VGX_PICK_RECT_BY_DRAW) && m < Q.mesh_begin ? Q.mesh_begin : m;
}

// out->top: bestMesh + 1 and bestTriangle + 1, 0 = none
VGX_HD vgx_pick_hit vgx_pickr_record(uint32_t meshPlus1, uint32_t triPlus1, const vgx_mesh* meshes)
{
	return vgx_pick_decode(meshPlus1 && triPlus1 ? vgx_pick_key(meshPlus1 - 1u, triPlus1 - 1u) : 0ull, meshes);
}

// The argument check of vgx_pick_rect and vgxt_pick_rect (host only). The first failing check of this order decides
static inline int vgx_pickr_check_args(const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_pick_rect_query* queries, uint32_t nqueries,
                                       const vgx_pick_rect_out* out)
{
	if (!frame || !out || (nqueries && !queries)) { return VGX_E_INVALID_ARG; }
	if (out->reserved != 0u || (out->list_cap && !out->list)) { return VGX_E_INVALID_ARG; }
	if (nqueries && frame->num_meshes && (!frame->pos || !frame->color || !frame->idx || !frame->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)queries & 15u) || ((uintptr_t)out->top & 15u) || ((uintptr_t)out->list & 3u) || ((uintptr_t)out->count & 3u) || ((uintptr_t)mesh_bounds & 15u)
		|| ((uintptr_t)frame->pos & 7u) || ((uintptr_t)frame->color & 3u) || ((uintptr_t)frame->idx & 1u) || ((uintptr_t)frame->meshes & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (nqueries > VGX_PICK_RECT_MAX_QUERIES || frame->num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	return VGX_OK;
}

#endif
