// vgx_pick.h -- the arithmetic of vgx_pick for ONE triangle, ONE box and ONE key: host + device.
// The kernels of vgx_pick.hip run it one mesh / one triangle per lane; libvgx_hosttest.so (vgx_hosttest.cpp: vgxt_pick) runs the same
// functions mesh after mesh and triangle after triangle so that the CPU suite pins the arithmetic without a GPU.
//
// The specification is in include/vgx.h (vgx_pick). The build compiles with -ffp-contract=off on both sides: nothing may contract the
// binary64 expressions below into FMAs, or host and device would round differently.
#ifndef VGX_PICK_H
#define VGX_PICK_H

#include "vgx_lane.h"
#include "vgx_raster.h" // vgx_pick_frame (below) wraps the raster's coverage and state functions

#define VGX_PICK_NONE 0xFFFFFFFFu

// ---- the closed box test, binary32 compares: false with a NaN on either side ---------------------------------------------
VGX_HD bool vgx_pick_in_box(float px, float py, float minx, float miny, float maxx, float maxy)
{
	return px >= minx && px <= maxx && py >= miny && py <= maxy;
}

// ---- the triangles of a mesh: a mesh of kind VGX_MESH_CONTOURS holds edge pairs and is never hit ------------------------------
VGX_HD uint32_t vgx_pick_mesh_triangles(const vgx_mesh& me) { return (me.subpath_kind >> 28) == VGX_MESH_CONTOURS ? 0u : me.num_indices / 3u; }

// ---- point in triangle -------------------------------------------------------------------------------------------------
// The triangle's own box first (cheap, and what makes the mesh-box prefilter exact), then the signs of the three edge expressions
// against the sign of the area, in binary64. A NaN vertex passes or fails the box test depending on which side of min / max it sits,
// and it does not matter: it makes A NaN and the answer "no hit" either way.
VGX_HD bool vgx_pick_tri(V2 a, V2 b, V2 c, float px, float py)
{
	const float lox = a.x < b.x ? (a.x < c.x ? a.x : c.x) : (b.x < c.x ? b.x : c.x);
	const float hix = a.x > b.x ? (a.x > c.x ? a.x : c.x) : (b.x > c.x ? b.x : c.x);
	const float loy = a.y < b.y ? (a.y < c.y ? a.y : c.y) : (b.y < c.y ? b.y : c.y);
	const float hiy = a.y > b.y ? (a.y > c.y ? a.y : c.y) : (b.y > c.y ? b.y : c.y);
	if (!vgx_pick_in_box(px, py, lox, loy, hix, hiy)) { return false; }
	const double ax = a.x, ay = a.y, bx = b.x, by = b.y, cx = c.x, cy = c.y, x = px, y = py;
	const double A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
	const double e0 = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
	const double e1 = (cx - bx) * (y - by) - (cy - by) * (x - bx);
	const double e2 = (ax - cx) * (y - cy) - (ay - cy) * (x - cx);
	if (A > 0.0) { return e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0; }
	if (A < 0.0) { return e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0; }
	return false; // A == 0 or NaN
}

// ---- the key: painter's order as one integer -----------------------------------------------------------------------------
// ((mesh + 1) << 32) | triangle, 0 = no hit: the maximum over all hit triangles is the topmost mesh's last triangle.
// mesh < 2^32 - 2 (vgx_pick refuses larger tables), triangle < 2^32 / 3.
VGX_HD uint64_t vgx_pick_key(uint32_t mesh, uint32_t triangle) { return (((uint64_t)mesh + 1u) << 32) | (uint64_t)triangle; }

VGX_HD vgx_pick_hit vgx_pick_decode(uint64_t key, const vgx_mesh* meshes)
{
	vgx_pick_hit h;
	if (key == 0) {
		h.mesh = VGX_PICK_NONE; h.triangle = VGX_PICK_NONE; h.draw = VGX_PICK_NONE; h.subpath_kind = VGX_PICK_NONE;
		return h;
	}
	h.mesh = (uint32_t)(key >> 32) - 1u;
	h.triangle = (uint32_t)key;
	h.draw = meshes[h.mesh].draw;
	h.subpath_kind = meshes[h.mesh].subpath_kind;
	return h;
}

// Triangle t of a mesh: its three indices, and whether it takes part at all (every index inside the mesh's own vertex range).
VGX_HD bool vgx_pick_tri_valid(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t numVertices)
{
	return i0 < numVertices && i1 < numVertices && i2 < numVertices;
}

// VGX_PICK_SKIP_TRANSPARENT: a vertex of alpha 0 (the outer ring of an AA fringe)
VGX_HD bool vgx_pick_tri_transparent(uint32_t c0, uint32_t c1, uint32_t c2) { return (c0 >> 24) == 0 || (c1 >> 24) == 0 || (c2 >> 24) == 0; }

// ---- vgx_pick_frame: what is under the point in the IMAGE of vgx_raster_concave (include/vgx.h) ------------------------------------
// Nothing of the arithmetic is restated here: coverage is vgx_raster.h's (vgx_raster_setup / _cover for a triangle, vgx_raster_contour_*
// for a contour mesh), the state is vgx_raster_draw_type and vgx_raster_stamp_pass. What is added is the point, the state of a mesh under
// its draw in FRAME pixels (vgx_raster_mesh_state is relative to a target and depends on a level), and the hit decision.

// The point of a query: its binary64 coordinates and the frame pixel it lies in. false: the hit is "none"
// (|px| < 2^31, so the floor fits an int32 and the 64-bit compares of the scissor rule are compares of small numbers)
VGX_HD bool vgx_pickf_point(float x, float y, double* px, double* py, int32_t* X, int32_t* Y)
{
	*px = (double)x; *py = (double)y;
	if (!(fabs(*px) < 2147483648.0) || !(fabs(*py) < 2147483648.0)) { *X = 0; *Y = 0; return false; }
	*X = (int32_t)(int64_t)floor(*px); *Y = (int32_t)(int64_t)floor(*py);
	return true;
}

// What vgx_pick_frame and vgx_pick_commands stage of a query in LDS: its point, and in bit 31 of its flags whether it takes part -- a
// point, and `wellFormed` by the call's own rule. The records that extend it (24 and 32 bytes) stay apart: DESIGN.md has the LDS figures
#define VGX_PICK_STAGED_VALID 0x80000000u
struct VgxPickStagedPoint { float x, y; int32_t X, Y; };
VGX_HD uint32_t vgx_pick_stage_point(float x, float y, uint32_t flags, bool wellFormed, VgxPickStagedPoint* p)
{
	double px, py;
	p->x = x; p->y = y;
	const bool point = vgx_pickf_point(x, y, &px, &py, &p->X, &p->Y);
	return (flags & ~VGX_PICK_STAGED_VALID) | (point && wellFormed ? VGX_PICK_STAGED_VALID : 0u);
}

// Mode (VGX_RF_PLAIN / IN / OUT / STAMP), f, n of a mesh under its draw, its element count (triangles, or edges of a contour mesh; 0: the
// mesh can cover nothing) and its draw's scissor as frame pixels [rect[0], rect[2]) x [rect[1], rect[3]). me.draw < num_draws is the caller's check
struct VgxPickfMesh { uint32_t mode, f, n, elems; uint32_t rect[4]; }; // 32 bytes
VGX_HD void vgx_pickf_mesh_state(const vgx_mesh& me, uint32_t stateKey, const vgx_draw_state& ds, VgxPickfMesh* st)
{
	st->f = 0u; st->n = 0u;
	if (vgx_raster_draw_type(stateKey) == 3u) {
		st->mode = VGX_RF_STAMP; st->f = me.draw;
	} else if (ds.clip_first_draw == VGX_RASTER_STAMP_NONE || ds.clip_num_draws == 0u) {
		st->mode = VGX_RF_PLAIN;
	} else {
		st->mode = ds.clip_rule == 0u ? VGX_RF_IN : VGX_RF_OUT;
		st->f = ds.clip_first_draw; st->n = ds.clip_num_draws;
	}
	st->elems = vgx_raster_mesh_elements(me);
	if (vgx_raster_kind_is_contours(me.subpath_kind) && me.num_vertices == 0u) { st->elems = 0u; } // a mesh with no vertices does nothing
	st->rect[0] = ds.scissor[0]; st->rect[1] = ds.scissor[1];
	st->rect[2] = (uint32_t)ds.scissor[0] + ds.scissor[2]; st->rect[3] = (uint32_t)ds.scissor[1] + ds.scissor[3];
}

// x <= X < x + w && y <= Y < y + h in 64-bit integers
VGX_HD bool vgx_pickf_in_scissor(const uint32_t* rect, int32_t X, int32_t Y)
{
	return (int64_t)rect[0] <= (int64_t)X && (int64_t)X < (int64_t)rect[2] && (int64_t)rect[1] <= (int64_t)Y && (int64_t)Y < (int64_t)rect[3];
}

// the closed box of a mesh (its entry of mesh_bounds), binary64 compares: false with a NaN bound
VGX_HD bool vgx_pickf_in_box(const float* box, double px, double py)
{
	return px >= (double)box[0] && px <= (double)box[2] && py >= (double)box[1] && py <= (double)box[3];
}

// a triangle covers the point: the raster's rule (binary64 box, canonical edge values, tie rule, S > 0); no colour is looked at
VGX_HD bool vgx_pickf_tri(V2 a, V2 b, V2 c, double px, double py)
{
	VgxRasterTri T;
	double E[3], S;
	return vgx_raster_setup(a, b, c, 0u, 0u, 0u, &T) && vgx_raster_cover(T, px, py, E, &S);
}

// what the directed edge u -> v of a contour mesh adds to W at the point
VGX_HD int32_t vgx_pickf_edge(V2 u, V2 v, double px, double py)
{
	VgxRasterTri T;
	return vgx_raster_contour_edge(u, v, &T) ? vgx_raster_contour_winding(T, px, py) : 0;
}

// VGX_PICK_SKIP_TRANSPARENT plays no part for a clip mesh: stamping is the image's, not the query's
VGX_HD bool vgx_pickf_skips(uint32_t mode, uint32_t queryFlags) { return mode != VGX_RF_STAMP && (queryFlags & VGX_PICK_SKIP_TRANSPARENT) != 0u; }

// Mesh m of state (mode, f, n), covered at the point under the query's flags, with the stamp S the meshes below it left: a hit?
VGX_HD bool vgx_pickf_hit(uint32_t mode, uint32_t f, uint32_t n, uint32_t S, uint64_t m, uint32_t queryMeshEnd)
{
	if (mode == VGX_RF_STAMP || m >= (uint64_t)queryMeshEnd) { return false; }
	return mode == VGX_RF_PLAIN || vgx_raster_stamp_pass(S, f, n, mode == VGX_RF_IN ? 0u : 1u);
}

VGX_HD vgx_pick_hit vgx_pickf_record(uint32_t mesh, uint32_t triangle, const vgx_mesh* meshes)
{
	vgx_pick_hit h;
	h.mesh = mesh; h.triangle = triangle;
	h.draw = mesh == VGX_PICK_NONE ? VGX_PICK_NONE : meshes[mesh].draw;
	h.subpath_kind = mesh == VGX_PICK_NONE ? VGX_PICK_NONE : meshes[mesh].subpath_kind;
	return h;
}

// The argument check of vgx_pick_frame and vgxt_pick_frame (host only): the union of vgx_pick's and vgx_raster_frame's. The first
// failing check of this order decides
static inline int vgx_pickf_check_args(const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_raster_draws* state, const vgx_pick_query* queries,
                                       uint32_t nqueries, const vgx_pick_hit* hits, const uint32_t* status)
{
	if (!frame || !state || (nqueries && (!queries || !hits))) { return VGX_E_INVALID_ARG; }
	if (state->reserved != 0u || (state->num_draws && (!state->draws || !state->draw_state))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)state->draws & 3u) || ((uintptr_t)state->draw_state & 3u)) { return VGX_E_INVALID_ARG; }
	if (frame->num_meshes && (!frame->pos || !frame->color || !frame->idx || !frame->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)queries & 15u) || ((uintptr_t)hits & 15u) || ((uintptr_t)mesh_bounds & 15u) || ((uintptr_t)status & 3u) || ((uintptr_t)frame->pos & 7u)
		|| ((uintptr_t)frame->color & 3u) || ((uintptr_t)frame->idx & 1u) || ((uintptr_t)frame->meshes & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (nqueries > VGX_PICK_MAX_QUERIES || frame->num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	return VGX_OK;
}

#endif
