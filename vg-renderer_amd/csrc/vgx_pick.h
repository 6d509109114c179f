// vgx_pick.h -- the arithmetic of vgx_pick for ONE triangle, ONE box and ONE key: host + device.
// The kernels of vgx_pick.hip run it one mesh / one triangle per lane; libvgx_hosttest.so (vgx_hosttest.cpp: vgxt_pick) runs the same
// functions mesh after mesh and triangle after triangle so that the CPU suite pins the arithmetic without a GPU.
//
// The specification is in include/vgx.h (vgx_pick). The build compiles with -ffp-contract=off on both sides: nothing may contract the
// binary64 expressions below into FMAs, or host and device would round differently.
#ifndef VGX_PICK_H
#define VGX_PICK_H

#include "vgx_lane.h"

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

#endif
