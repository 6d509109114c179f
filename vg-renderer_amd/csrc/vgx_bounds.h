// vgx_bounds.h -- the arithmetic of vgx_mesh_bounds and vgx_cache_cull for ONE value, ONE box and ONE instance: host + device.
// The kernels of vgx_bounds.hip run it one vertex / one instance per lane; libvgx_hosttest.so (vgx_hosttest.cpp) runs the same functions
// mesh after mesh and instance after instance so that the CPU suite pins the arithmetic without a GPU.
//
// Why a box of four corners is enough (include/vgx.h, vgx_cache_cull): vgx_cache_submit moves every cached vertex through v2xform,
// (m0*x + m2*y) + m4 in binary32 without FMA. Each operation in it is a monotone function of x and of y (rounding is monotone), so
// the extremes over a box of (x, y) are taken at its corners: the min / max of the four transformed corners of a mesh range's local
// box, computed with the same function, contains every submitted vertex exactly. No margin, no tolerance.
#ifndef VGX_BOUNDS_H
#define VGX_BOUNDS_H

#include "vgx_lane.h"

struct VgxBox { float minx, miny, maxx, maxy; };

// ---- float <-> order-preserving uint32 -------------------------------------------------------------------------------
// a < b as floats  <=>  vgx_ord_from_float(a) < vgx_ord_from_float(b) as unsigned integers (negatives: every bit flipped; others:
// the sign bit set). -0 maps directly below +0. Integer min / max of these images are what atomicMin / atomicMax combine: order
// independent and bitwise reproducible.
VGX_HD uint32_t vgx_ord_from_float(float f)
{
	union { float f; uint32_t u; } c; c.f = f;
	return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
VGX_HD float vgx_float_from_ord(uint32_t o)
{
	union { float f; uint32_t u; } c;
	c.u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
	return c.f;
}
#define VGX_ORD_POS_INF 0xFF800000u // vgx_ord_from_float(+inf): where a minimum starts
#define VGX_ORD_NEG_INF 0x007FFFFFu // vgx_ord_from_float(-inf): where a maximum starts

// ---- boxes -----------------------------------------------------------------------------------------------------------
VGX_HD VgxBox vgx_box_empty()
{
	union { float f; uint32_t u; } p, n; p.u = 0x7F800000u; n.u = 0xFF800000u;
	VgxBox b; b.minx = p.f; b.miny = p.f; b.maxx = n.f; b.maxy = n.f;
	return b;
}
VGX_HD bool vgx_box_is_empty(VgxBox b) { return b.minx > b.maxx || b.miny > b.maxy; }
VGX_HD VgxBox vgx_box_load(const float* p) { VgxBox b; b.minx = p[0]; b.miny = p[1]; b.maxx = p[2]; b.maxy = p[3]; return b; }
VGX_HD void vgx_box_store(float* p, VgxBox b) { p[0] = b.minx; p[1] = b.miny; p[2] = b.maxx; p[3] = b.maxy; }

// min / max that hand a NaN on, whichever side it is on (a plain `a < b ? a : b` drops it on one side)
VGX_HD float vgx_min_nan(float a, float b) { return (a < b || a != a) ? a : b; }
VGX_HD float vgx_max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

VGX_HD VgxBox vgx_box_union(VgxBox a, VgxBox b)
{
	VgxBox r;
	r.minx = vgx_min_nan(a.minx, b.minx); r.miny = vgx_min_nan(a.miny, b.miny);
	r.maxx = vgx_max_nan(a.maxx, b.maxx); r.maxy = vgx_max_nan(a.maxy, b.maxy);
	return r;
}

// the union of mesh_bounds[first .. first + n): what ONE lane does for a short range (the kernel lets the wave do long ones)
VGX_HD VgxBox vgx_box_union_range(const float* meshBounds, uint64_t first, uint32_t n)
{
	VgxBox L = vgx_box_empty();
	for (uint32_t k = 0; k < n; ++k) { L = vgx_box_union(L, vgx_box_load(meshBounds + 4 * (first + k))); }
	return L;
}

// The device box of a local box: min / max over its four corners through the function vgx_cache_submit's copy kernel calls.
VGX_HD VgxBox vgx_box_transform(VgxBox L, const float* mtx)
{
	const V2 a = v2xform(v2(L.minx, L.miny), mtx), b = v2xform(v2(L.maxx, L.miny), mtx);
	const V2 c = v2xform(v2(L.maxx, L.maxy), mtx), d = v2xform(v2(L.minx, L.maxy), mtx);
	VgxBox B;
	B.minx = vgx_min_nan(vgx_min_nan(a.x, b.x), vgx_min_nan(c.x, d.x)); B.miny = vgx_min_nan(vgx_min_nan(a.y, b.y), vgx_min_nan(c.y, d.y));
	B.maxx = vgx_max_nan(vgx_max_nan(a.x, b.x), vgx_max_nan(c.x, d.x)); B.maxy = vgx_max_nan(vgx_max_nan(a.y, b.y), vgx_max_nan(c.y, d.y));
	return B;
}

// ---- the cull rule ---------------------------------------------------------------------------------------------------
// view = x0, y0, x1, y1, closed. An empty view (x0 > x1 or y0 > y1: the reference's empty scissor, vg.cpp:4543-4567) culls everything;
// else a box is culled iff it lies wholly on one side. Every comparison with a NaN is false: such a box is kept.
VGX_HD bool vgx_box_culled(VgxBox B, const float* view)
{
	const float x0 = view[0], y0 = view[1], x1 = view[2], y1 = view[3];
	if (x0 > x1 || y0 > y1) { return true; }
	return B.maxx < x0 || B.minx > x1 || B.maxy < y0 || B.miny > y1;
}

// Is the instance's range inside the cache and its view inside the table?
VGX_HD bool vgx_cull_valid(const vgx_cache_instance& in, uint64_t cacheMeshes, uint32_t view, uint32_t nviews)
{
	return in.first_mesh <= cacheMeshes && (uint64_t)in.num_meshes <= cacheMeshes - in.first_mesh && view < nviews;
}

// One VALID instance whose local box L is known: its device box, and whether it is kept.
VGX_HD bool vgx_cull_decide(VgxBox L, const float* mtx, const float* view, VgxBox* B)
{
	if (vgx_box_is_empty(L)) { *B = vgx_box_empty(); return false; } // an empty range, or nothing but 0-vertex meshes: draws nothing
	*B = vgx_box_transform(L, mtx);
	return !vgx_box_culled(*B, view);
}

#endif
