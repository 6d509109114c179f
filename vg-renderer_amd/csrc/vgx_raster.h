// vgx_raster.h -- the arithmetic of vgx_raster for ONE triangle, ONE sample and ONE pixel: host + device.
// The tile kernel of vgx_raster.hip runs it one triangle per lane (setup) and one pixel per lane (coverage, colour, blend);
// libvgx_hosttest.so (vgx_hosttest.cpp: vgxt_raster) runs the same functions mesh after mesh, triangle after triangle and pixel after
// pixel so that the CPU suite pins the arithmetic without a GPU.
//
// The specification is in include/vgx.h (vgx_raster). The build compiles with -ffp-contract=off on both sides: nothing may contract the
// binary64 expressions below into FMAs, or host and device would round differently. Division is the correctly rounded one.
#ifndef VGX_RASTER_H
#define VGX_RASTER_H

#include "vgx_lane.h"
#include <math.h>

#define VGX_RASTER_TILE 16 // pixels per tile side: one workgroup of 256 lanes, one pixel per lane

// ---- the setup record of a triangle: what a pixel needs, computed once ---------------------------------------------------
// Edge k (0: a->b, 1: b->c, 2: c->a) in its canonical form: lo = the smaller endpoint by (x, then y), d = hi - lo in binary64.
// g = d.x * (py - lo.y) - d.y * (px - lo.x) is the same number for both triangles that share the edge.
struct VgxRasterEdge { float lox, loy; double dx, dy; };
#define VGX_RT_NEG(k)  (1u << (k))        // E_k = -g_k (orientation and direction together)
#define VGX_RT_ZERO(k) (8u << (k))        // u == v bit for bit: E_k = 0
#define VGX_RT_TIE(k)  (64u << (k))       // the oriented edge takes E_k == 0
#define VGX_RT_FLAT(ch) (512u << (ch))    // channel ch (0 = R .. 3 = A) is the same on all three vertices
struct VgxRasterTri
{
	float minx, miny, maxx, maxy; // the triangle's own box
	VgxRasterEdge e[3];
	uint32_t col[3];              // ca, cb, cc
	uint32_t flags;               // VGX_RT_*
};                                // 104 bytes

VGX_HD bool vgx_raster_bits_equal(V2 u, V2 v)
{
	union { float f; uint32_t u; } a, b, c, d;
	a.f = u.x; b.f = v.x; c.f = u.y; d.f = v.y;
	return a.u == b.u && c.u == d.u;
}

// the directed edge u->v of a triangle of orientation s (+1 / -1)
VGX_HD uint32_t vgx_raster_edge(V2 u, V2 v, bool positive, int k, VgxRasterEdge* e)
{
	const bool uIsLo = u.x < v.x || (u.x == v.x && u.y <= v.y);
	const V2 lo = uIsLo ? u : v, hi = uIsLo ? v : u;
	e->lox = lo.x; e->loy = lo.y;
	e->dx = (double)hi.x - (double)lo.x; e->dy = (double)hi.y - (double)lo.y;
	uint32_t f = 0;
	if (positive != uIsLo) { f |= VGX_RT_NEG(k); }
	if (vgx_raster_bits_equal(u, v)) { f |= VGX_RT_ZERO(k); }
	// oriented direction (dx, dy) = s * (v - u): the tie goes to dy > 0, or dy == 0 && dx < 0
	const bool tie = positive ? (v.y > u.y || (v.y == u.y && v.x < u.x)) : (v.y < u.y || (v.y == u.y && v.x > u.x));
	if (tie) { f |= VGX_RT_TIE(k); }
	return f;
}

// false: the triangle covers nothing (A == 0 or NaN)
VGX_HD bool vgx_raster_setup(V2 a, V2 b, V2 c, uint32_t ca, uint32_t cb, uint32_t cc, VgxRasterTri* T)
{
	const double ax = a.x, ay = a.y, bx = b.x, by = b.y, cx = c.x, cy = c.y;
	const double A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
	if (!(A > 0.0 || A < 0.0)) { return false; }
	const bool positive = A > 0.0;
	T->minx = a.x < b.x ? (a.x < c.x ? a.x : c.x) : (b.x < c.x ? b.x : c.x);
	T->maxx = a.x > b.x ? (a.x > c.x ? a.x : c.x) : (b.x > c.x ? b.x : c.x);
	T->miny = a.y < b.y ? (a.y < c.y ? a.y : c.y) : (b.y < c.y ? b.y : c.y);
	T->maxy = a.y > b.y ? (a.y > c.y ? a.y : c.y) : (b.y > c.y ? b.y : c.y);
	uint32_t f = vgx_raster_edge(a, b, positive, 0, &T->e[0]) | vgx_raster_edge(b, c, positive, 1, &T->e[1]) | vgx_raster_edge(c, a, positive, 2, &T->e[2]);
	for (int ch = 0; ch < 4; ++ch) {
		const uint32_t x = (ca >> (8 * ch)) & 255u;
		if (x == ((cb >> (8 * ch)) & 255u) && x == ((cc >> (8 * ch)) & 255u)) { f |= VGX_RT_FLAT(ch); }
	}
	T->col[0] = ca; T->col[1] = cb; T->col[2] = cc;
	T->flags = f;
	return true;
}

VGX_HD double vgx_raster_edge_value(const VgxRasterEdge& e, uint32_t flags, int k, double px, double py)
{
	const double g = e.dx * (py - (double)e.loy) - e.dy * (px - (double)e.lox);
	if (flags & VGX_RT_ZERO(k)) { return 0.0; }
	return (flags & VGX_RT_NEG(k)) ? -g : g;
}

VGX_HD bool vgx_raster_accepts(double E, uint32_t flags, int k) { return E > 0.0 || (E == 0.0 && (flags & VGX_RT_TIE(k)) != 0); }

// Coverage of the sample (px, py); E[0..2] and S are what the colour needs
VGX_HD bool vgx_raster_cover(const VgxRasterTri& T, double px, double py, double* E, double* S)
{
	if (!(px >= (double)T.minx && px <= (double)T.maxx && py >= (double)T.miny && py <= (double)T.maxy)) { return false; }
	E[0] = vgx_raster_edge_value(T.e[0], T.flags, 0, px, py);
	if (!vgx_raster_accepts(E[0], T.flags, 0)) { return false; }
	E[1] = vgx_raster_edge_value(T.e[1], T.flags, 1, px, py);
	if (!vgx_raster_accepts(E[1], T.flags, 1)) { return false; }
	E[2] = vgx_raster_edge_value(T.e[2], T.flags, 2, px, py);
	if (!vgx_raster_accepts(E[2], T.flags, 2)) { return false; }
	*S = (E[0] + E[1]) + E[2];
	return *S > 0.0;
}

// One channel at a covered sample. A channel that is the same on all three vertices IS that value: the rule below would give
// v = x * (1 + e), |e| < 2^-49 (three products, two sums, one sum for S, one division, each within 2^-53), so |v - x| < 2^-41 and
// (uint32)(v + 0.5) = x; the division is skipped, the result is the rule's.
VGX_HD uint32_t vgx_raster_channel(const VgxRasterTri& T, int ch, const double* E, double S)
{
	const uint32_t xa = (T.col[0] >> (8 * ch)) & 255u;
	if (T.flags & VGX_RT_FLAT(ch)) { return xa; }
	const uint32_t xb = (T.col[1] >> (8 * ch)) & 255u, xc = (T.col[2] >> (8 * ch)) & 255u;
	const double v = ((E[1] * (double)xa + E[2] * (double)xb) + E[0] * (double)xc) / S;
	const uint32_t q = (uint32_t)(v + 0.5);
	return q < 255u ? q : 255u;
}

VGX_HD uint32_t vgx_raster_div255(uint32_t x) { return (x + 127u) / 255u; }

// BLEND_FUNC_SEPARATE(SRC_ALPHA, INV_SRC_ALPHA, ONE, INV_SRC_ALPHA) on UNORM8 in integers: src over dst, both 0xAABBGGRR
VGX_HD uint32_t vgx_raster_blend(uint32_t dst, uint32_t r, uint32_t g, uint32_t b, uint32_t a)
{
	const uint32_t ia = 255u - a;
	const uint32_t dr = dst & 255u, dg = (dst >> 8) & 255u, db = (dst >> 16) & 255u, da = dst >> 24;
	return vgx_raster_div255(r * a + dr * ia) | (vgx_raster_div255(g * a + dg * ia) << 8) | (vgx_raster_div255(b * a + db * ia) << 16)
	     | (vgx_raster_div255(255u * a + da * ia) << 24);
}

// The triangle on the pixel whose sample is (px, py): the pixel's new value
VGX_HD uint32_t vgx_raster_pixel(const VgxRasterTri& T, double px, double py, uint32_t dst)
{
	double E[3], S;
	if (!vgx_raster_cover(T, px, py, E, &S)) { return dst; }
	const uint32_t a = vgx_raster_channel(T, 3, E, S);
	if (a == 0u) { return dst; }
	return vgx_raster_blend(dst, vgx_raster_channel(T, 0, E, S), vgx_raster_channel(T, 1, E, S), vgx_raster_channel(T, 2, E, S), a);
}

// ---- which pixels can a box reach? --------------------------------------------------------------------------------------
// Pixel i samples at origin + i + 0.5. The pixels of [c0, c1) whose sample MAY lie in [lo, hi], as an inclusive range: a superset
// (rounding is monotone, floor / ceil take the outer integer), which is all a prefilter needs -- the rule starts with the triangle's
// own box. A NaN bound compares false and bounds nothing. false: none.
VGX_HD bool vgx_raster_span(float lo, float hi, int32_t origin, uint32_t c0, uint32_t c1, uint32_t* i0, uint32_t* i1)
{
	const double base = (double)origin + 0.5;
	const double dlo = (double)lo - base, dhi = (double)hi - base;
	double fa = (double)c0, fb = (double)c1 - 1.0;
	if (dlo > fa) { fa = floor(dlo); }
	if (dhi < fb) { fb = ceil(dhi); }
	if (!(fa <= fb)) { return false; }
	*i0 = (uint32_t)fa; *i1 = (uint32_t)fb;
	return true;
}

// the kinds that carry UVs: vgx_raster and vgx_raster_frame skip them, the wider calls draw them
VGX_HD bool vgx_raster_kind_has_uv(uint32_t subpathKind)
{
	const uint32_t k = subpathKind >> 28;
	return k == VGX_MESH_TEXT || k == VGX_MESH_TRILIST;
}

// the kind that holds directed edges, not triangles: drawn by vgx_raster_concave, skipped whole by every call below it
VGX_HD bool vgx_raster_kind_is_contours(uint32_t subpathKind) { return (subpathKind >> 28) == VGX_MESH_CONTOURS; }

// ---- the calls: vgx_raster < vgx_raster_frame < vgx_raster_textured < vgx_raster_painted < vgx_raster_concave (include/vgx.h) -------
// One loop on the host and one kernel family on the device serve the frame-level calls; what differs is the level: which kinds are
// drawn, which meshes are sampled or painted, and which tables are read (vgx_raster_mesh_state below). VGX_RL_PLAIN is vgx_raster, for
// the argument check and the kinds alone
enum { VGX_RL_PLAIN = 0, VGX_RL_FRAME = 1, VGX_RL_TEXTURED = 2, VGX_RL_PAINTED = 3, VGX_RL_CONCAVE = 4 };

// elements of a mesh: triangles, or the edges of a contour mesh
VGX_HD uint32_t vgx_raster_mesh_elements(const vgx_mesh& me) { return vgx_raster_kind_is_contours(me.subpath_kind) ? me.num_indices / 2u : me.num_indices / 3u; }

// Bin entries of a mesh: the tiles its box can reach inside the scissor (a rectangle of tiles). Below VGX_RL_TEXTURED a mesh of kind
// TEXT / TRILIST has none, below VGX_RL_CONCAVE a mesh of kind CONTOURS has none
struct VgxRasterRect { uint32_t tx0, ty0, tx1, ty1; }; // inclusive
VGX_HD bool vgx_raster_mesh_tiles(const vgx_mesh& me, const float* box, int32_t x0, int32_t y0, const uint32_t* scissor, int level, VgxRasterRect* r)
{
	if (level < VGX_RL_TEXTURED && vgx_raster_kind_has_uv(me.subpath_kind)) { return false; }
	if (vgx_raster_kind_is_contours(me.subpath_kind) ? (level < VGX_RL_CONCAVE || me.num_vertices == 0u || me.num_indices < 2u) : me.num_indices < 3u) { return false; }
	uint32_t i0, i1, j0, j1;
	if (!vgx_raster_span(box[0], box[2], x0, scissor[0], scissor[2], &i0, &i1) || !vgx_raster_span(box[1], box[3], y0, scissor[1], scissor[3], &j0, &j1)) { return false; }
	r->tx0 = i0 / VGX_RASTER_TILE; r->tx1 = i1 / VGX_RASTER_TILE; r->ty0 = j0 / VGX_RASTER_TILE; r->ty1 = j1 / VGX_RASTER_TILE;
	return true;
}

// ---- per-draw scissors and clip regions (every level) ---------------------------------------------------------------------------
#define VGX_RASTER_STAMP_NONE 0xFFFFFFFFu // S of a pixel no clip mesh has touched; clip_first_draw of a draw without a region
// what a mesh does with the stamp
enum { VGX_RF_PLAIN = 0, VGX_RF_IN = 1, VGX_RF_OUT = 2, VGX_RF_STAMP = 3, VGX_RF_NOTHING = 4, VGX_RF_INVALID = 5 };
// what a mesh is drawn with, beside the handle (bits 0 .. 15) in VgxRasterMeshState::pad and beside slot and mode in a tile record
#define VGX_RT_SAMPLED  0x10000u // kind TEXT / TRILIST under a draw of type 0: the handle names an image
#define VGX_RT_GRADIENT 0x20000u // a draw of type 1: the handle names a gradient
#define VGX_RT_PATTERN  0x40000u // a draw of type 2: the handle names a pattern
#define VGX_RT_PAINTED  (VGX_RT_GRADIENT | VGX_RT_PATTERN)
#define VGX_RT_CONTOUR  0x80000u // kind CONTOURS at VGX_RL_CONCAVE: the mesh's elements are edges; beside the paint flags, never beside SAMPLED
#define VGX_RT_FLUSH    0x100000u // in a tile record only: the element behind a contour mesh's last edge
// Per mesh of the range (context scratch of the frame-level calls only). rect = the target's scissor cut by the draw's, in image
// pixels, half open; f, n = the region of a tested mesh, f = the mesh's draw for VGX_RF_STAMP
struct VgxRasterMeshState { uint32_t mode, f, n, pad; uint32_t rect[4]; }; // 32 bytes

VGX_HD uint32_t vgx_raster_draw_type(uint32_t stateKey) { return (stateKey >> 16) & 0xFu; } // 3 = Clip

// Frame pixels [s, s + w) as pixels of the image (pixel i is frame pixel origin + i) inside [c0, c1): 64-bit integers. false: none
VGX_HD bool vgx_raster_draw_span(uint16_t s, uint16_t w, int32_t origin, uint32_t c0, uint32_t c1, uint32_t* i0, uint32_t* i1)
{
	int64_t a = (int64_t)s - (int64_t)origin, b = a + (int64_t)w;
	if (a < (int64_t)c0) { a = (int64_t)c0; }
	if (b > (int64_t)c1) { b = (int64_t)c1; }
	if (a >= b) { return false; }
	*i0 = (uint32_t)a; *i1 = (uint32_t)b;
	return true;
}

VGX_HD bool vgx_raster_stamp_pass(uint32_t S, uint32_t f, uint32_t n, uint32_t rule)
{
	return (S != VGX_RASTER_STAMP_NONE && S >= f && S - f < n) == (rule == 0u);
}

// The triangle of a mesh of state (mode, f, n) on the pixel whose sample is (px, py) and lies inside the mesh's rect: the pixel's
// new value; *S is the pixel's stamp
VGX_HD uint32_t vgx_raster_frame_pixel(const VgxRasterTri& T, uint32_t mode, uint32_t f, uint32_t n, double px, double py, uint32_t* S, uint32_t dst)
{
	if (mode == VGX_RF_STAMP) {
		double E[3], sum;
		if (vgx_raster_cover(T, px, py, E, &sum)) { *S = f; }
		return dst;
	}
	if (mode != VGX_RF_PLAIN && !vgx_raster_stamp_pass(*S, f, n, mode == VGX_RF_IN ? 0u : 1u)) { return dst; }
	return vgx_raster_pixel(T, px, py, dst);
}

// ---- from the textured level on: text and user meshes sampled from an RGBA8 image (include/vgx.h) --------------------------------
// Every kind is drawn; a mesh of kind TEXT / TRILIST under a draw of type 0 is sampled, the image = the low 16 bits of the state key
VGX_HD bool vgx_raster_mesh_sampled(uint32_t subpathKind, uint32_t stateKey) { return vgx_raster_kind_has_uv(subpathKind) && vgx_raster_draw_type(stateKey) == 0u; }

VGX_HD bool vgx_raster_image_valid(const vgx_raster_image& im)
{
	return im.pixels != nullptr && ((uintptr_t)im.pixels & 3u) == 0u && im.width >= 1u && im.width <= 16384u && im.height >= 1u && im.height <= 16384u
	    && im.stride >= im.width;
}

// the UV of vertex v of the stream as two binary64 values: binary32 widened, or int16 / 32767
VGX_HD void vgx_raster_uv_widen(const void* uv, uint32_t uvBytes, uint64_t v, double* out)
{
	if (uvBytes == 8u) {
		const float* p = (const float*)uv + 2u * v;
		out[0] = (double)p[0]; out[1] = (double)p[1];
	} else {
		const int16_t* p = (const int16_t*)uv + 2u * v;
		out[0] = (double)p[0] / 32767.0; out[1] = (double)p[1] / 32767.0;
	}
}

// one UV component at a covered sample: the form of vgx_raster_channel
VGX_HD double vgx_raster_uv_at(double ua, double ub, double uc, const double* E, double S) { return ((E[1] * ua + E[2] * ub) + E[0] * uc) / S; }

// texel coordinate; false: the sample leaves the pixel alone
VGX_HD bool vgx_raster_texcoord(double u, uint32_t W, double* U)
{
	*U = u * (double)W;
	return fabs(*U) < 2147483648.0;
}

VGX_HD uint32_t vgx_raster_wrap(int64_t i, uint32_t W, bool clamp)
{
	if (clamp) { return i < 0 ? 0u : (i > (int64_t)W - 1 ? W - 1u : (uint32_t)i); }
	int64_t r = i % (int64_t)W;
	if (r < 0) { r += (int64_t)W; }
	return (uint32_t)r;
}

// the linear filter's index pair and weight of one axis
VGX_HD void vgx_raster_linear_axis(double U, uint32_t W, bool clamp, uint32_t* i0, uint32_t* i1, uint32_t* w)
{
	const int64_t T = (int64_t)floor((U - 0.5) * 256.0 + 0.5);
	const int64_t lo = T >> 8;
	*w = (uint32_t)(T & 255);
	*i0 = vgx_raster_wrap(lo, W, clamp); *i1 = vgx_raster_wrap(lo + 1, W, clamp);
}

VGX_HD uint32_t vgx_raster_bilinear(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, uint32_t wx, uint32_t wy)
{
	return (c00 * (256u - wx) * (256u - wy) + c10 * wx * (256u - wy) + c01 * (256u - wx) * wy + c11 * wx * wy + 32768u) >> 16;
}

// The texel of image `im` at the texel coordinates (U, V), both already in range. fetch(x, y), x < width, y < height, reads a texel
template <class Fetch>
VGX_HD uint32_t vgx_raster_sample(const vgx_raster_image& im, double U, double V, Fetch fetch)
{
	const bool cu = (im.flags & VGX_IMAGE_CLAMP_U) != 0u, cv = (im.flags & VGX_IMAGE_CLAMP_V) != 0u;
	if (im.flags & VGX_IMAGE_NEAREST) {
		return fetch(vgx_raster_wrap((int64_t)floor(U), im.width, cu), vgx_raster_wrap((int64_t)floor(V), im.height, cv));
	}
	uint32_t x0, x1, wx, y0, y1, wy;
	vgx_raster_linear_axis(U, im.width, cu, &x0, &x1, &wx);
	vgx_raster_linear_axis(V, im.height, cv, &y0, &y1, &wy);
	const uint32_t c00 = fetch(x0, y0), c10 = fetch(x1, y0), c01 = fetch(x0, y1), c11 = fetch(x1, y1);
	uint32_t r = 0;
	for (int ch = 0; ch < 4; ++ch) {
		const int sh = 8 * ch;
		r |= vgx_raster_bilinear((c00 >> sh) & 255u, (c10 >> sh) & 255u, (c01 >> sh) & 255u, (c11 >> sh) & 255u, wx, wy) << sh;
	}
	return r;
}

// The triangle of a SAMPLED mesh (mode is never VGX_RF_STAMP: its draw has type 0) with the vertex UVs uv[0 .. 5] = ua, va, ub, vb,
// uc, vc on the pixel whose sample is (px, py): the pixel's new value
template <class Fetch>
VGX_HD uint32_t vgx_raster_textured_pixel(const VgxRasterTri& T, const double* uv, const vgx_raster_image& im, uint32_t mode, uint32_t f, uint32_t n,
                                          double px, double py, uint32_t S, uint32_t dst, Fetch fetch)
{
	if (mode != VGX_RF_PLAIN && !vgx_raster_stamp_pass(S, f, n, mode == VGX_RF_IN ? 0u : 1u)) { return dst; }
	double E[3], sum, U, V;
	if (!vgx_raster_cover(T, px, py, E, &sum)) { return dst; }
	if (!vgx_raster_texcoord(vgx_raster_uv_at(uv[0], uv[2], uv[4], E, sum), im.width, &U)
	 || !vgx_raster_texcoord(vgx_raster_uv_at(uv[1], uv[3], uv[5], E, sum), im.height, &V)) { return dst; }
	const uint32_t tc = vgx_raster_sample(im, U, V, fetch);
	const uint32_t a = vgx_raster_div255(vgx_raster_channel(T, 3, E, sum) * (tc >> 24));
	if (a == 0u) { return dst; }
	return vgx_raster_blend(dst, vgx_raster_div255(vgx_raster_channel(T, 0, E, sum) * (tc & 255u)), vgx_raster_div255(vgx_raster_channel(T, 1, E, sum) * ((tc >> 8) & 255u)),
	                        vgx_raster_div255(vgx_raster_channel(T, 2, E, sum) * ((tc >> 16) & 255u)), a);
}

// ---- at the painted level: gradient and image-pattern paints (include/vgx.h) ------------------------------------------------------
// A mesh whose draw has type 1 (ColorGradient) or 2 (ImagePattern) is painted, whatever its kind: the handle in the low 16 bits of the
// state key indexes the table of that type
VGX_HD uint32_t vgx_raster_mesh_painted(uint32_t stateKey)
{
	const uint32_t type = vgx_raster_draw_type(stateKey);
	return type == 1u ? VGX_RT_GRADIENT : (type == 2u ? VGX_RT_PATTERN : 0u);
}

// What a pixel needs of a paint: 48 bytes. m = matrix[0], [1], [3], [4], [6], [7] of the vgx_paint; a gradient keeps its four params and
// its two ends as 8-bit channels (0xAABBGGRR), a pattern the record of its image
struct VgxRasterPaint
{
	float m[6];
	union {
		struct { float params[4]; uint32_t inner, outer; } g;
		vgx_raster_image im;
	};
};

// the paint coordinate of the sample (px, py): affine, so a function of the sample alone
VGX_HD void vgx_raster_paint_coord(const float* m, double px, double py, double* qx, double* qy)
{
	*qx = ((double)m[0] * px + (double)m[2] * py) + (double)m[4];
	*qy = ((double)m[1] * px + (double)m[3] * py) + (double)m[5];
}

// The square root of the rule: IEEE squareRoot. x86-64's sqrtsd is; the device's is shown to be by tests/native/exact_sqrt64_test.hip
VGX_HD double vgx_raster_sqrt(double x) { return sqrt(x); }

// fs_color_gradient.sc's sdroundrect and the feather ramp, clamped to [0, 1]; a NaN gives 0
VGX_HD double vgx_raster_gradient_t(const float* params, double qx, double qy)
{
	const double ex = (double)params[0], ey = (double)params[1], rad = (double)params[2], fe = (double)params[3];
	const double ax = fabs(qx) - (ex - rad);
	const double ay = fabs(qy) - (ey - rad);
	const double mx = ax > ay ? ax : ay;
	const double in = mx < 0.0 ? mx : 0.0;
	const double ox = ax > 0.0 ? ax : 0.0;
	const double oy = ay > 0.0 ? ay : 0.0;
	const double len = vgx_raster_sqrt(ox * ox + oy * oy);
	const double sd = (in + len) - rad;
	double t = (sd + fe * 0.5) / fe;
	t = t > 0.0 ? t : 0.0;
	t = t < 1.0 ? t : 1.0;
	return t;
}

// a gradient end's channel as 8 bits: what the decoder's c / 255.0f came from
VGX_HD uint32_t vgx_raster_q8(float c)
{
	const double x = (double)c * 255.0 + 0.5;
	if (!(x > 0.0)) { return 0u; }
	if (x >= 256.0) { return 255u; }
	return (uint32_t)x;
}
VGX_HD uint32_t vgx_raster_q8x4(const float* c) { return vgx_raster_q8(c[0]) | (vgx_raster_q8(c[1]) << 8) | (vgx_raster_q8(c[2]) << 16) | (vgx_raster_q8(c[3]) << 24); }

// GLSL mix of two 8-bit ends, rounded to 8 bits
VGX_HD uint32_t vgx_raster_mix8(uint32_t I, uint32_t O, double t)
{
	const double v = (double)I * (1.0 - t) + (double)O * t;
	const uint32_t g = (uint32_t)(v + 0.5);
	return g < 255u ? g : 255u;
}

// The compact record of paint p. `images` is read for a pattern only (its index is inside the table: the mesh state's check)
VGX_HD void vgx_raster_paint_record(const vgx_paint& p, const vgx_raster_image* images, VgxRasterPaint* r)
{
	r->m[0] = p.matrix[0]; r->m[1] = p.matrix[1]; r->m[2] = p.matrix[3]; r->m[3] = p.matrix[4]; r->m[4] = p.matrix[6]; r->m[5] = p.matrix[7];
	if (p.type == 1u) {
		for (int k = 0; k < 4; ++k) { r->g.params[k] = p.params[k]; }
		r->g.inner = vgx_raster_q8x4(p.inner_color); r->g.outer = vgx_raster_q8x4(p.outer_color);
	} else {
		r->im = images[p.image & 0xFFFFu];
	}
}

// The triangle of a mesh of a GRADIENT draw on the pixel whose sample is (px, py): fs_color_gradient.sc, mix(inner, outer, t) with the
// alpha times the vertex alpha; vertex RGB is not used
// ... from the vertex alpha on: what a covered sample of vertex alpha va becomes
VGX_HD uint32_t vgx_raster_gradient_shade(const VgxRasterPaint& P, uint32_t va, double px, double py, uint32_t dst)
{
	double qx, qy;
	if (va == 0u) { return dst; } // a == div255(g_A * 0) == 0
	vgx_raster_paint_coord(P.m, px, py, &qx, &qy);
	const double t = vgx_raster_gradient_t(P.g.params, qx, qy);
	const uint32_t a = vgx_raster_div255(vgx_raster_mix8(P.g.inner >> 24, P.g.outer >> 24, t) * va);
	if (a == 0u) { return dst; }
	return vgx_raster_blend(dst, vgx_raster_mix8(P.g.inner & 255u, P.g.outer & 255u, t), vgx_raster_mix8((P.g.inner >> 8) & 255u, (P.g.outer >> 8) & 255u, t),
	                        vgx_raster_mix8((P.g.inner >> 16) & 255u, (P.g.outer >> 16) & 255u, t), a);
}
VGX_HD uint32_t vgx_raster_gradient_pixel(const VgxRasterTri& T, const VgxRasterPaint& P, uint32_t mode, uint32_t f, uint32_t n, double px, double py, uint32_t S, uint32_t dst)
{
	if (mode != VGX_RF_PLAIN && !vgx_raster_stamp_pass(S, f, n, mode == VGX_RF_IN ? 0u : 1u)) { return dst; }
	double E[3], sum;
	if (!vgx_raster_cover(T, px, py, E, &sum)) { return dst; }
	return vgx_raster_gradient_shade(P, vgx_raster_channel(T, 3, E, sum), px, py, dst);
}

// The triangle of a mesh of an IMAGE PATTERN draw: fs_image_pattern.sc, the texel rule of vgx_raster_textured at (u, v) = the paint
// coordinate, modulated by the interpolated vertex colour (the pattern's tint). No UV of the stream is read
// ... at a covered sample; vc(ch) gives the vertex colour's channel ch there
template <class Fetch, class Channel>
VGX_HD uint32_t vgx_raster_pattern_shade(const VgxRasterPaint& P, double px, double py, uint32_t dst, Fetch fetch, Channel vc)
{
	double qx, qy, U, V;
	vgx_raster_paint_coord(P.m, px, py, &qx, &qy);
	if (!vgx_raster_texcoord(qx, P.im.width, &U) || !vgx_raster_texcoord(qy, P.im.height, &V)) { return dst; }
	const uint32_t tc = vgx_raster_sample(P.im, U, V, fetch);
	const uint32_t a = vgx_raster_div255(vc(3) * (tc >> 24));
	if (a == 0u) { return dst; }
	return vgx_raster_blend(dst, vgx_raster_div255(vc(0) * (tc & 255u)), vgx_raster_div255(vc(1) * ((tc >> 8) & 255u)), vgx_raster_div255(vc(2) * ((tc >> 16) & 255u)), a);
}
template <class Fetch>
VGX_HD uint32_t vgx_raster_pattern_pixel(const VgxRasterTri& T, const VgxRasterPaint& P, uint32_t mode, uint32_t f, uint32_t n, double px, double py, uint32_t S,
                                         uint32_t dst, Fetch fetch)
{
	if (mode != VGX_RF_PLAIN && !vgx_raster_stamp_pass(S, f, n, mode == VGX_RF_IN ? 0u : 1u)) { return dst; }
	double E[3], sum;
	if (!vgx_raster_cover(T, px, py, E, &sum)) { return dst; }
	return vgx_raster_pattern_shade(P, px, py, dst, fetch, [&](int ch) { return vgx_raster_channel(T, ch, E, sum); });
}

// ---- at the concave level: a mesh of kind VGX_MESH_CONTOURS is filled by winding number (include/vgx.h) ---------------------------
// The record of one directed edge u -> v lives in a VgxRasterTri: e[0] and the NEG / ZERO flags of edge 0 hold the canonical edge
// value of u -> v (vgx_raster_edge with positive = true), miny = u.y, maxy = v.y, minx = the smaller x. false: the edge adds 0 at
// every sample (horizontal, or a NaN in y)
VGX_HD bool vgx_raster_contour_edge(V2 u, V2 v, VgxRasterTri* T)
{
	if (!(u.y < v.y || v.y < u.y)) { return false; }
	T->flags = vgx_raster_edge(u, v, true, 0, &T->e[0]);
	T->minx = u.x < v.x ? u.x : v.x; T->miny = u.y; T->maxy = v.y;
	return true;
}

// what the edge adds to W at the sample (px, py)
VGX_HD int32_t vgx_raster_contour_winding(const VgxRasterTri& T, double px, double py)
{
	const double uy = (double)T.miny, vy = (double)T.maxy;
	const bool up = uy < py && py <= vy, dn = vy < py && py <= uy;
	if (!up && !dn) { return 0; }
	const double E = vgx_raster_edge_value(T.e[0], T.flags, 0, px, py);
	return up ? (E < 0.0 ? 1 : 0) : (E > 0.0 ? -1 : 0);
}

// can the edge add anything at a sample of rows [py0, py1] and columns up to px1?
VGX_HD bool vgx_raster_contour_edge_reaches(const VgxRasterTri& T, double py0, double py1, double px1)
{
	const double lo = (double)(T.miny < T.maxy ? T.miny : T.maxy), hi = (double)(T.miny < T.maxy ? T.maxy : T.miny);
	return lo < py1 && hi >= py0 && (double)T.minx <= px1;
}

// covered: inside the closed box of the mesh's vertices, and the fill rule on W
VGX_HD bool vgx_raster_contour_covered(int32_t W, uint32_t subpathKind, const float* box, double px, double py)
{
	if (!(px >= (double)box[0] && px <= (double)box[2] && py >= (double)box[1] && py <= (double)box[3])) { return false; }
	return (subpathKind & VGX_CONTOUR_EVEN_ODD) ? (W & 1) != 0 : W != 0;
}

// A covered sample of a contour mesh of the flat colour c: a covered sample of vertex colour c in every rule of the levels below.
// pad = the mesh state's (VGX_RT_GRADIENT / VGX_RT_PATTERN or neither); *S is the pixel's stamp
template <class Fetch>
VGX_HD uint32_t vgx_raster_contour_pixel(uint32_t c, uint32_t pad, const VgxRasterPaint& P, uint32_t mode, uint32_t f, uint32_t n, double px, double py, uint32_t* S,
                                         uint32_t dst, Fetch fetch)
{
	if (mode == VGX_RF_STAMP) { *S = f; return dst; }
	if (mode != VGX_RF_PLAIN && !vgx_raster_stamp_pass(*S, f, n, mode == VGX_RF_IN ? 0u : 1u)) { return dst; }
	if (pad & VGX_RT_GRADIENT) { return vgx_raster_gradient_shade(P, c >> 24, px, py, dst); }
	if (pad & VGX_RT_PATTERN) { return vgx_raster_pattern_shade(P, px, py, dst, fetch, [c](int ch) { return (c >> (8 * ch)) & 255u; }); }
	if ((c >> 24) == 0u) { return dst; }
	return vgx_raster_blend(dst, c & 255u, (c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
}

// ---- what a mesh does at a level -----------------------------------------------------------------------------------------------------
// The state of mesh `me` under its draw (me.draw < num_draws is the caller's check, at every level and whatever the kind). Every level:
// mode, region and rectangle. From VGX_RL_TEXTURED on a sampled mesh leaves VGX_RT_SAMPLED and its handle in `pad`; at VGX_RL_PAINTED
// a painted mesh leaves its table and handle there; at VGX_RL_CONCAVE a contour mesh adds VGX_RT_CONTOUR. VGX_RF_INVALID: the handle, the record it names or a pattern's image is no good.
// A table is read only at a level that uses it, and only the record a mesh names; below that level it may be null
VGX_HD void vgx_raster_mesh_state(int level, const vgx_mesh& me, uint32_t stateKey, const vgx_draw_state& ds, int32_t x0, int32_t y0, const uint32_t* scissor,
                                  const vgx_raster_image* images, uint32_t numImages, const vgx_paint* gradients, uint32_t numGradients,
                                  const vgx_paint* patterns, uint32_t numPatterns, VgxRasterMeshState* st)
{
	st->pad = 0u; st->f = 0u; st->n = 0u;
	if (!vgx_raster_draw_span(ds.scissor[0], ds.scissor[2], x0, scissor[0], scissor[2], &st->rect[0], &st->rect[2])
	 || !vgx_raster_draw_span(ds.scissor[1], ds.scissor[3], y0, scissor[1], scissor[3], &st->rect[1], &st->rect[3])) {
		st->rect[0] = st->rect[1] = st->rect[2] = st->rect[3] = 0u;
		st->mode = VGX_RF_NOTHING;
	} else if (vgx_raster_draw_type(stateKey) == 3u) {
		st->mode = VGX_RF_STAMP; st->f = me.draw;
	} else if (ds.clip_first_draw == VGX_RASTER_STAMP_NONE || ds.clip_num_draws == 0u) {
		st->mode = VGX_RF_PLAIN;
	} else {
		st->mode = ds.clip_rule == 0u ? VGX_RF_IN : VGX_RF_OUT;
		st->f = ds.clip_first_draw; st->n = ds.clip_num_draws;
	}
	const uint32_t handle = stateKey & 0xFFFFu;
	if (level >= VGX_RL_TEXTURED && vgx_raster_mesh_sampled(me.subpath_kind, stateKey)) { // a draw of type 0: not painted
		if (handle >= numImages || !vgx_raster_image_valid(images[handle])) { st->mode = VGX_RF_INVALID; return; }
		st->pad = VGX_RT_SAMPLED | handle;
		return;
	}
	const uint32_t contour = level >= VGX_RL_CONCAVE && vgx_raster_kind_is_contours(me.subpath_kind) ? VGX_RT_CONTOUR : 0u;
	const uint32_t painted = level >= VGX_RL_PAINTED ? vgx_raster_mesh_painted(stateKey) : 0u;
	if (!painted) { st->pad = contour; return; }
	const bool grad = painted == VGX_RT_GRADIENT;
	if (handle >= (grad ? numGradients : numPatterns)) { st->mode = VGX_RF_INVALID; return; }
	const vgx_paint* const p = (grad ? gradients : patterns) + handle;
	if (p->type != (grad ? 1u : 2u)) { st->mode = VGX_RF_INVALID; return; }
	if (!grad) {
		const uint32_t im = p->image & 0xFFFFu;
		if (im >= numImages || !vgx_raster_image_valid(images[im])) { st->mode = VGX_RF_INVALID; return; }
	}
	st->pad = painted | handle | contour;
}

// ---- the arguments of the calls (host only) ----------------------------------------------------------------------------------------
// Every check of these functions answers VGX_E_INVALID_ARG, and the callers put their VGX_E_RANGE checks last: which of several failing
// checks decides cannot be observed, so the checkers fold their common parts without minding the order.
// The target's size and origin: what the damage marks ask of a target, which write no pixel
static inline int vgx_target_extent_check(const vgx_raster_target& t)
{
	if (t.width > 16384u || t.height > 16384u || t.x0 > (1 << 23) || t.x0 < -(1 << 23) || t.y0 > (1 << 23) || t.y0 < -(1 << 23)) { return VGX_E_INVALID_ARG; }
	return VGX_OK;
}

// A target a call draws into: the extent, the stride, the scissor inside the image, and pixels unless the scissor is empty
static inline int vgx_target_check(const vgx_raster_target* target)
{
	if (!target || vgx_target_extent_check(*target) != VGX_OK) { return VGX_E_INVALID_ARG; }
	const vgx_raster_target& t = *target;
	if (t.stride < t.width || ((uintptr_t)t.pixels & 3u)) { return VGX_E_INVALID_ARG; }
	if (t.scissor[0] > t.scissor[2] || t.scissor[1] > t.scissor[3] || t.scissor[2] > t.width || t.scissor[3] > t.height) { return VGX_E_INVALID_ARG; }
	const bool empty = t.scissor[0] == t.scissor[2] || t.scissor[1] == t.scissor[3];
	return !empty && !t.pixels ? VGX_E_INVALID_ARG : VGX_OK;
}

// What vgx_raster (VGX_RL_PLAIN: state, tex and paints are not looked at), vgx_raster_frame, vgx_raster_textured and vgx_raster_painted
// refuse before anything runs, for the device calls and for the vgxt_* host loops alike: VGX_OK, VGX_E_INVALID_ARG or VGX_E_RANGE.
// `status` is where the call leaves its status (may be null)
static inline int vgx_raster_check_args(int level, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                                        const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_paints* paints,
                                        const vgx_raster_target* target, const uint32_t* status)
{
	if (!frame || vgx_target_check(target) != VGX_OK || (level >= VGX_RL_FRAME && !state) || (level >= VGX_RL_TEXTURED && !tex) || (level >= VGX_RL_PAINTED && !paints)) { return VGX_E_INVALID_ARG; }
	if (level >= VGX_RL_PAINTED) {
		if ((paints->num_gradients && !paints->gradients) || (paints->num_patterns && !paints->patterns)) { return VGX_E_INVALID_ARG; }
		if (((uintptr_t)paints->gradients & 3u) || ((uintptr_t)paints->patterns & 3u)) { return VGX_E_INVALID_ARG; }
	}
	if (level >= VGX_RL_TEXTURED) {
		if ((tex->uv_bytes != 4u && tex->uv_bytes != 8u) || (tex->num_images && !tex->images) || ((uintptr_t)tex->images & 7u)) { return VGX_E_INVALID_ARG; }
		const uint64_t e = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
		if (mesh_begin < e && (!tex->uv || ((uintptr_t)tex->uv & (tex->uv_bytes - 1u)))) { return VGX_E_INVALID_ARG; }
	}
	if (level >= VGX_RL_FRAME) {
		if (state->reserved != 0u || (state->num_draws && (!state->draws || !state->draw_state))) { return VGX_E_INVALID_ARG; }
		if (((uintptr_t)state->draws & 3u) || ((uintptr_t)state->draw_state & 3u)) { return VGX_E_INVALID_ARG; }
	}
	if (frame->num_meshes && (!frame->pos || !frame->color || !frame->idx || !frame->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)status & 3u) || ((uintptr_t)mesh_bounds & 15u) || ((uintptr_t)frame->pos & 7u)
		|| ((uintptr_t)frame->color & 3u) || ((uintptr_t)frame->idx & 1u) || ((uintptr_t)frame->meshes & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (frame->num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	return VGX_OK;
}

#endif
