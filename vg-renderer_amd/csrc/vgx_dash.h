// vgx_dash.h -- the arithmetic of the dash pass (vgx_dash, include/vgx.h "dashed strokes") for ONE draw's pattern, ONE segment,
// ONE "on" interval and ONE output vertex: host + device. The kernels of vgx_dash.hip run it one lane per segment / interval / output
// vertex; libvgx_hosttest.so (vgxt_dash, vgx_hosttest.cpp) runs the same functions list after list, interval after interval, so
// that the CPU suite pins them bit for bit against the sequential model in tests/dash_model.py without a GPU.
//
// Everything that decides WHERE a cut lies is integer: lengths in 2^-16 units (q), prefix sums S_j of a list in uint64, the
// pattern's prefix sums A_k, the period P and the phase f. Sums of integers do not depend on the order they are taken in, so the
// device-wide scan, this header and a sequential loop agree on every bit. Floats appear twice: the length of a segment (three
// rounded operations and a correctly rounded sqrtf) and the interpolated point of a cut inside a segment.
//
// "On" interval j = r * H + h (H = count / 2 intervals per period) is [r P + A[2h] - f, r P + A[2h+1] - f) cut to [0, T]; the
// intervals of a list that can meet [0, T] are j_lo .. j_hi, both closed-form (vgx_dash_intervals): one division and at most
// `count` comparisons. An interval that survives snapping is one piece; which vertices it holds follows from two searches in S.
#ifndef VGX_DASH_H
#define VGX_DASH_H

#include "vgx_lane.h"

#define VGX_DASH_SNAP 256ull                 // D: 2^-8 units
#define VGX_DASH_MAX_T (1ull << 62)          // longest list, fixed units
#define VGX_DASH_MAX_ENTRY 1099511627776.0f  // 2^40 units: pattern entries and the phase lie below it (P stays below 2^61)
#define VGX_DASH_MAX_LEN 70368744177664.0f   // 2^46 units: a longer segment alone exceeds VGX_DASH_MAX_T
#define VGX_DASH_MAX_INTERVALS 0xFFFFFFFFull // "on" intervals of one call (one work item each)

// the pattern of one draw, in fixed units
struct VgxDashPat
{
	uint64_t A[VGX_DASH_MAX + 1]; // A[k] = p_0 + ... + p_{k-1}
	uint64_t P, f;                // A[count], q(phase) mod P
	uint32_t count, pad;          // 0: the draw is not dashed
};

VGX_HD bool vgx_dash_finite(float v)
{
	union { float f; uint32_t u; } c; c.f = v;
	return (c.u & 0x7F800000u) != 0x7F800000u;
}

// q(x) for a finite x in [0, 2^46)
VGX_HD uint64_t vgx_dash_q(float x) { return (uint64_t)((double)x * 65536.0 + 0.5); }

VGX_HD bool vgx_dash_entry_ok(float v) { return vgx_dash_finite(v) && v >= 0.0f && v < VGX_DASH_MAX_ENTRY; }

// Validation of one record + its pattern in fixed units. false: the record breaks a rule (pat then says "not dashed").
VGX_HD bool vgx_dash_pat_build(const struct vgx_dash& d, const float* pattern, uint64_t npattern, VgxDashPat* pat)
{
	pat->P = 0; pat->f = 0; pat->count = 0; pat->pad = 0; pat->A[0] = 0;
	if (d.reserved != 0 || (d.count & 1u) || d.count > VGX_DASH_MAX) { return false; }
	if ((uint64_t)d.first > npattern || (uint64_t)d.count > npattern - d.first) { return false; }
	if (!vgx_dash_entry_ok(d.phase)) { return false; }
	if (d.count == 0) { return true; }
	uint64_t acc = 0;
	for (uint32_t k = 0; k < d.count; ++k) {
		const float p = pattern[(uint64_t)d.first + k];
		if (!vgx_dash_entry_ok(p)) { return false; }
		acc += vgx_dash_q(p);
		pat->A[k + 1] = acc;
	}
	if (acc == 0) { return false; }
	pat->P = acc; pat->f = vgx_dash_q(d.phase) % acc; pat->count = d.count;
	return true;
}

// segments of a list of n vertices
VGX_HD uint32_t vgx_dash_num_segments(uint32_t n, uint32_t flags) { return n < 2u ? 0u : ((flags & 1u) ? n : n - 1u); }

// len_i of the segment a -> b; false: not finite or beyond VGX_DASH_MAX_LEN
VGX_HD bool vgx_dash_seg_q(float ax, float ay, float bx, float by, uint64_t* q)
{
	const float dx = bx - ax;
	const float dy = by - ay;
	const float len = vgm_sqrt(dx * dx + dy * dy);
	*q = 0;
	if (!(len < VGX_DASH_MAX_LEN)) { return false; }
	*q = vgx_dash_q(len);
	return true;
}

// The "on" intervals of a list of length T that can meet [0, T]: *jlo = the first one, returns how many (0 for T = 0).
VGX_HD uint64_t vgx_dash_intervals(const VgxDashPat& pat, uint64_t T, uint64_t* jlo)
{
	*jlo = 0;
	if (T == 0 || pat.count == 0) { return 0; }
	const uint32_t H = pat.count / 2u;
	uint32_t h0 = 0; // the first interval that ends behind 0: A[2h+1] > f in period 0, or (f inside the last gap) interval 0 of period 1 = j H
	while (h0 < H && pat.A[2u * h0 + 1u] <= pat.f) { ++h0; }
	const uint64_t U = T + pat.f;            // an interval starts in front of T when r P + A[2h] < U
	const uint64_t r1 = (U - 1u) / pat.P;
	const uint64_t rem = U - r1 * pat.P;     // 1 .. P
	uint32_t hc = 1;                         // A[0] = 0 < rem
	while (hc < H && pat.A[2u * hc] < rem) { ++hc; }
	if (r1 > VGX_DASH_MAX_INTERVALS) { return ~0ull; }
	const uint64_t jhi = r1 * H + (hc - 1u);
	*jlo = h0;
	return jhi >= h0 ? jhi - h0 + 1u : 0u;
}

// One list: its vertices, its prefix sums (S_j = G[j] - G[0], j = 0 .. m) and its length
struct VgxDashList
{
	const float* v;    // [n][2]
	const uint64_t* G; // [m + 1]
	uint64_t T;
	uint32_t n, m;
};
VGX_HD uint64_t vgx_dash_S(const VgxDashList& L, uint32_t j) { return L.G[j] - L.G[0]; }
// the largest j in 0 .. m with S_j <= c
VGX_HD uint32_t vgx_dash_upper(const VgxDashList& L, uint64_t c)
{
	uint32_t lo = 0, hi = L.m + 1u; // S_lo <= c, S_hi > c (hi = m + 1: behind the end)
	while (hi - lo > 1u) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (vgx_dash_S(L, mid) <= c) { lo = mid; } else { hi = mid; }
	}
	return lo;
}
// the smallest j in 0 .. m with S_j >= c (c <= T)
VGX_HD uint32_t vgx_dash_lower(const VgxDashList& L, uint64_t c)
{
	if (c == 0) { return 0; }
	uint32_t lo = 0, hi = L.m; // S_lo < c, S_hi >= c
	while (hi - lo > 1u) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (vgx_dash_S(L, mid) < c) { lo = mid; } else { hi = mid; }
	}
	return hi;
}
VGX_HD uint64_t vgx_dash_snap(const VgxDashList& L, uint64_t c)
{
	uint32_t i = vgx_dash_upper(L, c);
	if (i >= L.m) { i = L.m - 1u; }
	const uint64_t s0 = vgx_dash_S(L, i), s1 = vgx_dash_S(L, i + 1u);
	if (c - s0 <= VGX_DASH_SNAP) { return s0; }
	if (s1 - c <= VGX_DASH_SNAP) { return s1; }
	return c;
}

// One piece: [s, e] after snapping, js = the largest j with S_j <= s, je = the smallest j with S_j >= e; it holds X(s), the
// vertices js + 1 .. je - 1 and X(e): je - js + 1 of them.
struct VgxDashPiece
{
	uint64_t s, e;
	uint32_t js, je;
};
// "on" interval j of a list with m >= 1 segments; false: it produces nothing
VGX_HD bool vgx_dash_piece(const VgxDashList& L, const VgxDashPat& pat, uint64_t j, VgxDashPiece* p)
{
	const uint32_t H = pat.count / 2u;
	const uint64_t r = j / H;
	const uint32_t h = (uint32_t)(j % H);
	const int64_t base = (int64_t)(r * pat.P) - (int64_t)pat.f;
	const int64_t a = base + (int64_t)pat.A[2u * h], b = base + (int64_t)pat.A[2u * h + 1u];
	if (b <= a || b <= 0 || a >= (int64_t)L.T) { return false; }
	uint64_t s = a < 0 ? 0ull : (uint64_t)a;
	uint64_t e = b > (int64_t)L.T ? L.T : (uint64_t)b;
	s = vgx_dash_snap(L, s);
	e = vgx_dash_snap(L, e);
	if (e <= s) { return false; }
	p->s = s; p->e = e;
	p->js = vgx_dash_upper(L, s);
	p->je = vgx_dash_lower(L, e);
	return true;
}
VGX_HD uint32_t vgx_dash_piece_vertices(const VgxDashPiece& p) { return p.je - p.js + 1u; }

VGX_HD V2 vgx_dash_vertex(const VgxDashList& L, uint32_t j)
{
	const uint32_t i = j >= L.n ? j - L.n : j; // j mod n for j <= m <= n
	return v2(L.v[2u * (size_t)i], L.v[2u * (size_t)i + 1u]);
}
// X(c) for a c strictly inside segment i
VGX_HD V2 vgx_dash_cut(const VgxDashList& L, uint32_t i, uint64_t c)
{
	const uint64_t s0 = vgx_dash_S(L, i), s1 = vgx_dash_S(L, i + 1u);
	const float t = (float)((double)(c - s0) / (double)(s1 - s0));
	const V2 a = vgx_dash_vertex(L, i), b = vgx_dash_vertex(L, i + 1u);
	return v2(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t);
}
// vertex k (0 .. je - js) of a piece
VGX_HD V2 vgx_dash_piece_vertex(const VgxDashList& L, const VgxDashPiece& p, uint32_t k)
{
	if (k == 0) { return vgx_dash_S(L, p.js) == p.s ? vgx_dash_vertex(L, p.js) : vgx_dash_cut(L, p.js, p.s); }
	if (k == p.je - p.js) { return vgx_dash_S(L, p.je) == p.e ? vgx_dash_vertex(L, p.je) : vgx_dash_cut(L, p.je - 1u, p.e); }
	return vgx_dash_vertex(L, p.js + k);
}

#endif
