// vgx_dash.hip -- the dash pass between vgx_flatten and the stroker-level entry (include/vgx.h "dashed strokes"): every vertex list of a
// dashed draw is cut into its "on" pieces. The arithmetic lives in vgx_dash.h (host + device); this file distributes it.
//
//   k_dash_draws     per draw: validation (a flagged reduction into the status word) + the pattern in fixed units (VgxDashPat);
//                    per pattern entry: validation
//   scan over lists  segments per list -> seg_base                                             (OpDashSegs,  vgx_scan.h)
//   scan over segs   q(len_i) of every segment of every dashed list -> G: S_j of list l = G[seg_base[l] + j] - G[seg_base[l]]. The sum is
//                    taken modulo 2^64 over the whole batch -- differences inside one list are exact as long as the list's own length
//                    fits, which the second component (sum of q >> 31) decides                  (OpDashLen)
//   scan over lists  "on" intervals per list, closed form from T, P, A_k, f -> cand_off        (OpDashCand)
//   k_dash_count     VGX_DASH_RANGES workgroups, each owning a contiguous range of the call's intervals, one lane per interval: does it
//                    survive snapping, how many vertices -> pieces / vertices per range
//   k_dash_ranges    scan over the ranges (one workgroup), totals, capacity check
//   k_dash_emit      the same ranges again, tile of 256 intervals after tile: one lane writes a piece's whole sub-path record; then the
//                    tile's OUTPUT vertices one per lane (the piece by a search in the tile's scanned counts in LDS): dense stores, and no
//                    lane loops over the pieces of a segment -- a 60 000-unit segment under [1,1] is 30 000 intervals = 30 000 lanes.
// Nothing is stored per interval or per output vertex: the scratch is per draw, per list, per segment (G) and per range.
#include "vgx_internal.h"
#include "vgx_scan.h"
#include "vgx_dash.h"

namespace {

__device__ __forceinline__ void dash_fail(VgxTotals* t, uint32_t err) { atomicCAS(&t->status, (uint32_t)VGX_OK, err); }

// the last list l with key(l) <= i, l in [0, n)  (key non-decreasing, key(0) <= i)
template <class KEY> __device__ __forceinline__ uint64_t dash_find(uint64_t n, uint64_t i, KEY key)
{
	uint64_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (key(mid) <= i) { lo = mid; } else { hi = mid; }
	}
	return lo;
}

// lists of the call: a host value, or (vgx_tessellate_dashed) a word an earlier launch wrote
__device__ __forceinline__ uint64_t dash_nsubs(const VgxDashArgs& A) { return A.nsubs_dev ? *A.nsubs_dev : A.nsubs; }

__device__ __forceinline__ bool dash_list_dashed(const VgxDashArgs& A, uint64_t l, uint32_t* draw)
{
	const uint32_t d = A.sub_draw[l];
	*draw = d;
	return d < A.ndraws && A.pat[d].count != 0;
}

// ---- per draw / per pattern entry ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dash_draws(VgxDashArgs A)
{
	const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
	bool bad = false;
	for (uint64_t d = gid; d < A.ndraws; d += stride) {
		if (!vgx_dash_pat_build(A.dashes[d], A.pattern, A.npattern, &A.pat[d])) { bad = true; } // (a failed build leaves "not dashed")
	}
	for (uint64_t k = gid; k < A.npattern; k += stride) {
		if (!vgx_dash_entry_ok(A.pattern[k])) { bad = true; }
	}
	if (__any(bad) && (threadIdx.x & 63u) == 0) { dash_fail(A.totals, VGX_E_INVALID_ARG); }
}

// ---- scan operators ----------------------------------------------------------------------------------------------
struct OpDashSegs // segments per list -> seg_base
{
	VgxDashArgs A;
	__device__ uint64_t size() const { return dash_nsubs(A); }
	__device__ Sum3 load(uint64_t l) const
	{
		Sum3 r = sum3_zero();
		uint32_t d;
		const bool dashed = dash_list_dashed(A, l, &d);
		if (d >= A.ndraws) { dash_fail(A.totals, VGX_E_INVALID_ARG); return r; }
		const vgx_subpath sp = A.subs[l];
		if (sp.num_vertices > 0x7FFFFFFFu) { dash_fail(A.totals, VGX_E_RANGE); return r; }
		r.a = dashed ? vgx_dash_num_segments(sp.num_vertices, sp.flags) : 0u;
		return r;
	}
	__device__ void store(uint64_t l, Sum3 e) const { A.lists[l].seg_base = e.a; }
	__device__ void finish(Sum3 t) const
	{
		A.lists[dash_nsubs(A)].seg_base = t.a;
		A.tot[0] = t.a;
		if (t.a > A.seg_cap) { dash_fail(A.totals, VGX_E_GROWN); }
	}
};

struct OpDashLen // q(len) per segment -> G (and the guard sums)
{
	VgxDashArgs A;
	__device__ uint64_t size() const { return A.totals->status == VGX_OK ? A.tot[0] : 0ull; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const VgxDashListRec* lists = A.lists;
		const uint64_t l = dash_find(dash_nsubs(A), i, [lists](uint64_t k) { return lists[k].seg_base; });
		const vgx_subpath sp = A.subs[l];
		const uint32_t k = (uint32_t)(i - lists[l].seg_base);
		const uint32_t k1 = k + 1u == sp.num_vertices ? 0u : k + 1u;
		const float2 a = *(const float2*)(A.poly + 2 * (sp.first_vertex + k)), b = *(const float2*)(A.poly + 2 * (sp.first_vertex + k1));
		uint64_t q;
		if (!vgx_dash_seg_q(a.x, a.y, b.x, b.y, &q)) { A.tot[2] = 1; } // becomes VGX_E_RANGE in finish(): size() must not change under the scan
		r.a = q; r.b = q >> 31;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { A.G[i] = e.a; A.Ghi[i] = e.b; }
	__device__ void finish(Sum3 t) const
	{
		const uint64_t n = size();
		A.G[n] = t.a; A.Ghi[n] = t.b;
		if (A.tot[2]) { dash_fail(A.totals, VGX_E_RANGE); }
	}
};

// what a list contributes: its "on" intervals (an undashed list: one, the copy). false: the batch is out of range
__device__ __forceinline__ bool dash_list_eval(const VgxDashArgs& A, uint64_t l, uint64_t* ncand, uint64_t* jlo, uint64_t* T)
{
	*ncand = 0; *jlo = 0; *T = 0;
	uint32_t d;
	if (!dash_list_dashed(A, l, &d)) { *ncand = A.frame ? 0u : 1u; return true; } // (a frame keeps the mesh descriptor of such a list: no copy)
	const vgx_subpath sp = A.subs[l];
	const uint32_t m = vgx_dash_num_segments(sp.num_vertices, sp.flags);
	if (m == 0) { return true; }
	const uint64_t base = A.lists[l].seg_base;
	if (A.Ghi[base + m] - A.Ghi[base] > (1ull << 31)) { return false; } // T >= 2^31 * that; at or below it the modular difference is T itself
	const uint64_t t = A.G[base + m] - A.G[base];
	if (t > VGX_DASH_MAX_T) { return false; }
	const uint64_t n = vgx_dash_intervals(A.pat[d], t, jlo);
	if (n > VGX_DASH_MAX_INTERVALS) { return false; }
	*ncand = n; *T = t;
	return true;
}

struct OpDashCand // "on" intervals per list -> cand_off, jlo, T
{
	VgxDashArgs A;
	__device__ uint64_t size() const { return A.totals->status == VGX_OK ? dash_nsubs(A) : 0ull; }
	__device__ Sum3 load(uint64_t l) const
	{
		Sum3 r = sum3_zero();
		uint64_t jlo, T;
		if (!dash_list_eval(A, l, &r.a, &jlo, &T)) { A.tot[2] = 1; r.a = 0; } // VGX_E_RANGE in finish()
		return r;
	}
	__device__ void store(uint64_t l, Sum3 e) const
	{
		uint64_t n, jlo, T;
		(void)dash_list_eval(A, l, &n, &jlo, &T);
		A.lists[l].cand_off = e.a; A.lists[l].jlo = jlo; A.lists[l].T = T;
	}
	__device__ void finish(Sum3 t) const
	{
		A.lists[dash_nsubs(A)].cand_off = t.a;
		A.tot[1] = t.a;
		if (t.a > VGX_DASH_MAX_INTERVALS || A.tot[2]) { dash_fail(A.totals, VGX_E_RANGE); }
	}
};

// ---- per interval --------------------------------------------------------------------------------------------------
struct DashItem // what one lane knows about its interval
{
	VgxDashList L;
	VgxDashPiece p;
	uint64_t list;
	uint32_t nv;     // vertices it writes
	uint32_t flags;  // of its record
	uint32_t draw;
	bool exists, copy;
};

__device__ __forceinline__ VgxDashList dash_list_of(const VgxDashArgs& A, uint64_t l, const vgx_subpath& sp)
{
	VgxDashList L;
	L.v = A.poly + 2 * sp.first_vertex;
	L.G = A.G + A.lists[l].seg_base;
	L.T = A.lists[l].T;
	L.n = sp.num_vertices; L.m = vgx_dash_num_segments(sp.num_vertices, sp.flags);
	return L;
}

__device__ __forceinline__ void dash_item(const VgxDashArgs& A, uint64_t c, DashItem* it)
{
	const VgxDashListRec* lists = A.lists;
	const uint64_t l = dash_find(dash_nsubs(A), c, [lists](uint64_t k) { return lists[k].cand_off; });
	const vgx_subpath sp = A.subs[l];
	it->list = l;
	it->copy = !dash_list_dashed(A, l, &it->draw);
	if (it->copy) { it->exists = true; it->nv = sp.num_vertices; it->flags = sp.flags; it->L.v = A.poly + 2 * sp.first_vertex; return; }
	it->L = dash_list_of(A, l, sp);
	it->flags = 0;
	it->exists = vgx_dash_piece(it->L, A.pat[it->draw], lists[l].jlo + (c - lists[l].cand_off), &it->p);
	it->nv = it->exists ? vgx_dash_piece_vertices(it->p) : 0u;
}

// the range of intervals workgroup b owns
__device__ __forceinline__ void dash_range(const VgxDashArgs& A, uint64_t* lo, uint64_t* hi)
{
	const uint64_t n = A.tot[1];
	uint64_t per = (n + VGX_DASH_RANGES - 1) / VGX_DASH_RANGES;
	per = (per + 255u) / 256u * 256u;
	uint64_t l = per * blockIdx.x, h = l + per;
	if (l > n) { l = n; }
	if (h > n) { h = n; }
	*lo = l; *hi = h;
}

__global__ __launch_bounds__(256) void k_dash_count(VgxDashArgs A)
{
	__shared__ Sum3 sWave[4];
	Sum3 acc = sum3_zero();
	if (A.totals->status == VGX_OK) { // block-uniform
		uint64_t lo, hi;
		dash_range(A, &lo, &hi);
		for (uint64_t c = lo + threadIdx.x; c < hi; c += 256u) {
			DashItem it;
			dash_item(A, c, &it);
			acc.a += it.exists ? 1u : 0u; acc.b += it.nv;
		}
	}
	Sum3 tot;
	block_incl_scan<256>(acc, sWave, &tot);
	if (threadIdx.x == 0) { A.range_sum[2 * blockIdx.x] = tot.a; A.range_sum[2 * blockIdx.x + 1] = tot.b; }
}

__global__ __launch_bounds__(VGX_DASH_RANGES) void k_dash_ranges(VgxDashArgs A)
{
	__shared__ Sum3 sWave[VGX_DASH_RANGES / 64];
	Sum3 v = sum3_zero();
	v.a = A.range_sum[2 * threadIdx.x]; v.b = A.range_sum[2 * threadIdx.x + 1];
	Sum3 tot;
	const Sum3 incl = block_incl_scan<VGX_DASH_RANGES>(v, sWave, &tot);
	A.range_off[2 * threadIdx.x] = incl.a - v.a; A.range_off[2 * threadIdx.x + 1] = incl.b - v.b;
	if (threadIdx.x == 0 && A.totals->status == VGX_OK) {
		A.totals->sizes.num_subpaths = tot.a; A.totals->sizes.num_poly_vertices = tot.b;
		if (A.check_caps && (tot.a > A.cap_subs || tot.b > A.cap_poly)) { dash_fail(A.totals, VGX_E_NOSPACE); }
	}
}

__global__ __launch_bounds__(256) void k_dash_emit(VgxDashArgs A)
{
	__shared__ Sum3 sWave[4];
	__shared__ uint64_t sV0[256], sS[256], sE[256], sList[256];
	__shared__ uint32_t sJs[256], sJe[256];
	if (A.totals->status != VGX_OK) { return; } // block-uniform: the last writer (k_dash_ranges) ran before this launch
	const uint32_t t = threadIdx.x;
	uint64_t lo, hi;
	dash_range(A, &lo, &hi);
	uint64_t pOff = A.range_off[2 * blockIdx.x], vOff = A.range_off[2 * blockIdx.x + 1];
	for (uint64_t base = lo; base < hi; base += 256u) {
		const uint64_t c = base + t;
		DashItem it;
		it.exists = false; it.copy = false; it.nv = 0; it.list = 0; it.p.s = 0; it.p.e = 0; it.p.js = 0; it.p.je = 0;
		if (c < hi) { dash_item(A, c, &it); }
		Sum3 v = sum3_zero();
		v.a = it.exists ? 1u : 0u; v.b = it.nv;
		Sum3 tot;
		const Sum3 incl = block_incl_scan<256>(v, sWave, &tot);
		const uint64_t v0 = incl.b - v.b;
		if (it.exists) { // the record, whole, by this lane
			const uint64_t slot = pOff + (incl.a - v.a);
			vgx_subpath rec;
			rec.first_vertex = vOff + v0; rec.num_vertices = it.nv; rec.flags = it.flags;
			A.out_subs[slot] = rec;
			A.out_draw[slot] = it.draw;
			if (A.out_src) { A.out_src[slot] = (uint32_t)it.list; }
		}
		sV0[t] = v0; sList[t] = it.copy ? (it.list | (1ull << 63)) : it.list;
		sS[t] = it.p.s; sE[t] = it.p.e; sJs[t] = it.p.js; sJe[t] = it.p.je;
		__syncthreads();
		// the tile's output vertices, one per lane
		for (uint64_t o = t; o < tot.b; o += 256u) {
			uint32_t a = 0, b = 256;
			while (b - a > 1u) {
				const uint32_t mid = (a + b) >> 1;
				if (sV0[mid] <= o) { a = mid; } else { b = mid; }
			}
			const uint32_t k = (uint32_t)(o - sV0[a]);
			const uint64_t l = sList[a] & ~(1ull << 63);
			const vgx_subpath sp = A.subs[l];
			V2 x;
			if (sList[a] >> 63) {
				const float2 w = *(const float2*)(A.poly + 2 * (sp.first_vertex + k));
				x = v2(w.x, w.y);
			} else {
				const VgxDashList L = dash_list_of(A, l, sp);
				VgxDashPiece p;
				p.s = sS[a]; p.e = sE[a]; p.js = sJs[a]; p.je = sJe[a];
				x = vgx_dash_piece_vertex(L, p, k);
			}
			*(float2*)(A.out_poly + 2 * (vOff + o)) = make_float2(x.x, x.y);
		}
		__syncthreads();
		pOff += tot.a; vOff += tot.b;
	}
}

__global__ __launch_bounds__(256) void k_subpath_draws(const vgx_draw_info* dinfo, uint64_t ndraws, uint32_t* subDraw, uint64_t nsubs)
{
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nsubs; i += stride) {
		// the last draw whose first sub-path is at or before i (draws without sub-paths share their successor's first_subpath)
		subDraw[i] = (uint32_t)dash_find(ndraws, i, [dinfo](uint64_t k) { return dinfo[k].first_subpath; });
	}
}

} // namespace

void vgx_launch_dash(const VgxDashArgs& a, bool emit, hipStream_t s)
{
	const uint64_t work = a.ndraws > a.npattern ? a.ndraws : a.npattern;
	const uint64_t blocks = (work + 255) / 256;
	hipLaunchKernelGGL(k_dash_draws, dim3((uint32_t)(blocks > 1024 ? 1024 : (blocks ? blocks : 1))), dim3(256), 0, s, a);
	OpDashSegs o1; o1.A = a;
	vgx_device_scan(o1, a.partial, s, a.nsubs);
	OpDashLen o2; o2.A = a;
	vgx_device_scan(o2, a.partial, s, a.seg_cap);
	OpDashCand o3; o3.A = a;
	vgx_device_scan(o3, a.partial, s, a.nsubs);
	hipLaunchKernelGGL(k_dash_count, dim3(VGX_DASH_RANGES), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dash_ranges, dim3(1), dim3(VGX_DASH_RANGES), 0, s, a);
	if (emit) { hipLaunchKernelGGL(k_dash_emit, dim3(VGX_DASH_RANGES), dim3(256), 0, s, a); }
}

void vgx_launch_subpath_draws(const vgx_draw_info* dinfo, uint64_t ndraws, uint32_t* subDraw, uint64_t nsubs, hipStream_t s)
{
	const uint64_t blocks = (nsubs + 255) / 256;
	hipLaunchKernelGGL(k_subpath_draws, dim3((uint32_t)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, dinfo, ndraws, subDraw, nsubs);
}
