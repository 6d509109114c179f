// vgx_pick_cmds.hip -- hit testing of a draw-command table on gfx950 (include/vgx.h: vgx_pick_commands, vgx_pick_commands_boxed; the rules:
// vgx_pick_cmds.h, vgx_cmd_bounds.h).
//
// vgx_pick_frame compacts candidate MESHES by their boxes and keeps one covered bit per (candidate, query). A command has no box and
// holds tens of thousands of triangles, and the caller wants the triangle, not only the command: the limit of a click-through lies
// INSIDE a command. So this family works on chunks of 64 consecutive triangles of one command, as k_rasterc_count does, and keeps one
// word per (query, command): the largest counting triangle + 1.
//   k_pickc_cmds     one lane per command (grid-stride: the real count may live on the device), the queries' points staged once per
//                    workgroup in LDS: validity of the record, mode, region and scissor (vgx_pickc_cmd_state), and whether the command
//                    is a candidate -- it has a triangle and some point lies in its scissor. The same grid zeroes the top table
//   scan OpPickcCmds every candidate's first chunk, the chunk total and the count of invalid records; finish() decides dev_status
//   k_pickc_tris     the hot path. Fixed grid, one WAVE per chunk, the chunks of a wave contiguous (VgxChunkWalk, vgx_raster_cmds.h). A
//                    lane loads three indices and three positions once and runs vgx_raster_setup once -- and only when some query
//                    lies in the chunk's box -- and three colours only when some query asks for the transparency rule and the command
//                    is no Clip. A wave reduction over the corners (vgx_wave.h) gives the chunk's box. The queries are staged in LDS
//                    SORTED by x (a rank count per workgroup), so a chunk bisects to the queries inside its box's x range and loops
//                    over those alone; the loop is wave-uniform: a query outside the command's scissor or the box's y range, or whose
//                    limit lies below the chunk, costs scalar tests and no vector work. Lanes ascend in t, so the highest counting
//                    lane holds the chunk's maximum: ONE atomicMax of t + 1 per wave and query. No per-chunk storage: overlapping
//                    index ranges leave the chunk total unbounded
//   k_pickc_resolve  one workgroup per query over the commands in ascending blocks of 256: "the last covering clip command so far"
//                    (stamper_before_me, vgx_wave.h), then the stamp test; the answer is the highest passing command, its triangle
//                    is the table's word. One lane does the owner search and writes the record
// Maxima only: the result does not depend on the order of the work.
// vgx_pick_commands_boxed runs the BOXED instantiations of k_pickc_cmds and k_pickc_tris: a command is a candidate only when some point
// lies in its scissor AND in its entry of the caller's box table (vgx_cmd_bounds.h), so a boxed-out command gets no chunks, and the
// per-query scalar tests of k_pickc_tris gain the same clause. vgx_pick_commands keeps the instantiations without it.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_pick_cmds.h"
#include "vgx_cmd_bounds.h"

namespace {

#define VGX_PICKC_CAND  0x100u      // beside the mode in VgxPickfMesh::mode: the command has chunks

struct PickcQuery : VgxPickStagedPoint { uint32_t cmd_end, tri_end, flags, q; }; // 32 bytes; q: the query's number, once the list is sorted

__device__ __forceinline__ PickcQuery pickc_query(const vgx_pick_cmd_query Q)
{
	PickcQuery P;
	P.cmd_end = Q.cmd_end; P.tri_end = Q.tri_end; P.q = 0u;
	P.flags = vgx_pick_stage_point(Q.x, Q.y, Q.flags, Q.reserved == 0u, &P); // takes part: vgx_pickc_point
	return P;
}

// BOXED (vgx_pick_commands_boxed): a command is a candidate only when some point also lies in its box. vgx_pick_commands launches the
// instantiations without it, which hold none of its code
template<bool BOXED>
__global__ __launch_bounds__(256) void k_pickc_cmds(VgxPickcArgs A)
{
	__shared__ PickcQuery s_q[VGX_PICK_MAX_QUERIES];
	if (threadIdx.x < A.nqueries) { s_q[threadIdx.x] = pickc_query(A.queries[threadIdx.x]); }
	__syncthreads();
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t words = (uint64_t)A.nqueries * A.num_cmds;
	for (uint64_t w = first; w < words; w += stride) { A.top[w] = 0u; }
	const uint32_t n = vgx_real_cmds(A.num_cmds, A.dev_num_cmds);
	for (uint64_t c = first; c < n; c += stride) {
		VgxPickfMesh st;
		vgx_pickc_cmd_state(A.cmds[c], (uint32_t)c, A.num_vertices, A.num_indices, n, &st);
		if (st.mode != VGX_RF_INVALID && st.elems) {
			bool cand = false;
			float box[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			if (BOXED) { const float4 b = *(const float4*)(A.cmd_bounds + 4ull * c); box[0] = b.x; box[1] = b.y; box[2] = b.z; box[3] = b.w; }
			for (uint32_t q = 0; q < A.nqueries; ++q) {
				const PickcQuery Q = s_q[q];
				cand = cand || ((Q.flags & VGX_PICK_STAGED_VALID) && vgx_pickf_in_scissor(st.rect, Q.X, Q.Y) && (!BOXED || vgx_cmdb_holds(box, Q.x, Q.y)));
			}
			if (cand) { st.mode |= VGX_PICKC_CAND; }
		}
		A.cmd_state[c] = st;
	}
}

struct OpPickcCmds
{
	VgxPickcArgs A;
	__device__ uint64_t size() const { return vgx_real_cmds(A.num_cmds, A.dev_num_cmds); }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t mode = A.cmd_state[i].mode;
		r.a = (mode & VGX_PICKC_CAND) ? vgx_rasterc_chunks(A.cmds[i]) : 0u;
		r.c = mode == VGX_RF_INVALID ? 1u : 0u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { A.cmd_first[i] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		const uint32_t n = vgx_real_cmds(A.num_cmds, A.dev_num_cmds);
		A.cmd_first[n] = t.a;
		A.state[VGX_PICKC_CHUNKS] = t.a; A.state[VGX_PICKC_INVALID] = t.c; A.state[VGX_PICKC_CMDS] = n;
		if (A.status) { *A.status = t.c ? (uint32_t)VGX_E_INVALID_ARG : (uint32_t)VGX_OK; }
	}
};

template<bool BOXED>
__global__ __launch_bounds__(256) void k_pickc_tris(VgxPickcArgs A)
{
	__shared__ PickcQuery s_q[VGX_PICK_MAX_QUERIES];
	__shared__ float s_x[VGX_PICK_MAX_QUERIES];
	// the queries that take part, sorted by x (ties by number), the others behind them: a chunk looks only at those inside its box's x
	// range. The order of the work changes; maxima do not care
	const uint32_t tid = threadIdx.x;
	PickcQuery P = {};
	bool valid = false, wantAlpha = false;
	if (tid < A.nqueries) {
		P = pickc_query(A.queries[tid]);
		valid = (P.flags & VGX_PICK_STAGED_VALID) != 0u;
		wantAlpha = valid && (P.flags & VGX_PICK_SKIP_TRANSPARENT) != 0u;
	}
	s_x[tid] = valid ? P.x : __int_as_float(0x7FC00000); // NaN: compares false, counts for nothing below
	const uint32_t nvalid = (uint32_t)__syncthreads_count(valid ? 1 : 0);
	const bool anyAlpha = __syncthreads_or(wantAlpha ? 1 : 0) != 0;
	if (tid < A.nqueries) {
		uint32_t rank = 0;
		if (valid) {
			for (uint32_t j = 0; j < A.nqueries; ++j) { const float xj = s_x[j]; rank += (xj < P.x || (xj == P.x && j < tid)) ? 1u : 0u; }
		} else {
			rank = nvalid;
			for (uint32_t j = 0; j < tid; ++j) { const float xj = s_x[j]; rank += xj == xj ? 0u : 1u; }
		}
		P.q = tid;
		s_q[rank] = P; // a permutation of [0, nqueries)
	}
	__syncthreads();
	if (A.state[VGX_PICKC_INVALID] != 0ull) { return; } // every hit is "none": k_pickc_resolve
	const uint64_t total = A.state[VGX_PICKC_CHUNKS];
	const uint32_t n = (uint32_t)A.state[VGX_PICKC_CMDS];
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	const float inf = __int_as_float(0x7F800000);
	// a wave takes a contiguous run of chunks (VgxChunkWalk): the command's record, state and box are loaded once per command, not once
	// per chunk (a stride over the chunks paid ten dependent loads for each)
	VgxChunkWalk W(A.cmd_first, n, total, (uint64_t)blockIdx.x * (blockDim.x / VGX_WAVE) + (threadIdx.x / VGX_WAVE), (uint64_t)gridDim.x * (blockDim.x / VGX_WAVE));
	if (W.k0 >= W.k1) { return; }
	vgx_raster_cmd cmd = A.cmds[W.c];
	VgxPickfMesh st = A.cmd_state[W.c];
	float box[4] = { 0.0f, 0.0f, 0.0f, 0.0f }; // BOXED: the command's entry, wave-uniform as the record and the state are
	if (BOXED) { const float4 b = *(const float4*)(A.cmd_bounds + 4ull * W.c); box[0] = b.x; box[1] = b.y; box[2] = b.z; box[3] = b.w; }
	for (uint64_t k = W.k0; k < W.k1; ++k) {
		if (W.advance(k)) {
			cmd = A.cmds[W.c]; st = A.cmd_state[W.c];
			if (BOXED) { const float4 b = *(const float4*)(A.cmd_bounds + 4ull * W.c); box[0] = b.x; box[1] = b.y; box[2] = b.z; box[3] = b.w; }
		}
		const uint32_t c = W.c;
		const uint32_t mode = st.mode & 0xFFu;
		const uint32_t t0 = (uint32_t)(k - W.first) * VGX_RASTERC_CHUNK;
		const uint32_t t = t0 + (uint32_t)lane;
		uint64_t v[3];
		float2 p0 = make_float2(0.0f, 0.0f), p1 = p0, p2 = p0;
		const bool have = vgx_rasterc_triangle(cmd, A.idx, t, v); // inside the command's ranges, and those inside the streams: k_pickc_cmds
		if (have) {
			const float2* pp = (const float2*)A.pos;
			p0 = pp[v[0]]; p1 = pp[v[1]]; p2 = pp[v[2]];
		}
		if (!wave_ballot(have)) { continue; }
		// The chunk's box over the corners of ALL its triangles, before any setup: a superset of every covering triangle's box, which is
		// all the tests below need (fminf / fmaxf pass over a NaN; a box of NaNs alone compares false and sends the chunk on to the
		// setup, which then finds nothing). Most chunks of a large frame end here. Scalars: the query loops below are wave-uniform
		const float bx0 = wave_uniform_f32(wave_min_f32(have ? fminf(fminf(p0.x, p1.x), p2.x) : inf)), by0 = wave_uniform_f32(wave_min_f32(have ? fminf(fminf(p0.y, p1.y), p2.y) : inf));
		const float bx1 = wave_uniform_f32(wave_max_f32(have ? fmaxf(fmaxf(p0.x, p1.x), p2.x) : -inf)), by1 = wave_uniform_f32(wave_max_f32(have ? fmaxf(fmaxf(p0.y, p1.y), p2.y) : -inf));
		uint32_t qa = 0, qb = nvalid; // the first sorted query with x >= bx0
		while (qa < qb) {
			const uint32_t mid = qa + ((qb - qa) >> 1);
			if (s_q[mid].x < bx0) { qa = mid + 1u; } else { qb = mid; }
		}
		bool any = false; // binary32 compares: the same as the binary64 compares of the widened values
		for (uint32_t k2 = qa; k2 < nvalid && !any; ++k2) {
			const PickcQuery Q = s_q[k2];
			if (Q.x > bx1) { break; }
			any = !(Q.y < by0) && !(Q.y > by1) && vgx_pickf_in_scissor(st.rect, Q.X, Q.Y) && (!BOXED || vgx_cmdb_holds(box, Q.x, Q.y));
		}
		if (!any) { continue; }
		VgxRasterTri Tri;
		bool ok = false, transparent = false;
		if (have) {
			ok = vgx_raster_setup(v2(p0.x, p0.y), v2(p1.x, p1.y), v2(p2.x, p2.y), 0u, 0u, 0u, &Tri);
			if (ok && anyAlpha && mode != VGX_RF_STAMP) { transparent = vgx_pick_tri_transparent(A.color[v[0]], A.color[v[1]], A.color[v[2]]); } // a clip command's colours are not read
		}
		if (!wave_ballot(ok)) { continue; }
		for (uint32_t k2 = qa; k2 < nvalid; ++k2) {
			const PickcQuery Q = s_q[k2];
			if (Q.x > bx1) { break; }
			if (Q.y < by0 || Q.y > by1 || !vgx_pickf_in_scissor(st.rect, Q.X, Q.Y) || (BOXED && !vgx_cmdb_holds(box, Q.x, Q.y))) { continue; }
			const double px = (double)Q.x, py = (double)Q.y;
			if (mode != VGX_RF_STAMP && !vgx_pickc_below(c, t0, Q.cmd_end, Q.tri_end)) { continue; } // the limit lies at or below the chunk's first triangle
			double E[3], S;
			const bool hit = ok && vgx_pickc_counts(mode, c, t, transparent, Q.cmd_end, Q.tri_end, Q.flags) && vgx_raster_cover(Tri, px, py, E, &S);
			const uint64_t hits = wave_ballot(hit);
			// triangles ascend with the lane: the highest counting lane holds the chunk's maximum
			if (hits && lane == 0) { atomicMax(A.top + (uint64_t)Q.q * A.num_cmds + c, t0 + (uint32_t)(63 - __clzll((long long)hits)) + 1u); }
		}
	}
}

__global__ __launch_bounds__(256) void k_pickc_resolve(VgxPickcArgs A)
{
	__shared__ uint32_t s_w[4];
	const uint32_t q = blockIdx.x, tid = threadIdx.x;
	double px, py;
	int32_t X, Y;
	const bool point = vgx_pickc_point(A.queries[q], &px, &py, &X, &Y);
	const uint64_t n = point && A.state[VGX_PICKC_INVALID] == 0ull ? A.state[VGX_PICKC_CMDS] : 0ull; // an invalid record: every hit is "none"
	const uint32_t* top = A.top + (uint64_t)q * A.num_cmds;
	uint32_t carry = 0, best = 0; // command numbers + 1: the last covering clip command of the blocks before, my highest hit
	for (uint64_t base = 0; base < n; base += 256) {
		const uint64_t c = base + tid;
		const bool covered = c < n && top[c] != 0u;
		if (!__syncthreads_or(covered ? 1 : 0)) { continue; }
		uint32_t mode = VGX_RF_NOTHING, f = 0, nn = 0;
		if (covered) {
			const uint4 s0 = *(const uint4*)(A.cmd_state + c);
			mode = s0.x & 0xFFu; f = s0.y; nn = s0.z;
		}
		const uint32_t stamper = stamper_before_me(covered && mode == VGX_RF_STAMP ? (uint32_t)c + 1u : 0u, &carry, s_w);
		if (covered && vgx_pickc_hit(mode, f, nn, stamper ? stamper - 1u : VGX_RASTER_STAMP_NONE)) { best = (uint32_t)c + 1u; } // a clip command stamps its own index
	}
	best = block_max_u32(best, s_w);
	if (tid == 0) {
		A.hits[q] = vgx_pickc_record(best ? best - 1u : VGX_PICK_NONE, best ? top[best - 1u] - 1u : VGX_PICK_NONE, A.cmds, A.meshes, A.num_meshes);
	}
}

} // namespace

void vgx_launch_pick_commands(const VgxPickcArgs& a, void* partial, uint32_t grid, hipStream_t s)
{
	if (a.num_cmds) {
		const uint64_t items = (uint64_t)a.num_cmds * (a.nqueries ? a.nqueries : 1u);
		const uint64_t blocks = (items + 255u) / 256u;
		const dim3 g((unsigned)(blocks < 1024u ? blocks : 1024u));
		if (a.cmd_bounds) { hipLaunchKernelGGL(k_pickc_cmds<true>, g, dim3(256), 0, s, a); } else { hipLaunchKernelGGL(k_pickc_cmds<false>, g, dim3(256), 0, s, a); }
	}
	const OpPickcCmds op = { a };
	vgx_device_scan(op, (Sum3*)partial, s, a.num_cmds); // an empty table too: it leaves the totals and the status
	if (!a.nqueries) { return; }
	if (a.num_cmds) {
		if (a.cmd_bounds) { hipLaunchKernelGGL(k_pickc_tris<true>, dim3(grid), dim3(256), 0, s, a); } else { hipLaunchKernelGGL(k_pickc_tris<false>, dim3(grid), dim3(256), 0, s, a); }
	}
	hipLaunchKernelGGL(k_pickc_resolve, dim3(a.nqueries), dim3(256), 0, s, a);
}
