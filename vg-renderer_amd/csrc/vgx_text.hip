// vgx_text.hip -- the device half of renderTextQuads (reference src/vg.cpp:5541-5621) for a batch of text runs: the glyph quads
// FontStash made on the caller's side -> positions (vgutil::batchTransformTextQuads), replicated colours, UVs, quad indices
// (vgutil::genQuadIndices_unaligned), each run at the places the caller chose. The arithmetic lives in vgx_text.h (host + device).
//
// The kernel is a stream: 32 bytes read and 76 (int16 UVs) or 92 (float UVs) bytes written per quad, no arithmetic worth the name.
// A workgroup takes a tile of VGX_TEXT_TILE consecutive quads, one quad per lane:
//   - the first run of the tile comes from a per-tile table the run kernel wrote (runs are in quad order; one thread per run
//     writes its index to the tiles that begin inside it) -- or, for a frame-sized call that is ONE launch, from one binary search
//     by one lane; where the runs that begin inside the tile begin goes into an LDS table, a quad finds its run by a binary search
//     there, and the lanes of a run read its 80-byte record from the same address;
//   - runs laid out back to back (the dense layout, the usual case) make every output stream of the tile one contiguous range
//     whatever the run boundaries inside it. That is detected per tile (vertex / index place of quad j = place of the tile's first quad + 4 j / 6 j);
//     the tile is then staged in LDS at the misalignment of its global range and leaves as whole, aligned 16-byte stores contiguous
//     across lanes (a lane per 16 output bytes of a stream), with element-sized stores for a ragged head / tail only;
//   - any other tile (gaps, runs that write nothing, odd placements) takes the edge path: element-sized stores per quad.
#include "vgx_internal.h"
#include "vgx_text.h"

#define VGX_TEXT_TILE 256u // quads per workgroup = lanes per workgroup
#define VGX_TEXT_RT 320u   // LDS run-table entries per tile (a tile with more runs -- hundreds of empty ones -- searches in memory)

namespace {

// ---- per run: validation, mesh record, totals, tile table ---------------------------------------------------
__device__ __forceinline__ void text_run_records(const VgxTextArgs& A, uint64_t gid, uint64_t gstride)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t ntiles = (A.nquads + VGX_TEXT_TILE - 1) / VGX_TEXT_TILE;
	// totals of this lane's runs; one set of atomics per workgroup at the end (same-address atomics are served one after the other:
	// a set per wave of 64 runs took longer than the whole quad kernel)
	uint32_t st = VGX_OK;
	uint64_t endV = 0, endI = 0, nq = 0;
	for (uint64_t r = gid; r < A.nruns; r += gstride) {
		const vgx_text_run run = A.runs[r];
		float m[6];
		uint32_t rst = (uint32_t)vgx_text_run_status(run, m);
		bool ordered = run.first_quad <= A.nquads && run.num_quads <= A.nquads - run.first_quad;
		if (r > 0) {
			const uint64_t pf = A.runs[r - 1].first_quad; const uint32_t pn = A.runs[r - 1].num_quads;
			ordered = ordered && pf <= run.first_quad && pn <= run.first_quad - pf;
		}
		if (rst == VGX_OK && !ordered) { rst = VGX_E_INVALID_ARG; }
		if (rst == VGX_OK) {
			const uint64_t nv = 4ull * run.num_quads, ni = 6ull * run.num_quads;
			const uint64_t ev = run.first_vertex > ~0ull - nv ? ~0ull : run.first_vertex + nv;
			const uint64_t ei = run.first_index > ~0ull - ni ? ~0ull : run.first_index + ni;
			endV = ev > endV ? ev : endV; endI = ei > endI ? ei : endI;
			nq += run.num_quads;
			if (!vgx_text_run_fits(run, A.cap_vertices, A.cap_indices)) { rst = VGX_E_NOSPACE; }
		}
		if (A.meshes) {
			const uint64_t slot = A.first_mesh + r;
			if (slot < A.cap_meshes) { A.meshes[slot] = vgx_text_run_mesh(run, rst == VGX_OK); }
			else if (rst == VGX_OK) { rst = VGX_E_NOSPACE; }
		}
		st = st ? st : rst;
		if (A.tile_run) { // tiles that begin in [first_quad, next run's first_quad): this run is the last one at or before their first quad
			const uint64_t f = r == 0 ? 0ull : run.first_quad;
			const uint64_t nx = r + 1 < A.nruns ? A.runs[r + 1].first_quad : ~0ull;
			const uint64_t tlo = f / VGX_TEXT_TILE + (f % VGX_TEXT_TILE ? 1u : 0u);
			uint64_t thi = nx / VGX_TEXT_TILE + (nx % VGX_TEXT_TILE ? 1u : 0u);
			if (thi > ntiles) { thi = ntiles; }
			for (uint64_t t = tlo; t < thi; ++t) { A.tile_run[t] = (uint32_t)r; }
		}
	}
	for (int o = 32; o > 0; o >>= 1) {
		const uint64_t v = __shfl_xor((unsigned long long)endV, o), i = __shfl_xor((unsigned long long)endI, o), q = __shfl_xor((unsigned long long)nq, o);
		const uint32_t s = __shfl_xor(st, o);
		endV = v > endV ? v : endV; endI = i > endI ? i : endI; nq += q;
		st = st ? st : s;
	}
	__shared__ uint64_t sTot[4][3];
	__shared__ uint32_t sSt[4];
	const uint32_t wave = threadIdx.x >> 6;
	if (lane == 0) { sTot[wave][0] = endV; sTot[wave][1] = endI; sTot[wave][2] = nq; sSt[wave] = st; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (uint32_t w = 1; w < 4; ++w) {
			endV = sTot[w][0] > endV ? sTot[w][0] : endV; endI = sTot[w][1] > endI ? sTot[w][1] : endI; nq += sTot[w][2];
			st = st ? st : sSt[w];
		}
		if (endV) { atomicMax((unsigned long long*)&A.totals->sizes.num_vertices, (unsigned long long)endV); }
		if (endI) { atomicMax((unsigned long long*)&A.totals->sizes.num_indices, (unsigned long long)endI); }
		if (nq) { atomicAdd((unsigned long long*)&A.totals->sizes.num_elements, (unsigned long long)nq); }
		if (st != VGX_OK) { atomicCAS(&A.totals->status, (uint32_t)VGX_OK, st); }
	}
	if (gid == 0) { A.totals->sizes.num_meshes = A.first_mesh + A.nruns; }
}

// ---- LDS -> global: one contiguous range, staged at the misalignment of its global address ----------------------
template <int U> __device__ __forceinline__ void copy_unit(char* g, const char* s)
{
	if (U == 2) { *(uint16_t*)g = *(const uint16_t*)s; }
	else if (U == 4) { *(uint32_t*)g = *(const uint32_t*)s; }
	else { *(uint2*)g = *(const uint2*)s; }
}
// g: U-aligned global address of the range, stage: 16-byte aligned LDS holding the range at offset (g & 15), nbytes: multiple of U
template <int U> __device__ __forceinline__ void copy_out(char* g, const char* stage, uint32_t nbytes, uint32_t t)
{
	const uint32_t mis = (uint32_t)((uintptr_t)g & 15u);
	uint32_t head = mis ? 16u - mis : 0u;
	if (head > nbytes) { head = nbytes; }
	const char* s = stage + mis;
	if (t < head / U) { copy_unit<U>(g + t * U, s + t * U); }
	const uint32_t nchunks = (nbytes - head) >> 4;
	for (uint32_t c = t; c < nchunks; c += VGX_TEXT_TILE) { *(uint4*)(g + head + 16u * c) = *(const uint4*)(s + head + 16u * c); }
	const uint32_t tailOff = head + (nchunks << 4);
	const uint32_t u = VGX_TEXT_TILE - 1u - t; // the tail's few units go to the lanes the head did not use
	if (u < (nbytes - tailOff) / U) { copy_unit<U>(g + tailOff + u * U, s + tailOff + u * U); }
}

// ---- per tile --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void text_tile(const VgxTextArgs& A, uint64_t tile)
{
	__shared__ uint32_t sStart[VGX_TEXT_RT]; // tile-local first quad of the runs that may hold quads of the tile
	__shared__ uint4 sPos[VGX_TEXT_TILE * 2 + 1], sCol[VGX_TEXT_TILE + 1], sUv[VGX_TEXT_TILE * 2 + 1], sIdx[(VGX_TEXT_TILE * 12) / 16 + 1];
	__shared__ uint64_t sRange[2];
	const uint32_t t = threadIdx.x;
	const uint64_t q0 = tile * VGX_TEXT_TILE;
	const uint32_t nq = A.nquads - q0 < VGX_TEXT_TILE ? (uint32_t)(A.nquads - q0) : VGX_TEXT_TILE;
	const uint64_t qEnd = q0 + nq;

	// the quad of this lane: two 16-byte loads
	float q[8];
	if (t < nq) {
		const float4 a = *(const float4*)(A.quads + 8 * (q0 + t)), b = *(const float4*)(A.quads + 8 * (q0 + t) + 4);
		q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
	}

	// runs [rLo, rEnd) may hold quads of the tile: rLo = the last run that begins at or before the tile's first quad (run 0 when none
	// does), rEnd = behind the last run that begins inside the tile
	uint64_t rLo, rEnd;
	if (A.tile_run) {
		rLo = A.tile_run[tile];
		if (rLo >= A.nruns) { rLo = A.nruns - 1; }
		rEnd = A.nruns;
		if (qEnd < A.nquads) { rEnd = (uint64_t)A.tile_run[tile + 1] + 1; if (rEnd > A.nruns) { rEnd = A.nruns; } }
		if (rEnd <= rLo) { rEnd = rLo + 1; }
	} else {
		if (t == 0) {
			uint64_t lo = 0, hi = A.nruns;
			while (hi - lo > 1) {
				const uint64_t mid = (lo + hi) >> 1;
				if (A.runs[mid].first_quad <= q0) { lo = mid; } else { hi = mid; }
			}
			uint64_t a = lo, b = A.nruns;
			while (b - a > 1) {
				const uint64_t mid = (a + b) >> 1;
				if (A.runs[mid].first_quad < qEnd) { a = mid; } else { b = mid; }
			}
			sRange[0] = lo; sRange[1] = b;
		}
		__syncthreads();
		rLo = sRange[0]; rEnd = sRange[1];
	}
	const uint64_t nr = rEnd - rLo;
	const bool table = nr <= VGX_TEXT_RT; // else (hundreds of empty runs inside one tile): the lanes search in memory
	if (table) {
		for (uint32_t i = t; i < (uint32_t)nr; i += VGX_TEXT_TILE) {
			const uint64_t fq = A.runs[rLo + i].first_quad;
			sStart[i] = fq <= q0 ? 0u : (fq - q0 > 0xFFFFFFFEull ? 0xFFFFFFFFu : (uint32_t)(fq - q0));
		}
		__syncthreads();
	}

	// the run of this lane's quad: the last one that begins at or before it
	uint64_t r = rLo;
	if (t < nq) {
		if (table) {
			uint32_t lo = 0, hi = (uint32_t)nr;
			while (hi - lo > 1) {
				const uint32_t mid = (lo + hi) >> 1;
				if (sStart[mid] <= t) { lo = mid; } else { hi = mid; }
			}
			r = rLo + lo;
		} else {
			uint64_t lo = rLo, hi = rEnd;
			while (hi - lo > 1) {
				const uint64_t mid = (lo + hi) >> 1;
				if (A.runs[mid].first_quad <= q0 + t) { lo = mid; } else { hi = mid; }
			}
			r = lo;
		}
	}
	const vgx_text_run run = A.runs[r]; // the lanes of a run read the same 80 bytes
	float m[6];
	const bool ok = vgx_text_run_status(run, m) == VGX_OK && vgx_text_run_fits(run, A.cap_vertices, A.cap_indices);
	const uint64_t local = q0 + t >= run.first_quad ? q0 + t - run.first_quad : ~0ull;
	const bool covered = t < nq && ok && local < run.num_quads;
	const uint64_t V = covered ? run.first_vertex + 4 * local : 0ull, I = covered ? run.first_index + 6 * local : 0ull;

	// dense tile? every quad is written and lies directly behind its predecessor in the vertex and in the index stream
	const uint64_t fq0 = A.runs[rLo].first_quad;
	const uint64_t V0 = A.runs[rLo].first_vertex + 4 * (q0 - fq0), I0 = A.runs[rLo].first_index + 6 * (q0 - fq0);
	const bool follows = t >= nq || (covered && fq0 <= q0 && V == V0 + 4ull * t && I == I0 + 6ull * t);
	const bool dense = __syncthreads_and(follows ? 1 : 0) != 0;

	float p[8];
	uint32_t uvw[4] = { 0, 0, 0, 0 };
	float uvf[8];
	uint16_t ix[6];
	if (covered) {
		vgx_text_quad_pos(q, m, p);
		if (A.uv_bytes == 4) { vgx_text_quad_uv16(q, uvw); } else { vgx_text_quad_uvf(q, uvf); }
		vgx_text_quad_idx((uint32_t)local, ix);
	}
	if (!dense) { // edge path
		if (!covered) { return; }
		float2* gp = (float2*)(A.pos + 2 * V);
		for (int k = 0; k < 4; ++k) { gp[k] = make_float2(p[2 * k], p[2 * k + 1]); A.color[V + k] = run.color; }
		if (A.uv && A.uv_bytes == 4) { uint32_t* gu = (uint32_t*)A.uv + V; for (int k = 0; k < 4; ++k) { gu[k] = uvw[k]; } }
		else if (A.uv) { float2* gu = (float2*)A.uv + V; for (int k = 0; k < 4; ++k) { gu[k] = make_float2(uvf[2 * k], uvf[2 * k + 1]); } }
		uint16_t* gi = A.idx + I;
		for (int k = 0; k < 6; ++k) { gi[k] = ix[k]; }
		return;
	}
	char* gPos = (char*)(A.pos + 2 * V0);
	char* gCol = (char*)(A.color + V0);
	char* gIdx = (char*)(A.idx + I0);
	char* gUv = A.uv ? (char*)A.uv + V0 * A.uv_bytes : nullptr;
	if (t < nq) {
		float2* sp = (float2*)((char*)sPos + ((uintptr_t)gPos & 15u) + 32u * t);
		uint32_t* sc = (uint32_t*)((char*)sCol + ((uintptr_t)gCol & 15u) + 16u * t);
		uint16_t* si = (uint16_t*)((char*)sIdx + ((uintptr_t)gIdx & 15u) + 12u * t);
		for (int k = 0; k < 4; ++k) { sp[k] = make_float2(p[2 * k], p[2 * k + 1]); sc[k] = run.color; }
		for (int k = 0; k < 6; ++k) { si[k] = ix[k]; }
		if (gUv && A.uv_bytes == 4) { uint32_t* su = (uint32_t*)((char*)sUv + ((uintptr_t)gUv & 15u) + 16u * t); for (int k = 0; k < 4; ++k) { su[k] = uvw[k]; } }
		else if (gUv) { float2* su = (float2*)((char*)sUv + ((uintptr_t)gUv & 15u) + 32u * t); for (int k = 0; k < 4; ++k) { su[k] = make_float2(uvf[2 * k], uvf[2 * k + 1]); } }
	}
	__syncthreads();
	copy_out<8>(gPos, (const char*)sPos, 32u * nq, t);
	copy_out<4>(gCol, (const char*)sCol, 16u * nq, t);
	if (gUv && A.uv_bytes == 4) { copy_out<4>(gUv, (const char*)sUv, 16u * nq, t); }
	else if (gUv) { copy_out<8>(gUv, (const char*)sUv, 32u * nq, t); }
	copy_out<2>(gIdx, (const char*)sIdx, 12u * nq, t);
}

__global__ __launch_bounds__(256) void k_text_runs(VgxTextArgs A)
{
	text_run_records(A, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// withRuns: the frame-sized call, one launch does both halves (the tile half then finds its first run by a search)
__global__ __launch_bounds__(256) void k_text_quads(VgxTextArgs A, int withRuns)
{
	if (withRuns) { text_run_records(A, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x); }
	if (A.nruns == 0 || (uint64_t)blockIdx.x * VGX_TEXT_TILE >= A.nquads) { return; }
	text_tile(A, blockIdx.x);
}

} // namespace

void vgx_launch_text_quads(const VgxTextArgs& a, hipStream_t s)
{
	const uint64_t ntiles = (a.nquads + VGX_TEXT_TILE - 1) / VGX_TEXT_TILE;
	const uint64_t runBlocks = (a.nruns + 255) / 256;
	if (!a.tile_run) {
		uint64_t g = ntiles > runBlocks ? ntiles : runBlocks;
		if (g == 0) { g = 1; }
		hipLaunchKernelGGL(k_text_quads, dim3((uint32_t)g), dim3(256), 0, s, a, 1);
		return;
	}
	hipLaunchKernelGGL(k_text_runs, dim3((uint32_t)(runBlocks > 1024 ? 1024 : (runBlocks ? runBlocks : 1))), dim3(256), 0, s, a); // grid-stride over the runs
	if (ntiles) { hipLaunchKernelGGL(k_text_quads, dim3((uint32_t)ntiles), dim3(256), 0, s, a, 0); }
}
