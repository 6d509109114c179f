// vgx_cmd_bounds.hip -- per-command bounding boxes of a draw-command table on gfx950 (include/vgx.h: vgx_command_bounds; the rules:
// vgx_cmd_bounds.h).
//
// vgx_mesh_bounds spreads its work by VERTEX, which needs ascending, disjoint vertex ranges. A command table promises neither, and a
// command's box is over the corners of its TRIANGLES (an unreferenced vertex, and a triangle with an index outside the command, take no
// part). So this family works on chunks of 64 consecutive triangles of one command, as k_pickc_tris does:
//   scan OpCmdBounds every command's first chunk among those of the range, the chunk total and the count of invalid records; store()
//                    also lays the empty box, as order-preserving images (vgx_bounds.h), into every entry of the range -- the
//                    initialising pass; finish() decides dev_status
//   k_cmdb_tris      fixed grid, one WAVE per chunk, the chunks of a wave contiguous (VgxChunkWalk, vgx_raster_cmds.h). A lane loads
//                    three indices and three positions; a wave reduction over the corners gives the chunk's box, which joins a running
//                    box kept wave-uniform across the chunks of one command. The running box is flushed once per (wave, command) with
//                    four atomicMin / atomicMax on the images: integer minima and maxima, so neither the order nor the decomposition
//                    of the work shows in the result
//   k_cmdb_decode    images -> floats, in place, over the range only
// The caller's `bounds` array is the only box table; the context holds the prefix.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_cmd_bounds.h"

namespace {

struct OpCmdBounds
{
	VgxCmdBoundsArgs A;
	__device__ uint64_t size() const { return vgx_cmdb_range(vgx_real_cmds(A.num_cmds, A.dev_num_cmds), A.cmd_begin, A.cmd_end); }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const vgx_raster_cmd c = A.cmds[A.cmd_begin + i];
		const bool valid = vgx_cmdb_valid(c, A.num_vertices, A.num_indices);
		r.a = valid ? vgx_rasterc_chunks(c) : 0u;
		r.c = valid ? 0u : 1u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		A.cmd_first[i] = e.a;
		((uint4*)A.bounds)[A.cmd_begin + i] = make_uint4(VGX_ORD_POS_INF, VGX_ORD_POS_INF, VGX_ORD_NEG_INF, VGX_ORD_NEG_INF);
	}
	__device__ void finish(Sum3 t) const
	{
		const uint64_t n = size();
		A.cmd_first[n] = t.a;
		A.state[VGX_CMDB_CHUNKS] = t.a; A.state[VGX_CMDB_CMDS] = n;
		if (A.status) { *A.status = t.c ? (uint32_t)VGX_E_INVALID_ARG : (uint32_t)VGX_OK; }
	}
};

// minimum / maximum of the images over the wave, on every lane, as scalars
__device__ __forceinline__ VgxOrdBox cmdb_wave_reduce(VgxOrdBox b)
{
	b.minx = wave_uniform_u32(wave_min_u32(b.minx)); b.miny = wave_uniform_u32(wave_min_u32(b.miny));
	b.maxx = wave_uniform_u32(wave_max_u32(b.maxx)); b.maxy = wave_uniform_u32(wave_max_u32(b.maxy));
	return b;
}

// the running box of (wave, command) into the command's entry; a box nothing joined is the entry's own start and is not sent
__device__ __forceinline__ void cmdb_flush(uint32_t* entry, VgxOrdBox b, int lane)
{
	if (lane != 0 || (b.minx == VGX_ORD_POS_INF && b.maxx == VGX_ORD_NEG_INF && b.miny == VGX_ORD_POS_INF && b.maxy == VGX_ORD_NEG_INF)) { return; }
	atomicMin(entry + 0, b.minx); atomicMin(entry + 1, b.miny); atomicMax(entry + 2, b.maxx); atomicMax(entry + 3, b.maxy);
}

__global__ __launch_bounds__(256) void k_cmdb_tris(VgxCmdBoundsArgs A)
{
	const uint64_t total = A.state[VGX_CMDB_CHUNKS];
	const uint32_t n = (uint32_t)A.state[VGX_CMDB_CMDS]; // the commands of the range; command i of it is cmds[cmd_begin + i]
	const int lane = threadIdx.x & (VGX_WAVE - 1);
	VgxChunkWalk W(A.cmd_first, n, total, (uint64_t)blockIdx.x * (blockDim.x / VGX_WAVE) + (threadIdx.x / VGX_WAVE), (uint64_t)gridDim.x * (blockDim.x / VGX_WAVE)); // a contiguous run of the chunks; command W.c of the range is cmds[cmd_begin + W.c]
	if (W.k0 >= W.k1) { return; }
	vgx_raster_cmd cmd = A.cmds[A.cmd_begin + W.c];
	VgxOrdBox run = vgx_ordbox_empty();
	for (uint64_t k = W.k0; k < W.k1; ++k) {
		const uint32_t left = W.c;
		if (W.advance(k)) {
			cmdb_flush(A.bounds + 4ull * (A.cmd_begin + left), run, lane);
			run = vgx_ordbox_empty();
			cmd = A.cmds[A.cmd_begin + W.c];
		}
		// inside the command's ranges, and those inside the streams: OpCmdBounds gave an invalid record no chunks
		const VgxOrdBox b = vgx_cmdb_triangle(cmd, A.idx, A.pos, (uint32_t)(k - W.first) * VGX_RASTERC_CHUNK + (uint32_t)lane);
		run = vgx_ordbox_union(run, cmdb_wave_reduce(b));
	}
	cmdb_flush(A.bounds + 4ull * (A.cmd_begin + W.c), run, lane);
}

__global__ __launch_bounds__(256) void k_cmdb_decode(VgxCmdBoundsArgs A)
{
	const uint64_t n = A.state[VGX_CMDB_CMDS];
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		uint4* const e = (uint4*)A.bounds + A.cmd_begin + i;
		const uint4 o = *e;
		float4 r;
		r.x = vgx_float_from_ord(o.x); r.y = vgx_float_from_ord(o.y); r.z = vgx_float_from_ord(o.z); r.w = vgx_float_from_ord(o.w);
		*(float4*)e = r;
	}
}

} // namespace

void vgx_launch_command_bounds(const VgxCmdBoundsArgs& a, void* partial, uint32_t grid, hipStream_t s)
{
	const uint32_t range = vgx_cmdb_range(a.num_cmds, a.cmd_begin, a.cmd_end); // an upper bound of the range: the real count lives on the device
	const OpCmdBounds op = { a };
	vgx_device_scan(op, (Sum3*)partial, s, range); // an empty range too: it leaves the totals and the status
	if (!range) { return; }
	hipLaunchKernelGGL(k_cmdb_tris, dim3(grid), dim3(256), 0, s, a);
	const uint32_t blocks = (range + 255u) / 256u;
	hipLaunchKernelGGL(k_cmdb_decode, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, s, a);
}
