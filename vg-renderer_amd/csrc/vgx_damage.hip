// vgx_damage.hip -- marking the tiles an edit can have changed, on gfx950 (include/vgx.h: vgx_damage_meshes, vgx_damage_instances; the
// rule: vgx_damage.h). The marks feed vgx_raster_damaged (vgx_raster.hip), which redraws the marked tiles alone.
//
// vgx_damage_meshes     k_damage_meshes: one lane per mesh of the range: box -> rectangle of tiles -> mark_tiles, one atomicOr per
//                       32-tile word per tile row, the form the raster's class bitmaps are filled in.
// vgx_damage_instances  a listed instance is one drawing of 435 meshes or a one-mesh instance, and the list holds one entry or a hundred
//                       thousand, so the work is spread by MESH of the listed entries, not by entry, as vgx_cache_update's is:
//   scan OpDamageList   one item per listed entry: the check of vgx_damage_entry, the exclusive sum of the mesh counts of the entries
//                       that pass (the others count nothing and are never walked), the status from the flag word
//   k_damage_instances  one lane per item of the "dirty mesh" space, grid-stride: the lane finds its entry by search in the prefix
//                       (which skips entries that count nothing), then marks as above.
// Duplicates mark the same bits twice; an OR depends neither on the order nor on the number of times. The bitmap is only ORed into.
// Bounds of every atomic: vgx_damage_box_tiles cuts the rectangle to the image, so every bit is < tiles_w * tiles_h; a mesh index is
// inside the table by vgx_damage_entry (slots[d + 1].first_mesh <= num_meshes) or by the host's cut of the range.
#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_scan.h"
#include "vgx_damage.h"

namespace {

__device__ __forceinline__ void damage_mark(const VgxDamageArgs& A, uint64_t m)
{
	const float4 box = ((const float4*)A.mesh_bounds)[m];
	const float b[4] = { box.x, box.y, box.z, box.w };
	VgxRasterRect r;
	if (vgx_damage_box_tiles(b, A.x0, A.y0, A.width, A.height, &r)) { mark_tiles(A.tile_bits, r, A.tiles_w); }
}

__global__ __launch_bounds__(256) void k_damage_meshes(VgxDamageArgs A)
{
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k < A.nrange) { damage_mark(A, A.mesh_begin + k); }
}

__device__ __forceinline__ uint64_t damage_list_size(const VgxDamageArgs& A)
{
	if (!A.dev_ndirty) { return A.ndirty; }
	const uint64_t n = *A.dev_ndirty;
	return n < A.ndirty ? n : A.ndirty;
}

struct OpDamageList
{
	VgxDamageArgs A;
	__device__ uint64_t size() const { return damage_list_size(A); }
	__device__ Sum3 load(uint64_t j) const
	{
		Sum3 r = sum3_zero();
		uint64_t first, count;
		if (!vgx_damage_entry(A.slots, A.ninst, A.num_meshes, A.dirty[j], &first, &count)) { atomicOr(A.flags, 1u); } // rare; as OpUpdateList
		r.a = count;
		return r;
	}
	__device__ void store(uint64_t j, Sum3 e) const { A.mesh_prefix[j] = e.a; }
	__device__ void finish(Sum3 t) const
	{
		A.mesh_prefix[size()] = t.a;
		// every load of the scan lies in front of this call (an earlier kernel, or the block barrier of the single-workgroup form)
		if (A.status) { *A.status = __hip_atomic_load(A.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? (uint32_t)VGX_E_INVALID_ARG : (uint32_t)VGX_OK; }
	}
};

__global__ __launch_bounds__(256) void k_damage_instances(VgxDamageArgs A)
{
	const uint64_t nlist = damage_list_size(A);
	const uint64_t* prefix = A.mesh_prefix;
	const uint64_t total = prefix[nlist];
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += step) {
		const uint64_t j = find_owner_u64(prefix, 0, nlist, q); // the last entry whose first dirty mesh is <= q: the one that owns q
		// (an entry that passed the check at the scan passes it here: the same words are read)
		damage_mark(A, A.slots[A.dirty[j]].first_mesh + (q - prefix[j]));
	}
}

} // namespace

void vgx_launch_damage_meshes(const VgxDamageArgs& a, hipStream_t s)
{
	if (a.nrange) { hipLaunchKernelGGL(k_damage_meshes, dim3((unsigned)((a.nrange + 255) / 256)), dim3(256), 0, s, a); }
}

void vgx_launch_damage_instances(const VgxDamageArgs& a, void* partial, hipStream_t s)
{
	OpDamageList op;
	op.A = a;
	vgx_device_scan_small(op, (Sum3*)partial, s, a.ndirty);
	if (!a.ndirty || !a.num_meshes) { return; }
	// The total stays on the device. The host knows a bound: every listed entry has at most the frame's meshes. Lanes beyond the total
	// leave at once
	const uint64_t big = ~0ull;
	const uint64_t bound = a.ndirty > big / a.num_meshes ? big : a.ndirty * a.num_meshes;
	const uint64_t want = (bound + 255) / 256;
	hipLaunchKernelGGL(k_damage_instances, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, s, a);
}
