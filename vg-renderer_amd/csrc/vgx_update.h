// vgx_update.h -- the arithmetic of vgx_cache_layout and vgx_cache_update for ONE instance, ONE listed entry and ONE mesh: host + device.
// The scan of vgx_cache_submit (OpCacheInst, vgx_api.hip), the kernels of vgx_update.hip and libvgx_hosttest.so (vgx_hosttest.cpp) all
// call these functions, so the offsets vgx_cache_layout hands out are the ones vgx_cache_submit writes to by construction, and the CPU
// suite pins the rules of an update without a GPU.
#ifndef VGX_UPDATE_H
#define VGX_UPDATE_H

#include "vgx_lane.h"

// ---- one instance's share of a frame -----------------------------------------------------------------------------------
// First vertex / index of cache mesh k; k == num_meshes names the end of the streams.
VGX_HD uint64_t vgx_cache_first_vertex(const vgx_cache_desc& c, uint64_t k) { return k < c.num_meshes ? c.meshes[k].first_vertex : c.num_vertices; }
VGX_HD uint64_t vgx_cache_first_index(const vgx_cache_desc& c, uint64_t k) { return k < c.num_meshes ? c.meshes[k].first_index : c.num_indices; }

struct VgxRangeCounts { uint64_t meshes, vertices, indices; };

// Meshes, vertices and indices of the mesh range of `in`. A range outside the cache contributes nothing: false, and *r is left as it was.
VGX_HD bool vgx_cache_range_counts(const vgx_cache_desc& c, const vgx_cache_instance& in, VgxRangeCounts* r)
{
	if (in.first_mesh > c.num_meshes || (uint64_t)in.num_meshes > c.num_meshes - in.first_mesh) { return false; }
	r->meshes = in.num_meshes;
	r->vertices = vgx_cache_first_vertex(c, in.first_mesh + in.num_meshes) - vgx_cache_first_vertex(c, in.first_mesh);
	r->indices = vgx_cache_first_index(c, in.first_mesh + in.num_meshes) - vgx_cache_first_index(c, in.first_mesh);
	return true;
}

// ---- one listed entry of vgx_cache_update ------------------------------------------------------------------------------
// The checks of include/vgx.h in their order. Bits of the call's flag word; the status follows from the OR over the list, so it does
// not depend on the order in which the entries are looked at.
#define VGX_UPD_INVALID 1u
#define VGX_UPD_STALE 2u

// 0: the slice of instance d is rewritten and *r holds its sizes; else VGX_UPD_INVALID or VGX_UPD_STALE and *r is zero.
VGX_HD uint32_t vgx_update_classify(const vgx_cache_desc& c, const vgx_cache_instance* inst, uint64_t ninst, const vgx_cache_slot* slots,
                                    uint64_t d, uint64_t frameVertices, uint64_t frameMeshes, VgxRangeCounts* r)
{
	r->meshes = 0; r->vertices = 0; r->indices = 0;
	if (d >= ninst) { return VGX_UPD_INVALID; }
	const vgx_cache_instance in = inst[d];
	VgxRangeCounts n = { 0, 0, 0 };
	if (!vgx_cache_range_counts(c, in, &n)) { return VGX_UPD_INVALID; }
	const vgx_cache_slot s0 = slots[d], s1 = slots[d + 1];
	if (in.first_mesh != s0.cache_first_mesh || n.meshes != s1.first_mesh - s0.first_mesh || n.vertices != s1.first_vertex - s0.first_vertex) {
		return VGX_UPD_STALE;
	}
	if (s1.first_vertex > frameVertices || s1.first_mesh > frameMeshes) { return VGX_UPD_INVALID; }
	*r = n;
	return 0u;
}

VGX_HD int vgx_update_status(uint32_t flags)
{
	return (flags & VGX_UPD_INVALID) ? VGX_E_INVALID_ARG : ((flags & VGX_UPD_STALE) ? VGX_E_STALE : VGX_OK);
}

// ---- one mesh of an updated instance -----------------------------------------------------------------------------------
// Meshes cached without per-vertex colours (the non-AA flavours) are drawn with the instance's colour (vgx_cache.hip).
VGX_HD bool vgx_mesh_takes_instance_colour(uint32_t subpathKind)
{
	const uint32_t kind = subpathKind >> 28;
	return kind == VGX_MESH_FILL || kind == VGX_MESH_STROKE;
}

// Where the vertices of cache mesh `src` sit inside the slice of an instance whose range starts at cache vertex `rangeFirst` and holds
// `sliceVertices` vertices: offset and count, clipped to the slice so that no table can lead outside it.
VGX_HD uint32_t vgx_update_mesh_span(const vgx_mesh& src, uint64_t rangeFirst, uint64_t sliceVertices, uint64_t* offset)
{
	const uint64_t off = src.first_vertex - rangeFirst;
	*offset = off;
	if (src.first_vertex < rangeFirst || off >= sliceVertices) { return 0u; }
	const uint64_t left = sliceVertices - off;
	return (uint64_t)src.num_vertices < left ? src.num_vertices : (uint32_t)left;
}

#endif
