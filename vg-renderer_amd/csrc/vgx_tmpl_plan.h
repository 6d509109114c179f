// vgx_tmpl_plan.h -- template mode, the host's decisions (compiles without HIP: tests/native/tmpl_plan_test.cpp), and the tile-boundary
// arithmetic the build kernels share with the host (tests/native/tmpl_tiles_test.cpp).
//
// What vgx_tessellate_count decides on the host between the kernels of vgx_tmpl.hip: which instances share a class, which emit
// kernel and tile size a template gets, the sizes of one instance of every class, and the batch's totals and tables. This is the
// ONE place where a kernel kind or a tile rule is defined; vgx_tmpl.hip and vgx_api.hip use the enums below.
#ifndef VGX_TMPL_PLAN_H
#define VGX_TMPL_PLAN_H

#include <stdint.h>
#include <string.h>
#include <stddef.h>
#include <vector>
#include <unordered_map>
#include "vgx_internal_types.h"

#ifndef VGX_TMPL_MAX_TILE
#define VGX_TMPL_MAX_TILE 2048 /* elements per tile = per workgroup (what its LDS stages hold); a multiple of VGX_TMPL_THREADS. Tiger x10k, same
                                * box: 256 threads x 1024 elements 2.18 ms, 512 x 2048 2.06, 512 x 3072 2.15, 1024 x 4096 2.15, 128 x 1024 2.26 */
#endif
#ifndef VGX_TMPL_RC_TILE
#define VGX_TMPL_RC_TILE 2048   /* k_tmpl_emit_round_aa / _open (VGX_TMPL_RC_THREADS threads per workgroup): elements per tile */
#endif
#ifndef VGX_TMPL_GENERAL_TILE
#define VGX_TMPL_GENERAL_TILE 2048 /* tile size of templates that hold general strokes (the LDS stages of k_tmpl_emit_general) */
#endif

// ---- stroke styles and kernel kinds ----------------------------------------------------------------------------------------
// Which stroke meshes the template holds that are NOT closed Miter AA / Thin strokes (those and fills are every kernel's):
// k_tmpl_styles ORs these into the class table's style word (VGX_TMPL_STYLES).
enum VgxTmplStyle : uint32_t
{
	VGX_TS_OPEN_MITER = 1u,       // open Miter strokes with Butt / Square caps (tmpl_stroke_elem_open)
	VGX_TS_OTHER = 2u,            // any other non-simple stroke (the general element body)
	VGX_TS_ROUND = 4u,            // Round joins: sizes counted per instance and step (set beside one of the other bits)
	VGX_TS_CLOSED_BEVEL = 8u,     // closed Bevel AA / Thin strokes (tmpl_stroke_elem_bevel)
	VGX_TS_ROUND_AA_CLOSED = 16u, // closed AA strokes with Round joins (tmpl_stroke_elem_round)
	VGX_TS_ROUND_AA_OPEN = 32u    // open AA strokes with Round joins
};
// The instantiation of the emit kernel a template needs (VgxTmplArgs::kernel), each named for its kernel.
enum VgxTmplKernel : uint32_t
{
	VGX_TK_EMIT = 0,          // k_tmpl_emit: fills, closed Miter AA / Thin strokes only (the headline's kernel)
	VGX_TK_OPEN = 1,          // k_tmpl_emit_open: + open Miter strokes with Butt / Square caps
	VGX_TK_GENERAL = 2,       // k_tmpl_emit_general: any stroke without Round joins (the general body)
	VGX_TK_ROUND = 3,         // k_tmpl_emit_round: the general body + Round joins
	VGX_TK_BEVEL = 4,         // k_tmpl_emit_bevel: closed Miter + closed Bevel strokes only
	VGX_TK_ROUND_AA = 5,      // k_tmpl_emit_round_aa: closed Miter / Bevel + closed AA strokes with Round joins
	VGX_TK_ROUND_AA_OPEN = 6  // k_tmpl_emit_round_aa_open: ... + open AA strokes with Round joins
};

inline VgxTmplKernel vgx_tmpl_kernel_for(uint32_t styles)
{
	if (styles & VGX_TS_ROUND) {
		if (styles & (VGX_TS_OPEN_MITER | VGX_TS_OTHER)) { return VGX_TK_ROUND; } // (non-AA Round joins are VGX_TS_OTHER)
		return (styles & VGX_TS_ROUND_AA_OPEN) ? VGX_TK_ROUND_AA_OPEN : VGX_TK_ROUND_AA;
	}
	if (styles & VGX_TS_OTHER) { return VGX_TK_GENERAL; }
	if (styles & VGX_TS_CLOSED_BEVEL) { return (styles & VGX_TS_OPEN_MITER) ? VGX_TK_GENERAL : VGX_TK_BEVEL; } // a kernel of their own beside closed Miter ones only
	return (styles & VGX_TS_OPEN_MITER) ? VGX_TK_OPEN : VGX_TK_EMIT;
}
// Round joins: vertices / indices are the instances' own, counted on the device by the sizes pass of every step
inline bool vgx_tmpl_kernel_is_round(VgxTmplKernel k) { return k == VGX_TK_ROUND || k == VGX_TK_ROUND_AA || k == VGX_TK_ROUND_AA_OPEN; }
// elements per tile; optTile: the context's option (VGX_TMPL_MAX_TILE unless VGX_TMPL_TILE overrides it)
inline uint32_t vgx_tmpl_tile_for(VgxTmplKernel k, uint32_t optTile)
{
	if ((k == VGX_TK_GENERAL || k == VGX_TK_ROUND) && optTile > VGX_TMPL_GENERAL_TILE) { return (uint32_t)VGX_TMPL_GENERAL_TILE; }
	if ((k == VGX_TK_ROUND_AA || k == VGX_TK_ROUND_AA_OPEN) && optTile == VGX_TMPL_MAX_TILE) { return VGX_TMPL_RC_TILE; } // (its own workgroup shape; an override stands)
	return optTile;
}

// ---- which elements a tile owns ------------------------------------------------------------------------------------------------
// The tile size T above is the SLOT size of the element table (tile t's slots are [t * T, t * T + nel)) and the capacity of the emit
// kernel's LDS stages. A tile's elements are cut out of its class's output-ordered element stream [elem0, end) at boundaries that avoid
// the short meshes: boundary k is nominally elem0 + k * S (the stride S a little below T) and, when that falls strictly inside a mesh of
// at most L = T / 8 elements, moves DOWN to that mesh's first element -- such a mesh lies whole in one tile, so none of its elements has
// a neighbour in another tile (no load behind the emit kernel's first barrier). A longer mesh is cut where the boundary falls.
// With Lmax = the longest mesh of the class of at most L elements (1: none) and S = T - (Lmax - 1): a boundary moves by at most
// Lmax - 1, so a tile holds at most S + Lmax - 1 = T elements, boundaries stay strictly increasing (S - Lmax + 1 > 0), every
// boundary is found on its own (no pass over the meshes in order), and the class has ceil(E / S) tiles.
// These are the lines k_tmpl_mesh_lmax / k_tmpl_classes / k_tmpl_elems (vgx_tmpl.hip) run; tests/native/tmpl_tiles_test.cpp runs them on the host.
#if defined(__HIPCC__)
#define VGX_TMPL_HD __host__ __device__
#else
#define VGX_TMPL_HD
#endif
VGX_TMPL_HD inline uint32_t vgx_tmpl_snap_limit(uint32_t T) { return T / 8u; }
// a mesh's contribution to Lmax (the maximum over the class's meshes; 0: the mesh is a long one)
VGX_TMPL_HD inline uint32_t vgx_tmpl_snap_len(uint64_t meshLen, uint32_t T) { return meshLen <= (uint64_t)vgx_tmpl_snap_limit(T) ? (uint32_t)meshLen : 0u; }
VGX_TMPL_HD inline uint32_t vgx_tmpl_stride(uint32_t T, uint32_t lmax) { return T - ((lmax ? lmax : 1u) - 1u); }
VGX_TMPL_HD inline uint64_t vgx_tmpl_tile_count(uint64_t classElems, uint32_t stride) { return (classElems + stride - 1) / stride; }
// boundary k of a class whose elements are [elem0, end), before the snap (k = the tile count: the class's end)
VGX_TMPL_HD inline uint64_t vgx_tmpl_nominal_boundary(uint64_t elem0, uint64_t end, uint64_t k, uint32_t stride)
{
	const uint64_t b = elem0 + k * (uint64_t)stride;
	return b < end ? b : end;
}
// the boundary given the mesh that owns element `nominal`: its first element and its length
VGX_TMPL_HD inline uint64_t vgx_tmpl_snap_boundary(uint64_t nominal, uint64_t meshFirst, uint64_t meshLen, uint32_t T)
{
	return (meshFirst < nominal && meshLen <= (uint64_t)vgx_tmpl_snap_limit(T)) ? meshFirst : nominal;
}
// Small classes -- a drawing of a few thousand meshes, the instanced case -- are packed greedily instead: every boundary as far behind the
// previous one as the slots reach (nominally start + T, then the same snap), which fills the tiles better than the stride does (the
// Tiger: 9 tiles instead of 10). One thread walks the boundaries in order (k_tmpl_classes), hence the limits: a static batch of
// millions of meshes keeps the stride rule, whose boundaries are found independently. Same invariants; the tile count is at most the
// stride rule's (every tile but the last holds more than T - Lmax >= S - 1 elements).
#ifndef VGX_TMPL_GREEDY_MAX_MESHES
#define VGX_TMPL_GREEDY_MAX_MESHES 4096u /* 0: the stride rule for every class (measurement builds) */
#endif
#define VGX_TMPL_GREEDY_MAX_TILES 64u
VGX_TMPL_HD inline bool vgx_tmpl_greedy_class(uint64_t classMeshes, uint64_t classElems, uint32_t T)
{
	return classMeshes <= VGX_TMPL_GREEDY_MAX_MESHES && classElems <= (uint64_t)VGX_TMPL_GREEDY_MAX_TILES * (T - vgx_tmpl_snap_limit(T));
}
VGX_TMPL_HD inline uint64_t vgx_tmpl_greedy_nominal(uint64_t start, uint64_t end, uint32_t T)
{
	const uint64_t b = start + T;
	return b < end ? b : end;
}
// tiles of a template whatever its meshes (what the element table and the build kernels' grids are sized for): every class rounds up on its own
VGX_TMPL_HD inline uint64_t vgx_tmpl_max_tiles(uint64_t elems, uint32_t T, uint32_t nclasses)
{
	return elems / vgx_tmpl_stride(T, vgx_tmpl_snap_limit(T)) + nclasses + 1;
}

// one instance of a class: only the mesh kinds k_tmpl_emit writes, every output stream of the instance below 4 GB
inline bool vgx_tmpl_eligible(const VgxTotals& ht, bool roundOk)
{
	const vgx_sizes& z = ht.sizes;
	return !((ht.num_round_meshes && !roundOk) || z.num_elements == 0 || z.num_elements >= (1ull << 31) || z.num_vertices >= (1ull << 29)
		|| z.num_indices >= (1ull << 31) || z.num_poly_vertices >= (1ull << 32) || z.num_meshes >= (1ull << 32));
}

// ---- classes ---------------------------------------------------------------------------------------------------------------
// Instances of equal hash share a class (candidates: k_tmpl_check_cls compares them bit by bit). Classes are numbered in first-seen
// order, reps[c] = the first instance of class c. False: more than VGX_TMPL_MAX_CLASSES flavours.
inline bool vgx_tmpl_group_classes(const unsigned long long* hashes, uint64_t ninst, std::vector<uint32_t>& instCls, std::vector<uint32_t>& reps)
{
	instCls.assign((size_t)ninst, 0u);
	reps.clear();
	std::unordered_map<unsigned long long, uint32_t> seen;
	for (uint64_t k = 0; k < ninst; ++k) {
		const auto it = seen.find(hashes[k]);
		uint32_t c;
		if (it != seen.end()) { c = it->second; }
		else {
			c = (uint32_t)reps.size();
			if (c == VGX_TMPL_MAX_CLASSES) { return false; }
			seen.emplace(hashes[k], c);
			reps.push_back((uint32_t)k);
		}
		instCls[(size_t)k] = c;
	}
	return true;
}

// Sizes of ONE instance of every class = what the concatenated run holds between the class's first draw and the next class's:
// cls [T + 1] (k_tmpl_classes), csum [T + 1][5] (k_tmpl_class_sums: polyline vertices, sub-paths, command instances, fill
// elements in FRONT of the class; serial draws: entry c + 1 holds class c's OWN count). False: a class beyond vgx_tmpl_eligible.
inline bool vgx_tmpl_class_sizes(const VgxTmplClass* cls, const unsigned long long* csum, uint32_t T, std::vector<vgx_sizes>& csz)
{
	csz.resize(T);
	for (uint32_t c = 0; c < T; ++c) {
		VgxTotals one; // the limits of one instance, per class
		memset(&one, 0, sizeof(one));
		vgx_sizes& q = one.sizes;
		q.num_meshes = cls[c + 1].mesh0 - cls[c].mesh0; q.num_elements = cls[c + 1].elem0 - cls[c].elem0;
		q.num_vertices = cls[c + 1].v0 - cls[c].v0; q.num_indices = cls[c + 1].i0 - cls[c].i0;
		const unsigned long long* a0 = &csum[(size_t)c * 5]; const unsigned long long* a1 = &csum[(size_t)(c + 1) * 5];
		q.num_poly_vertices = a1[0] - a0[0]; q.num_subpaths = a1[1] - a0[1]; q.num_cmd_instances = a1[2] - a0[2];
		q.num_fill_elements = a1[3] - a0[3]; q.num_serial_draws = a1[4];
		csz[c] = q;
		if (!vgx_tmpl_eligible(one, false)) { return false; }
	}
	return true;
}

// Round-join elements of one instance of every class and the Round-join meshes of the largest class (the sizes pass's LDS table),
// from the table k_tmpl_round_classes finished; roundMeshes / roundElems: those of the whole template.
inline void vgx_tmpl_round_layout(const VgxTmplClass* cls, uint32_t T, uint32_t roundMeshes, uint32_t roundElems, std::vector<uint64_t>& clsRelems, uint32_t& roundLds)
{
	clsRelems.assign(T, 0);
	clsRelems[0] = roundElems;
	roundLds = roundMeshes;
	if (T == 1) { return; }
	roundLds = 0;
	for (uint32_t c = 0; c < T; ++c) {
		const uint32_t r1 = c + 1 < T ? cls[c + 1].round[VGX_TC_MESH0] : roundMeshes, e1 = c + 1 < T ? cls[c + 1].round[VGX_TC_ELEM0] : roundElems;
		clsRelems[c] = e1 - cls[c].round[VGX_TC_ELEM0];
		if (r1 - cls[c].round[VGX_TC_MESH0] > roundLds) { roundLds = r1 - cls[c].round[VGX_TC_MESH0]; }
	}
}

// ---- the batch: instances x their class's sizes ------------------------------------------------------------------------------
inline void vgx_tmpl_add_instances(vgx_sizes& z, uint64_t n, const vgx_sizes& q) // z += n instances of sizes q (no draw commands: assembly's)
{
	z.num_poly_vertices += n * q.num_poly_vertices; z.num_subpaths += n * q.num_subpaths; z.num_meshes += n * q.num_meshes;
	z.num_vertices += n * q.num_vertices; z.num_indices += n * q.num_indices; z.num_serial_draws += n * q.num_serial_draws;
	z.num_cmd_instances += n * q.num_cmd_instances; z.num_elements += n * q.num_elements; z.num_fill_elements += n * q.num_fill_elements;
}

struct VgxTmplWg { uint32_t inst, tile; }; // one workgroup of a step: tile `tile` (of the concatenated template) of instance `inst`
struct VgxTmplPlan
{
	std::vector<uint64_t> cnt;     // instances per class
	vgx_sizes total;               // sizes of the whole batch
	uint64_t numWg;                // workgroups of one step
	uint64_t relemWords;           // Round-join table words of the whole batch
	std::vector<VgxTmplInst> inst; // several classes: [ninst + 1], the last entry = the totals
	std::vector<VgxTmplWg> wg;     // several classes: [numWg]
};

// cnt, total, numWg, relemWords. instCls / clsRelems: null for one class / no Round joins. False (several classes only): beyond
// the emit kernel's grid or the 32-bit mesh numbers of VgxTmplInst -- the ordinary pipeline.
inline bool vgx_tmpl_plan_totals(const vgx_sizes* csz, const VgxTmplClass* cls, uint32_t T, uint64_t ninst, const uint32_t* instCls, const uint64_t* clsRelems, VgxTmplPlan& p)
{
	p.cnt.assign(T, 0);
	if (T == 1) { p.cnt[0] = ninst; } else { for (uint64_t k = 0; k < ninst; ++k) { ++p.cnt[instCls[k]]; } }
	memset(&p.total, 0, sizeof(p.total));
	p.numWg = 0; p.relemWords = 0;
	for (uint32_t c = 0; c < T; ++c) {
		vgx_tmpl_add_instances(p.total, p.cnt[c], csz[c]);
		p.numWg += p.cnt[c] * (uint64_t)(cls[c + 1].tile0 - cls[c].tile0);
		if (clsRelems) { p.relemWords += p.cnt[c] * clsRelems[c]; }
	}
	return T == 1 || !(p.numWg > 0x7FFFFFFFull || p.total.num_meshes >= (1ull << 32));
}

// The totals above and, for several classes, the two tables of a step.
inline bool vgx_tmpl_plan_batch(const vgx_sizes* csz, const VgxTmplClass* cls, uint32_t T, uint64_t ninst, const uint32_t* instCls, const uint64_t* clsRelems, VgxTmplPlan& p)
{
	p.inst.clear(); p.wg.clear();
	if (!vgx_tmpl_plan_totals(csz, cls, T, ninst, instCls, clsRelems, p)) { return false; }
	if (T == 1) { return true; }
	p.inst.resize((size_t)ninst + 1);
	p.wg.resize((size_t)p.numWg);
	uint64_t v = 0, i = 0, m = 0, w = 0, re = 0;
	for (uint64_t k = 0; k <= ninst; ++k) {
		VgxTmplInst r;
		memset(&r, 0, sizeof(r));
		r.v = v; r.i = i; r.m = (uint32_t)m;
		if (k < ninst) {
			const uint32_t c = instCls[k];
			r.cls = c; r.cmesh0 = cls[c].mesh0;
			r.rel = clsRelems ? re - (uint64_t)cls[c].round[VGX_TC_ELEM0] : 0ull; // (the element numbers in the mesh records run over the whole template)
			v += csz[c].num_vertices; i += csz[c].num_indices; m += csz[c].num_meshes; re += clsRelems ? clsRelems[c] : 0;
		}
		p.inst[(size_t)k] = r;
	}
	// Workgroup order: class after class (the instances of a class in draw order). The output places are the instances' own
	// whatever the order; running one class's instances together keeps ONE class's tables hot in L2 instead of all of them
	// (instances in draw order: 3.9 GB of table re-reads from HBM for Tiger x 10k in 18 classes).
	std::vector<uint64_t> cursor(T, 0);
	for (uint32_t c = 0; c < T; ++c) { cursor[c] = w; w += p.cnt[c] * (uint64_t)(cls[c + 1].tile0 - cls[c].tile0); }
	for (uint64_t k = 0; k < ninst; ++k) {
		const uint32_t c = instCls[k];
		for (uint32_t t = cls[c].tile0; t < cls[c + 1].tile0; ++t) { const VgxTmplWg e = { (uint32_t)k, t }; p.wg[(size_t)cursor[c]++] = e; }
	}
	return true;
}

#endif
