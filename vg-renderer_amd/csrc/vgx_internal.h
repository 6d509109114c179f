// vgx_internal.h -- device-side data layout shared by the kernels and the C-ABI implementation.
#ifndef VGX_INTERNAL_H
#define VGX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vgx.h"
#include "vgx_lane.h"

#include "vgx_internal_types.h"
#include "vgx_tmpl_plan.h"

struct VgxFlattenArgs
{
	VgxPathSetDev ps;
	const vgx_draw* draws;
	uint64_t ndraws;
	const uint64_t* cmd_prefix; // [ndraws+1]
	const uint64_t* sub_prefix; // [ndraws+1] exclusive scan of the draws' static sub-path counts: the flatten kernels of vgx_tessellate store their sub-path records
	                            // densely, record j of draw d at sub_rec[sub_prefix[d] + j]
	uint32_t* cmd_cnt;          // [num_cmd_instances]
	vgx_draw_info* dinfo;       // [ndraws]
	float* poly;                // emit: [cap][2]
	vgx_subpath* subs;          // emit
	VgxMeshDesc* mdesc;         // emit (may be null: flatten-only API)
	VgxMeshPrep* mprep;         // single-pass pipeline: per-mesh constants written together with mdesc (else null: k_mesh_prepare does it)
	vgx_mesh* mtab;             // emit: closed-form mesh sizes are written together with mdesc
	VgxTotals* totals;
	VgxCaps caps;
	int apply_transform;
	// BUILD mode (single-pass flatten of vgx_tessellate): per-sub-path records stored sparsely at the command-instance
	// index of the sub-path's last command
	VgxSubRec* sub_rec;            // [>= static sub-paths of the batch] record j of draw d at sub_prefix[d] + j (BUILD mode)
	int build_mode;                // k_flatten_serial<count>: allocate the draw's vertices from the polyline heap
	uint32_t* serial_list;         // BUILD mode: draws for k_flatten_serial (static serial paths + degenerate draws), unordered
	float* leaf_overflow;          // [VGX_BUILD_WAVES][VGX_BUILD_OVERFLOW][64][2] leaves that did not fit the LDS slots
	int thin_static;               // every path of the set is MOVE_TO / LINE_TO / CLOSE only: k_flatten_thin (vgx_thin.h) in k_flatten_build's place
	// instanced batches (vgx_inst.hip): draws[i].path == draws[i % inst_period].path; 0 = not instanced. When set and the
	// device-side check of this call agrees, k_flatten_inst builds the batch and k_flatten_build exits at once.
	uint32_t inst_period;
	uint32_t inst_block;           // vertices per lane-private heap block
	int inst_waves;                // grid of k_flatten_inst
	// grouped mode of k_flatten_inst (draws that share paths in ANY order; null = periodic mode / off): the draws sorted by
	// path (k_inst_hist / k_inst_plan / k_inst_scatter, run by every vgx_tessellate in this mode)
	const uint32_t* inst_order;      // [ndraws] draw indices, grouped by path
	const uint64_t* inst_start;      // [npaths + 1] first entry of every path in inst_order
	const uint64_t* inst_task_start; // [npaths + 1] first task of every path
	const uint32_t* inst_task_path;  // [tasks] path of every task
	// periodic mode, instances of different scales: lane slot k of the instance walk takes instance inst_perm[k] -- the instances
	// sorted by the tolerance class of their first draw, so that the lanes of a wave flatten with (nearly) the same tolerance and
	// stay in lock-step. Any permutation is valid (null = identity): it only decides which instances share a wave.
	const uint32_t* inst_perm;       // [ndraws / inst_period]
};

struct VgxStrokeArgs
{
	const vgx_draw* draws;
	const float* poly;
	const VgxMeshDesc* mdesc;
	const uint64_t* elem_prefix; // [num_meshes+1] exclusive prefix of poly_n over the meshes of this kernel's kind class
	const uint64_t* elem_prefix_fill;   // fills only (strokes contribute 0)
	const uint64_t* elem_prefix_stroke; // strokes only
	VgxMeshPrep* mprep;          // [num_meshes]
	vgx_mesh* mtab;              // [num_meshes] count: writes num_*, scan fills first_*, emit reads
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	vgx_mesh* meshes_out;        // caller's mesh table (emit copies mtab into it)
	const uint32_t* mesh_base;   // assembly armed: vertices in front of each mesh inside its vertex buffer (added to every index); else null
	VgxTotals* totals;
	VgxCaps caps;
	int no_long;                 // frame-sized call: k_stroke takes the strokes whatever their length (k_stroke_long is not launched)
	int tile_mode;               // the host also launches k_emit_tiles (vgx_tile.hip): k_fill leaves the batches that kernel takes alone
};


// template mode (vgx_tmpl.hip)
#ifndef VGX_TMPL_THREADS
#define VGX_TMPL_THREADS 512   /* threads per workgroup of k_tmpl_emit */
#endif
struct VgxTmplBuild // count pass: the first period's ordinary count + emit results -> template tables
{
	const vgx_draw* draws;       // the batch's first period
	const VgxMeshDesc* mdesc;
	const VgxMeshPrep* mprep;
	const vgx_mesh* mtab;
	const float2* poly;            // the period's LOCAL polyline (two-phase flatten with apply_transform = 0)
	const uint64_t* prefix_fill;   // [num_meshes + 1]
	const uint64_t* prefix_stroke; // [num_meshes + 1]
	uint64_t num_meshes, num_elems;
	uint32_t tile;               // slots per tile of the processing order = the most elements a tile holds (a multiple of 64)
	uint32_t* lmax;              // [nclasses] per class its longest mesh of at most vgx_tmpl_snap_limit(tile) elements (zeroed by the caller, k_tmpl_mesh_lmax): the tile stride (vgx_tmpl_plan.h)
	uint64_t* tbound;            // [tiles] greedily packed classes (bit 31 of lmax[class], k_tmpl_classes): the first element of every tile
	VgxTmplMesh* tmesh;
	vgx_mesh* tmtab;
	VgxTmplElem* telem;
	VgxTmplTile* ttile;          // [tiles]
	uint32_t period;
	uint32_t nclasses;           // the draws are `nclasses` representatives of `period` draws each
	uint64_t num_vertices, num_indices; // output totals of the concatenated representatives
	VgxTmplClass* cls;           // [nclasses + 1], written by the first build kernel
	VgxTmplRoundMesh* trmesh;    // [num_meshes + 1] (used: Round-join meshes + 1)
	uint2* tmsz;                 // [num_meshes] vertices, indices of the mesh (Round joins: 0x80000000 | number among the Round-join meshes, 0)
	uint32_t has_round;          // the template holds Round-join meshes (k_tmpl_styles): number them
	struct Sum3* partial;        // scratch of the device scan
};
struct VgxTmplArgs // one step
{
	const vgx_draw* draws;
	uint64_t ndraws;
	uint64_t ninst;
	uint32_t period;
	uint32_t npaths;
	const vgx_draw* tdraws;      // the first period as vgx_tessellate_count saw it
	const float2* tpoly;         // local polyline of one period
	const VgxTmplMesh* tmesh;
	const vgx_mesh* tmtab;       // mesh records of one instance (offsets relative to the instance)
	const VgxTmplElem* telem;
	const VgxTmplTile* ttile;
	uint32_t tile;               // elements per tile (= one workgroup of k_tmpl_emit)
	uint32_t tiles_per_inst;
	vgx_sizes inst;              // sizes of ONE instance
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	vgx_mesh* meshes_out;        // may be null
	const uint32_t* mesh_base;   // assembly armed: [ninst * meshes] vertices in front of each mesh inside its draw command; else null
	VgxCaps caps;                // vertices / indices / meshes of the caller's buffers
	VgxTotals* totals;
	// several classes (else null / 0): instance k = class iinfo[k].cls, workgroup b = tile wg[b].y (of the concatenated template) of instance wg[b].x
	const VgxTmplInst* iinfo;    // [ninst + 1]; the last entry = the batch totals
	const uint2* wg;             // [num_wg]
	uint64_t num_wg;
	vgx_sizes total;             // sizes of the whole batch
	VgxTmplKernel kernel;        // which emit kernel the template needs (vgx_tmpl_plan.h)
	// Round joins (templates of ONE class): the arc of every join is counted on the instance's TRANSFORMED polyline (stroker.cpp:1146, 1592), so the
	// sizes of those meshes -- and with them every output place behind them -- belong to the instance. Per-step tables, written by
	// vgx_launch_tmpl_round_sizes and read by k_tmpl_emit_round:
	uint32_t num_round;          // Round-join stroke meshes per instance (VgxTmplMesh::round_no = the mesh's number among them + 1)
	uint32_t num_round_elems;    // their elements per instance
	const VgxTmplRoundMesh* trmesh; // [num_round + 1]
	const uint2* tmsz;           // [meshes of the template] vertices, indices (Round joins: 0x80000000 | number among the Round-join meshes, 0): what the scan over the meshes reads
	unsigned long long* rsz;     // [ninst * num_round * 2] vertices, indices of every such mesh
	uint2* relem;                // [ninst * num_round_elems] per element of such a mesh: first vertex / index inside the mesh, size and inner side of the element in front (tmpl_round_word)
	VgxTmplMeshPlace* mplace;    // [ninst * meshes] per mesh of the batch: first vertex, first index in the BATCH (iplace set: inside its INSTANCE); vertices, indices
	unsigned long long* itot;    // [ninst * 2] (per-instance shape of the sizes pass only, else null) vertices, indices of the instance
	unsigned long long* iplace;  // [ninst * 2] ... first vertex, first index of the instance in the batch
	// Round joins, several classes (round 6; the per-instance shape of the sizes pass only): class c's Round-join meshes are trmesh[cls[c].round[VGX_TC_MESH0] ..
	// cls[c + 1].round[VGX_TC_MESH0]) (entry [nclasses]: all of them), an instance's tables lie at iinfo[k].m (mplace) and iinfo[k].rel (relem)
	const VgxTmplClass* cls;     // [nclasses + 1] (null: one class)
	uint32_t round_lds;          // Round-join meshes of the largest class (k_tmpl_round_sizes_inst's LDS table)
};
struct Sum3;
bool vgx_tmpl_round_per_instance(const VgxTmplArgs& a); // the sizes pass places the meshes per instance (many instances of a few hundred meshes): the caller sets a.itot / a.iplace
void vgx_launch_tmpl_round_sizes(const VgxTmplArgs& a, Sum3* partial, hipStream_t s); // Round-join templates, in front of vgx_launch_tmpl_emit: the tables above, totals->sizes, VGX_E_NOSPACE against a.caps
void vgx_launch_tmpl_mtab(const VgxTmplArgs& a, vgx_mesh* mtab, VgxMeshDesc* mdesc, hipStream_t s); // assembly armed: the whole batch's mesh table + mesh -> draw
void vgx_launch_tmpl_check(const vgx_draw* draws, uint64_t ndraws, uint32_t npaths, VgxTotals* totals, hipStream_t s); // after vgx_launch_inst_detect
void vgx_launch_tmpl_styles(const VgxTmplBuild& b, hipStream_t s);  // stroke styles of the template -> VGX_TMPL_STYLES(b.cls, nclasses) (zeroed by the caller), needs mdesc only
void vgx_launch_tmpl_classes(const VgxTmplBuild& b, hipStream_t s); // fills b.cls from the representatives' count + emit results
void vgx_launch_tmpl_class_sums(const VgxTmplBuild& b, const vgx_draw_info* dinfo, const uint64_t* cmdPrefix, uint64_t numDraws, const vgx_sizes& all, unsigned long long* sums, hipStream_t s); // after vgx_launch_tmpl_classes: [nclasses + 1][5] prefixes in front of every class
void vgx_launch_tmpl_build(const VgxTmplBuild& b, hipStream_t s);   // after vgx_launch_tmpl_classes
void vgx_launch_tmpl_hash(const vgx_draw* draws, uint64_t ndraws, uint64_t period, unsigned long long* hashes, hipStream_t s); // hashes[instance], zeroed by the caller
void vgx_launch_tmpl_check_cls(const vgx_draw* draws, uint64_t ndraws, uint64_t period, const uint32_t* inst_cls, const uint32_t* cls_rep, VgxTotals* totals, hipStream_t s);
void vgx_launch_tmpl_emit(const VgxTmplArgs& a, hipStream_t s);
#ifndef VGX_TMPL_RC_THREADS
#define VGX_TMPL_RC_THREADS 512 /* k_tmpl_emit_round_aa (templates of closed strokes with Round joins): threads per workgroup (its tile: VGX_TMPL_RC_TILE) */
#endif
#ifndef VGX_TMPL_RC_WAVES
#define VGX_TMPL_RC_WAVES 6     /* waves per SIMD its registers are limited for (80 VGPRs: three workgroups per CU) */
#endif

// merging two mesh sequences of a frame (vgx_merge.hip)
struct VgxMergeArgs
{
	vgx_cache_desc a, b;       // sequence A (vgx_tessellate's meshes) and B (external meshes); both sorted by draw
	const uint32_t* b_draw;    // frame draw of every B mesh (null: the records' own draw fields)
	uint32_t* order;           // [na + nb] merged position -> source mesh (bit 31: from B)
	vgx_mesh* mtab;            // [na + nb] merged mesh table (context scratch; assembly reads it)
	VgxMeshDesc* mdesc;        // [na + nb] only .draw is written (assembly's mesh -> draw)
	vgx_mesh* meshes_out;      // caller's table (may be null)
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	const uint32_t* mesh_base; // assembly armed: index base per merged mesh; else null
	const void* b_uv;          // per-vertex UVs of sequence B (may be null), uv_bytes each
	void* uv_out;              // the armed assembly's UV stream (null: none)
	uint32_t uv_bytes;
	VgxTotals* totals;
	VgxCaps caps;
};
void vgx_launch_merge_rank(const VgxMergeArgs& a, hipStream_t s);
void vgx_launch_merge_scan(const VgxMergeArgs& a, void* partial, hipStream_t s);
void vgx_launch_merge_copy(const VgxMergeArgs& a, hipStream_t s);

// concave-fill fringes (vgx_concave.hip)
struct VgxConcaveArgs
{
	const float* contour_verts;
	const vgx_contour* contours;
	uint64_t ncontours;
	uint64_t num_contour_vertices;
	const vgx_concave_fill* fills;
	uint64_t nfills;
	float* moved;              // vgx_concave_move only
	const float* tess_pos;     // vgx_concave_emit only (and everything below)
	const uint16_t* tess_idx;
	const vgx_mesh* mtab;      // [nfills] after the scan over the fills
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	VgxTotals* totals;
};
void vgx_launch_concave_move(const VgxConcaveArgs& a, hipStream_t s);
void vgx_launch_concave_emit(const VgxConcaveArgs& a, hipStream_t s);

// vgx_concave_contours: the flatten output and the draws, the three per-draw exclusive prefixes of the size scan ([ndraws + 1] each:
// contour vertices of the mesh-making draws, output vertices, output meshes), and the streams
struct VgxContoursArgs
{
	const float* poly;
	const vgx_subpath* subpaths;
	const vgx_draw_info* draw_info;
	const vgx_draw* draws;
	uint64_t ndraws;
	const uint64_t* contour_prefix;
	const uint64_t* vertex_prefix;
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	const VgxTotals* totals;
};
void vgx_launch_concave_contours(const VgxContoursArgs& a, hipStream_t s);

// vgx_concave_triangulate (vgx_triangulate.hip): the flatten output and the draws; per draw its route, its ring's vertex count and three
// exclusive prefixes ([ndraws + 1] each: ring vertices of the draws whose geometry decides = their place in `tri`, output vertices, output
// indices); the clipping's ring-local triangles; the streams with the caller's capacities
struct VgxTriArgs
{
	const float* poly;
	const vgx_subpath* subpaths;
	const vgx_draw_info* draw_info;
	const vgx_draw* draws;
	uint64_t ndraws;
	uint32_t* route;           // [ndraws] scratch
	uint32_t* draw_route;      // the caller's, may be null
	uint64_t* ring_vertices;   // [ndraws + 1]
	uint64_t* cand_prefix;     // [ndraws + 1]
	uint64_t* vertex_prefix;   // [ndraws + 1]
	uint64_t* index_prefix;    // [ndraws + 1]
	uint16_t* tri;             // [cap_tri]: draw d's triangles at 3 * cand_prefix[d]
	uint64_t cap_tri;
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	vgx_mesh* meshes;          // may be null
	uint64_t cap_vertices, cap_indices, cap_meshes;
	VgxTotals* totals;
};
void vgx_launch_concave_triangulate(const VgxTriArgs& a, void* partial /* Sum3[VGX_SCAN_BLOCKS] */, hipStream_t s);
// vgx_concave_triangulate_rings: the same arguments; cand_prefix counts SLOTS (V + 2 H per deciding draw) and `tri` holds three indices per slot
void vgx_launch_concave_triangulate_rings(const VgxTriArgs& a, void* partial /* Sum3[VGX_SCAN_BLOCKS] */, hipStream_t s);
// vgx_concave_triangulate_nested: as the rings entry's; groups: [ndraws] scratch, per triangulated draw its group count G (3 (V + 2 S - 4 G) indices)
void vgx_launch_concave_triangulate_nested(const VgxTriArgs& a, uint32_t* groups, void* partial /* Sum3[VGX_SCAN_BLOCKS] */, hipStream_t s);

// text runs (vgx_text.hip)
struct VgxTextArgs
{
	const float* quads;
	uint64_t nquads;
	const vgx_text_run* runs;
	uint64_t nruns;
	uint64_t first_mesh;
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	vgx_mesh* meshes;          // may be null
	void* uv;                  // may be null
	uint32_t uv_bytes;         // 4 or 8 when uv is set
	uint64_t cap_vertices, cap_indices, cap_meshes;
	uint32_t* tile_run;        // [tiles of quads] scratch: the first run of every tile; null = one launch, the tiles search
	VgxTotals* totals;
};
void vgx_launch_text_quads(const VgxTextArgs& a, hipStream_t s);

// dashed strokes (vgx_dash.hip)
#define VGX_DASH_RANGES 1024 /* workgroups of k_dash_count / k_dash_emit = threads of k_dash_ranges */
struct VgxDashPat;
struct VgxDashListRec        // per source list. 32 bytes
{
	uint64_t seg_base;       // its first segment in G (undashed lists and lists of < 2 vertices own none)
	uint64_t cand_off;       // its first "on" interval among the call's
	uint64_t jlo;            // number of that interval in the list's own pattern space (vgx_dash.h)
	uint64_t T;              // its length, fixed units
};
struct VgxDashArgs
{
	const float* poly;
	const vgx_subpath* subs;
	const uint32_t* sub_draw;
	uint64_t nsubs;
	const struct vgx_dash* dashes;
	uint64_t ndraws;
	const float* pattern;
	uint64_t npattern;
	VgxDashPat* pat;           // [ndraws]
	VgxDashListRec* lists;     // [nsubs + 1]
	uint64_t* G;               // [seg_cap + 1] exclusive sums of q(len) over the segments of the batch, modulo 2^64
	uint64_t* Ghi;             // [seg_cap + 1] ... of q(len) >> 31: decides whether a list's length fits
	uint64_t seg_cap;
	uint64_t* range_sum;       // [VGX_DASH_RANGES][2] pieces, vertices per range
	uint64_t* range_off;       // [VGX_DASH_RANGES][2] ... in front of it
	uint64_t* tot;             // [4] segments, "on" intervals, out-of-range flag (zeroed by the caller)
	float* out_poly;
	vgx_subpath* out_subs;
	uint32_t* out_draw;
	uint32_t* out_src;         // may be null
	uint64_t cap_poly, cap_subs;
	int check_caps;
	VgxTotals* totals;
	struct Sum3* partial;
	// vgx_tessellate_dashed (vgx_dashframe.hip): the lists are the flatten stage's own mesh descriptors, so their number is a device
	// word (nsubs is then the host's bound of it), and a list of an undashed draw produces nothing (its mesh descriptor is used as it is)
	const uint64_t* nsubs_dev; // null: nsubs
	int frame;
};
void vgx_launch_dash(const VgxDashArgs& a, bool emit, hipStream_t s);

// a frame with dashed strokes (vgx_dashframe.hip; the slots: vgx_dashframe.h)
struct VgxDashFrameArgs
{
	const vgx_draw* draws;
	const struct vgx_dash* dashes;  // [ndraws]
	const VgxMeshDesc* mdesc;       // the flatten stage's meshes, frame order (source)
	const vgx_mesh* mtab;
	const VgxMeshPrep* mprep;
	VgxMeshDesc* mdesc2;            // the frame's meshes: kept source meshes + one per piece
	vgx_mesh* mtab2;
	VgxMeshPrep* mprep2;
	vgx_subpath* lists;             // [cap_meshes + 1] per source mesh: the list the dash pass cuts (dashed stroke meshes; else empty)
	uint32_t* list_draw;            // [cap_meshes + 1]
	uint64_t* dashed_before;        // [cap_meshes + 1] D(m)
	uint64_t* nlists;               // device word: source meshes (0 when the flatten stage failed)
	const vgx_subpath* piece_subs;  // the dash pass's records: first_vertex relative to piece_base
	const uint32_t* piece_src;      // source mesh of every piece
	uint64_t piece_base;            // first piece vertex in the polyline scratch (behind the flatten stage's heap: one allocation holds both)
	uint64_t cap_meshes;            // what the mesh tables hold
	VgxTotals* totals;              // the call's
	VgxTotals* dash_totals;         // the dash pass's (pieces, their vertices, its verdict)
	uint64_t* need;                 // [4] device: pieces, piece vertices, source meshes, 1 -> the host's mirror
	vgx_sizes* dev_dash_sizes;      // caller's, may be null
	struct Sum3* partial;
};
void vgx_launch_dashframe_lists(const VgxDashFrameArgs& a, hipStream_t s);
void vgx_launch_dashframe_place(const VgxDashFrameArgs& a, hipStream_t s);
void vgx_launch_subpath_draws(const vgx_draw_info* dinfo, uint64_t ndraws, uint32_t* subDraw, uint64_t nsubs, hipStream_t s);

// launchers (defined in the .hip files)
void vgx_launch_flatten(bool emit, const VgxFlattenArgs& a, int numBlocks, hipStream_t s);
void vgx_launch_flatten_build(const VgxFlattenArgs& a, int waves, hipStream_t s, bool serialCount = true);   // single-pass: subdivide once, polyline -> heap
void vgx_launch_flatten_inst(const VgxFlattenArgs& a, int waves, hipStream_t s);  // instanced batches: one lane per instance (vgx_inst.hip)
void vgx_launch_inst_perm(const vgx_draw* draws, uint64_t ninst, uint32_t period, uint32_t nc, uint32_t* classHist /* [nc + 1] */, uint32_t* perm /* [ninst] */, VgxTotals* totals, bool multi /* testing: the several-kernel form for any count */, hipStream_t s);
void vgx_launch_inst_detect(const vgx_draw* draws, uint64_t ndraws, VgxTotals* totals, hipStream_t s); // count pass: period of the path sequence
// grouped mode: histogram of the draws' paths -> per-path ranges and task list (taskPath may be null: counts only) -> draw order
// nc: tolerance classes per path (1 = sort by path only); hist / cursor / keyStart hold npaths * nc + 1 entries (keyStart unused when nc == 1)
void vgx_launch_inst_group(const vgx_draw* draws, uint64_t ndraws, uint32_t npaths, uint32_t nc, uint32_t* hist, uint32_t* cursor, uint64_t* keyStart, uint64_t* start,
	uint64_t* taskStart, uint32_t* taskPath, uint64_t capTasks, uint32_t* order, VgxTotals* totals, void* scanPartial /* Sum3[VGX_SCAN_BLOCKS] */, hipStream_t s);
// frame-sized batches (vgx_flatten.hip): one-workgroup kernels instead of chains of dependent launches; the operators are
// the OpCmdPrefix / OpDrawInfo / OpMeshAll of vgx_scan_ops.h, passed type-erased (the header is device code)
#define VGX_SMALL_DRAWS 2048
struct VgxStrokeArgs;
void vgx_launch_small_front(const void* opCmdPrefix, vgx_draw_info* dinfo, hipStream_t s);
void vgx_launch_small_middle(const VgxFlattenArgs& f, const VgxStrokeArgs& st, const void* opDraws, const void* opMeshes, vgx_sizes* devSizes, uint32_t* devStatus, hipStream_t s);
void vgx_launch_flatten_gather(const VgxFlattenArgs& a, hipStream_t s);  // after the draw scan: ordered mesh descriptors
// vgx_tessellate_immediate (vgx_flatten.hip): the sizing pass behind the flatten stage (exits at once unless the batch outgrew the
// context's scratch; with `publish` it ends the call: the verdict as vgx_launch_imm_publish) and the verdict (VGX_E_GROWN / what the
// pipeline left) into dev_sizes / dev_status and the totals
void vgx_launch_imm_size(const VgxPathSetDev& ps, const vgx_draw* draws, uint64_t ndraws, VgxTotals* totals, int fromStatus, bool publish, vgx_sizes* devSizes, uint32_t* devStatus, hipStream_t s);
void vgx_launch_imm_publish(VgxTotals* totals, vgx_sizes* devSizes, uint32_t* devStatus, hipStream_t s);
void vgx_launch_flatten_gather_ordered(const VgxFlattenArgs& a, hipStream_t s); // vgx_tessellate's one-walk route: mesh descriptors from k_flat1's ordered records
#ifndef VGX_BUILD_WAVES
#define VGX_BUILD_WAVES 4096
#endif
#define VGX_BUILD_BLOCK 8192 /* polyline vertices per wave-private heap block */
#define VGX_BUILD_OVERFLOW 120 /* leaves per lane beyond the LDS slots kept in the wave's global overflow area */
void vgx_launch_stroke(bool emit, const VgxStrokeArgs& a, int numBlocks, hipStream_t s);
void vgx_launch_mesh_prepare(const VgxStrokeArgs& a, hipStream_t s);

// draw-command assembly (vgx_assemble.hip)
struct VgxAsmArgs
{
	const vgx_mesh* mtab;      // after the scan over meshes (first_vertex / first_index filled)
	uint32_t* jump0;           // [meshes + 1] next / doubled jump table (ping)
	uint32_t* jump1;           // [meshes + 1] (pong)
	uint32_t* start;           // [cap_start] first mesh of every vertex buffer; cap_start is a power of two
	uint64_t cap_start;
	uint32_t* mesh_base;       // [meshes] out: vertices in front of the mesh inside its vertex buffer
	vgx_drawcmd* drawcmds;     // caller's table
	uint64_t cap_drawcmds;
	uint64_t* dev_num_drawcmds;
	uint32_t max_vb;
	VgxTotals* totals;
	// VGX_ASM_SPLIT_STATE: a change of the draws' state_key between consecutive meshes also starts a draw command
	uint32_t flags;
	const VgxMeshDesc* mdesc;  // mesh -> draw
	const vgx_draw* draws;     // draw -> state_key (null: no draws at this level, e.g. the shape cache)
	uint32_t* mesh_cmd;        // [meshes] scratch: draw command of every mesh (aliases jump0 once the doubling is done)
	void* partial;             // scan partials (Sum3[VGX_SCAN_BLOCKS])
	uint64_t max_meshes;       // capacity of the per-mesh scratch
	uint64_t scan_bound;       // host-known bound of the mesh count (launch shape of the scan over the meshes): the caller's mesh capacity when it gave a table
	// white-pixel UV stream (vg.cpp:5218-5225)
	void* uv; uint32_t uv_bytes; uint32_t uv_value[2];
};
void vgx_launch_assemble(const VgxAsmArgs& a, hipStream_t s);

// shape-cache instancing (vgx_cache.hip)
struct VgxCacheArgs
{
	vgx_cache_desc cache;
	const vgx_cache_instance* inst;
	uint64_t ninst;
	const uint64_t* inst_mesh_prefix; // [ninst + 1] exclusive scans over the instances
	const uint64_t* inst_vert_prefix;
	const uint64_t* inst_idx_prefix;
	vgx_mesh* mtab;                   // output mesh table (context scratch; the assembly step reads it)
	vgx_mesh* meshes_out;             // caller's copy (may be null)
	float* pos;
	uint32_t* color;
	uint16_t* idx;
	const uint32_t* mesh_base;        // assembly armed: index base per output mesh; else null
	VgxTotals* totals;
};
void vgx_launch_cache_localize(const vgx_draw* draws, uint64_t ndraws, float* pos, const vgx_mesh* meshes, uint64_t numMeshes, hipStream_t s);
void vgx_launch_cache_meshes(const VgxCacheArgs& a, hipStream_t s);
void vgx_launch_cache_copy(const VgxCacheArgs& a, int numBlocks, hipStream_t s);
void vgx_launch_fill(const VgxStrokeArgs& a, int numBlocks, hipStream_t s);

// mesh bounds and view culling of cached instances (vgx_bounds.hip)
struct VgxCullArgs
{
	uint64_t cache_meshes;            // meshes of the cache = entries of mesh_bounds
	const float* mesh_bounds;         // [cache_meshes][4], 16-byte aligned
	const vgx_cache_instance* inst;
	uint64_t ninst;
	const float* views;               // [nviews][4]
	uint32_t nviews;
	const uint32_t* inst_view;        // [ninst] or null: view 0
	vgx_cache_instance* out_inst;     // [ninst]; may be `inst`
	float* out_bounds;                // [ninst][4] or null
	uint8_t* flags;                   // [ninst] 1 = kept (context scratch), null when no compaction follows
	uint32_t* status;                 // the caller's dev_status (already VGX_OK) or null
};
void vgx_launch_mesh_bounds(const float* pos, const vgx_mesh* meshes, uint64_t numMeshes, float* bounds, hipStream_t s);
void vgx_launch_cache_cull(const VgxCullArgs& a, uint32_t* kept, uint64_t* numKept, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, hipStream_t s);

// hit testing (vgx_pick.hip)
struct VgxPickArgs
{
	const float* pos; const uint32_t* color; const uint16_t* idx; const vgx_mesh* meshes; // the frame
	uint64_t num_meshes;              // < 2^32 - 1
	const float* mesh_bounds;         // [num_meshes][4], 16-byte aligned: the caller's, or the context's own
	const vgx_pick_query* queries;
	uint32_t nqueries;                // <= VGX_PICK_MAX_QUERIES
	vgx_pick_hit* hits;
	uint64_t* keys;                   // [VGX_PICK_MAX_QUERIES] (context scratch, as everything below)
	uint32_t* cand_tris;              // [num_meshes] triangle count of a candidate, 0 for any other mesh
	uint32_t* cand_mesh;              // [num_meshes] the candidates, dense and ascending
	uint64_t* cand_prefix;            // [num_meshes + 1] exclusive prefix of the candidates' triangle counts, the total behind it
	uint64_t* totals;                 // candidates, candidate triangles
};
void vgx_launch_pick(const VgxPickArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, uint32_t grid, hipStream_t s);

// region queries (vgx_pick_rect.hip): vgx_pick_rect. One 64-bit word per mesh and plane, one bit per query; a block is 64 consecutive
// meshes (one wave of the selection and list kernels). Every table is sized by num_meshes
struct VgxPickrArgs
{
	const float* pos; const uint32_t* color; const uint16_t* idx; const vgx_mesh* meshes; // the frame
	uint64_t num_meshes;              // < 2^32 - 1
	const float* mesh_bounds;         // [num_meshes][4], 16-byte aligned: the caller's, or the context's own
	const vgx_pick_rect_query* queries;
	uint32_t nqueries;                // 1 .. VGX_PICK_RECT_MAX_QUERIES
	uint32_t list_cap;
	vgx_pick_hit* top; uint32_t* list; uint32_t* count; // the caller's, each may be null
	uint64_t* cand;                   // [num_meshes] (context scratch, as everything below) the queries the mesh is a candidate of; from k_pickr_select on: the queries that list an entry at the mesh
	uint64_t* inside;                 // [num_meshes] inside(m), 1 for a query whose range the mesh is not in; written only when a query has VGX_PICK_RECT_WINDOW
	uint64_t* touch;                  // [num_meshes] touch(m)
	uint32_t* cand_tris;              // [num_meshes] triangle count of a candidate, 0 for any other mesh; bit 31: the mesh begins a run
	uint32_t* cand_mesh;              // [num_meshes] the candidates, dense and ascending
	uint64_t* cand_prefix;            // [num_meshes + 1] exclusive prefix of the candidates' triangle counts, the total behind it
	uint32_t* run_of;                 // [num_meshes] the run of every mesh, runs numbered densely
	uint32_t* run_first;              // [num_meshes] the first mesh of every run
	uint64_t* run_touch;              // [num_meshes] per run the OR of touch ...
	uint64_t* run_inside;             // [num_meshes] ... and the AND of inside over its meshes; both only when a query has VGX_PICK_RECT_BY_DRAW
	uint32_t* block_count;            // [blocks][64] entries of (block, query); from k_pickr_finish on: the entries of the query in the blocks before
	uint32_t* block_top;              // [blocks][64] the block's largest mesh + 1 with a bit in its `touch` word for the query, 0: none
	uint64_t* totals;                 // candidates, candidate triangles, runs
};
void vgx_launch_pick_rect(const VgxPickrArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, uint32_t grid, hipStream_t s);

// ... under scissors, clip regions and contour fills (vgx_pick_frame). A candidate is a mesh of the range that some query's point can
// lie in (box and draw scissor); candidates are numbered densely in ascending mesh order, and every table below is sized by the range
struct VgxPickfMesh;
struct VgxPickfArgs
{
	const float* pos; const uint32_t* color; const uint16_t* idx; const vgx_mesh* meshes; // the frame
	const float* mesh_bounds;         // [num_meshes][4], 16-byte aligned: the caller's, or the context's own
	uint64_t mesh_begin, nrange;      // the meshes looked at: [mesh_begin, mesh_begin + nrange), the end < 2^32 - 1
	const vgx_draw* draws; const vgx_draw_state* draw_state; // [num_draws], checked by the host
	uint32_t num_draws;
	uint32_t nqueries;                // <= VGX_PICK_MAX_QUERIES
	const vgx_pick_query* queries;
	vgx_pick_hit* hits;
	uint32_t* status;                 // the caller's dev_status or null
	VgxPickfMesh* mesh_state;         // [nrange] (context scratch, as everything below): vgx_pick.h's record, VGX_PICKF_* flags beside the mode
	uint32_t* cand_mesh;              // [nrange] the candidates (mesh - mesh_begin), dense and ascending
	uint32_t* tri_cand;               // [nrange] the triangle candidates as candidate numbers, dense and ascending
	uint64_t* tri_prefix;             // [nrange + 1] exclusive prefix of their triangle counts, the total behind it
	uint32_t* con_cand;               // [nrange] the contour candidates as candidate numbers
	uint32_t* cover;                  // [nrange][8] per candidate one bit per query: covered at the point under the query's flags; zeroed by the scan
	uint64_t* totals;                 // candidates, candidate triangles, contour candidates, meshes with draw >= num_draws
};
void vgx_launch_pick_frame(const VgxPickfArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, uint32_t grid, hipStream_t s);

// ... of a draw-command table (vgx_pick_cmds.hip): vgx_pick_commands. Nothing is kept per chunk or per triangle: overlapping index
// ranges leave the chunk total unbounded by the index stream, so every table is sized by num_cmds and nqueries
struct VgxPickcArgs
{
	const float* pos; const uint32_t* color; const uint16_t* idx; // the streams, checked by the host
	uint64_t num_vertices, num_indices;
	const vgx_raster_cmd* cmds;       // [num_cmds]
	const uint32_t* dev_num_cmds;     // or null: the table is cmds[0 .. min(num_cmds, *dev_num_cmds))
	const vgx_mesh* meshes;           // [num_meshes] the owners, or null
	uint64_t num_meshes;
	uint32_t num_cmds;
	uint32_t nqueries;                // <= VGX_PICK_MAX_QUERIES
	const vgx_pick_cmd_query* queries;
	vgx_pick_cmd_hit* hits;
	uint32_t* status;                 // the caller's dev_status or null
	VgxPickfMesh* cmd_state;          // [num_cmds] (context scratch, as everything below): vgx_pick_cmds.h's record, VGX_PICKC_CAND beside the mode
	uint64_t* cmd_first;              // [num_cmds + 1] first chunk of every command, the total behind the real count
	uint32_t* top;                    // [nqueries][num_cmds] the largest counting triangle + 1 of (query, command), 0: none; zeroed by k_pickc_cmds
	uint64_t* state;                  // VGX_PICKC_*
	const float* cmd_bounds;          // vgx_pick_commands_boxed: [num_cmds][4], 16-byte aligned, or null. Read by the BOXED instantiations alone
};
enum { VGX_PICKC_CHUNKS = 0, VGX_PICKC_INVALID = 1, VGX_PICKC_CMDS = 2 /* the real command count */, VGX_PICKC_WORDS = 4 };
void vgx_launch_pick_commands(const VgxPickcArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, uint32_t grid, hipStream_t s);

// per-command boxes of a draw-command table (vgx_cmd_bounds.hip): vgx_command_bounds. The commands looked at are those of the range,
// [cmd_begin, min(cmd_end, real count)); command i of the range is cmds[cmd_begin + i]
struct VgxCmdBoundsArgs
{
	const float* pos; const uint16_t* idx; // the streams, checked by the host
	uint64_t num_vertices, num_indices;
	const vgx_raster_cmd* cmds;       // [num_cmds]
	const uint32_t* dev_num_cmds;     // or null: the table is cmds[0 .. min(num_cmds, *dev_num_cmds))
	uint32_t num_cmds, cmd_begin, cmd_end;
	uint32_t* bounds;                 // the caller's [num_cmds][4], 16-byte aligned: order-preserving images until k_cmdb_decode
	uint32_t* status;                 // the caller's dev_status or null
	uint64_t* cmd_first;              // [range + 1] (context scratch, as `state`): first chunk of every command of the range, the total behind them
	uint64_t* state;                  // VGX_CMDB_*
};
enum { VGX_CMDB_CHUNKS = 0, VGX_CMDB_CMDS = 1 /* the commands of the range */, VGX_CMDB_WORDS = 2 };
void vgx_launch_command_bounds(const VgxCmdBoundsArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, uint32_t grid, hipStream_t s);

// incremental update of a submitted frame (vgx_update.hip)
struct VgxUpdateArgs
{
	vgx_cache_desc cache;
	const vgx_cache_instance* inst;   // the edited array
	uint64_t ninst;
	const vgx_cache_slot* slots;      // [ninst + 1]
	const uint32_t* dirty;            // [ndirty]
	uint64_t ndirty;
	const uint64_t* dev_ndirty;       // or null: the list is dirty[0 .. min(ndirty, *dev_ndirty))
	float* pos; uint32_t* color;      // the frame
	uint64_t frame_vertices, frame_meshes;
	float* mesh_bounds;               // [frame_meshes][4] or null
	uint64_t* vert_prefix;            // [ndirty + 1] exclusive scans over the listed entries (context scratch, as the next two)
	uint64_t* mesh_prefix;            // [ndirty + 1]
	uint32_t* flags;                  // one word, zeroed: VGX_UPD_* of every listed entry, ORed
	uint32_t* status;                 // the caller's dev_status or null
};
void vgx_launch_cache_layout(const vgx_cache_desc& cache, const vgx_cache_instance* inst, uint64_t ninst, vgx_cache_slot* slots, uint32_t* status,
                             void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, hipStream_t s);
void vgx_launch_cache_update(const VgxUpdateArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, hipStream_t s);

// rendering to an image (vgx_raster.hip)
struct VgxRasterArgs
{
	const float* pos; const uint32_t* color; const uint16_t* idx; const vgx_mesh* meshes; // the frame
	const float* mesh_bounds;         // [num_meshes][4], 16-byte aligned: the caller's, or the context's own
	uint64_t mesh_begin, nrange;      // the meshes drawn: [mesh_begin, mesh_begin + nrange), the end < 2^32 - 1
	uint32_t* pixels;                 // the target, checked by the host
	uint32_t stride;
	int32_t x0, y0;
	uint32_t scissor[4];              // inside the image, not inverted
	uint32_t flags, clear_color;
	uint32_t tiles_w;                 // tiles per row of the IMAGE: tile number = ty * tiles_w + tx
	uint32_t tile_x0, tile_y0, tiles_x, tiles_y; // the tiles the scissor touches = the grid of k_raster_tiles (0 x 0: nothing to write)
	uint32_t sentinel, sort_bits;     // tiles of the image = the key behind every tile; its bits
	uint64_t entry_cap;               // entries keys / vals hold (each of the four arrays)
	uint64_t sort_n;                  // <= entry_cap: what the sort looks at (the host's bound of the entry count)
	uint32_t* mesh_entries;           // [nrange] (context scratch, as everything below)
	uint64_t* mesh_first;             // [nrange]
	uint32_t* keys; uint32_t* vals;   // [entry_cap] in mesh order
	uint32_t* sorted_keys; uint32_t* sorted_vals; // [entry_cap] in tile order
	unsigned long long* state;        // [0] the call's status, [1] its entries: what the pinned mirror carries to the next call
	uint32_t* status;                 // the caller's dev_status or null
};
size_t vgx_raster_sort_bytes(uint64_t n, uint32_t bits); // temporary storage the sort of n entries wants; 0: the query failed
hipError_t vgx_launch_raster(const VgxRasterArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, void* sortTemp, size_t sortBytes, hipStream_t s);

// ... of the frame-level calls (vgx_raster_frame, vgx_raster_textured, vgx_raster_painted): the same arguments and tables, the level
// (VGX_RL_*, vgx_raster.h), the draw state, per mesh of the range what k_rasterf_count made of it, and what the wider levels read
struct VgxRasterMeshState;
struct VgxRasterFrameArgs
{
	VgxRasterArgs R;
	int32_t level;                    // VGX_RL_FRAME .. VGX_RL_CONCAVE
	uint32_t num_draws;
	const vgx_draw* draws; const vgx_draw_state* draw_state; // [num_draws], checked by the host
	VgxRasterMeshState* mesh_state;   // [nrange] (context scratch)
	// from VGX_RL_TEXTURED on, else zero
	const void* uv;                   // [num_vertices][uv_bytes], checked by the host; read for the vertices of sampled meshes only
	const vgx_raster_image* images;   // [num_images]; a record is read (and checked, by k_rasterf_count) only when a mesh names it
	uint32_t uv_bytes, num_images;
	uint32_t* tile_tex;               // [(sentinel + 31) / 32] one bit per tile of the image, zero at the launch: a sampled mesh has an entry there (context scratch)
	// at VGX_RL_PAINTED, else zero
	const vgx_paint* gradients;       // [num_gradients]; an entry is read (and checked, by k_rasterf_count) only when a painted mesh names it
	const vgx_paint* patterns;        // [num_patterns]
	uint32_t num_gradients, num_patterns;
	uint32_t* tile_paint;             // [(sentinel + 31) / 32] as tile_tex: a painted mesh has an entry there (context scratch)
	// at VGX_RL_CONCAVE, else zero
	uint32_t* tile_contour;           // [(sentinel + 31) / 32] as tile_tex: a contour mesh has an entry there (context scratch)
	// vgx_raster_damaged (at VGX_RL_CONCAVE), else null: the kernels without the DAMAGE parameter run and never look at it
	const uint32_t* damage;           // [(sentinel + 31) / 32] the caller's: one bit per tile of the image, "redraw it"
};
hipError_t vgx_launch_raster_frame(const VgxRasterFrameArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, void* sortTemp, size_t sortBytes, hipStream_t s);

// a draw-command table to an image (vgx_raster_cmds.hip): vgx_raster_commands bins chunks of 64 consecutive triangles, not meshes
struct VgxRasterRect;
struct VgxRasterCmdArgs
{
	const float* pos; const uint32_t* color; const void* uv; const uint16_t* idx; // the streams, checked by the host
	uint64_t num_vertices, num_indices;
	const vgx_raster_cmd* cmds;       // [num_cmds]
	const uint32_t* dev_num_cmds;     // or null: the table is cmds[0 .. min(num_cmds, *dev_num_cmds))
	uint32_t num_cmds, uv_bytes;
	const vgx_raster_image* images;   // [num_images]; a record is read (and checked, by k_rasterc_cmds) only when a command names it
	const vgx_paint* gradients;       // [num_gradients], as images; null / 0 when the caller gave no paints
	const vgx_paint* patterns;        // [num_patterns]
	uint32_t num_images, num_gradients, num_patterns;
	uint32_t* pixels;                 // the target, checked by the host: the fields of VgxRasterArgs
	uint32_t stride;
	int32_t x0, y0;
	uint32_t scissor[4];
	uint32_t flags, clear_color;
	uint32_t tiles_w, tile_x0, tile_y0, tiles_x, tiles_y, sentinel, sort_bits;
	uint64_t chunk_cap;               // chunks chunk_rect / chunk_cmd / chunk_first hold
	uint64_t entry_cap;               // entries keys / vals hold (each of the four arrays)
	uint64_t sort_n;                  // <= entry_cap: what the sort looks at
	VgxRasterMeshState* cmd_state;    // [num_cmds] what every command does (context scratch, as everything below)
	uint64_t* cmd_first;              // [num_cmds + 1] first chunk of every command, the total behind the real count
	VgxRasterRect* chunk_rect;        // [chunk_cap] the tiles a chunk's triangles reach (empty: tx0 > tx1)
	uint32_t* chunk_cmd;              // [chunk_cap]
	uint64_t* chunk_first;            // [chunk_cap] first entry of every chunk
	uint32_t* keys; uint32_t* vals;   // [entry_cap] in chunk order: tile, global chunk ordinal
	uint32_t* sorted_keys; uint32_t* sorted_vals; // [entry_cap] in tile order
	uint32_t* tile_paint;             // [(sentinel + 31) / 32] one bit per tile of the image, zero at the launch: a painted command has an entry there
	unsigned long long* state;        // VGX_RASC_*: what the pinned mirror carries to the next call
	uint32_t* status;                 // the caller's dev_status or null
	const uint32_t* damage;           // vgx_raster_commands_damaged: the tile bits (vgx_damage.h); else null. Read by the DAMAGE instantiations alone
	const float* cmd_bounds;          // ... its [num_cmds][4] boxes, 16-byte aligned, or null: no command is skipped by its box
	uint32_t width, height;           // ... the image, for the tiles a box reaches
};
enum { VGX_RASC_STATUS = 0, VGX_RASC_ENTRIES = 1, VGX_RASC_CHUNKS = 2, VGX_RASC_INVALID = 3, VGX_RASC_BEYOND = 4 /* entries of the chunks behind chunk_cap */,
       VGX_RASC_CMDS = 5 /* the real command count */, VGX_RASC_WORDS = 6 };
hipError_t vgx_launch_raster_commands(const VgxRasterCmdArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, void* sortTemp, size_t sortBytes, hipStream_t s);

// vgx_raster_cmds_from_assembly (vgx_raster_cmds.hip)
struct VgxCmdsFromAsmArgs
{
	const vgx_drawcmd* drawcmds; uint64_t cap_drawcmds; const uint64_t* dev_num_drawcmds; // the table is [0, min(cap, *dev_num)) (dev_num null: cap)
	const vgx_mesh* meshes; uint64_t num_meshes;
	const vgx_draw_state* draw_state; uint32_t num_draws;
	vgx_raster_cmd* out;              // [cap_drawcmds]
	uint32_t* dev_num_cmds;
	uint32_t* flag;                   // one word, zeroed: != 0 once something was invalid (context scratch)
	uint32_t* status;                 // the caller's dev_status or null
};
void vgx_launch_cmds_from_assembly(const VgxCmdsFromAsmArgs& a, hipStream_t s);

// damage marks (vgx_damage.hip): the boxes of a mesh range, or of the frame meshes of the listed instances, ORed into a tile bitmap
struct VgxDamageArgs
{
	const float* mesh_bounds;         // [num_meshes][4], 16-byte aligned
	uint64_t num_meshes;
	uint64_t mesh_begin, nrange;      // vgx_damage_meshes: [mesh_begin, mesh_begin + nrange), inside the table
	const vgx_cache_slot* slots;      // vgx_damage_instances: [ninst + 1]
	uint64_t ninst;
	const uint32_t* dirty;            // [ndirty]
	uint64_t ndirty;
	const uint64_t* dev_ndirty;       // or null: the list is dirty[0 .. min(ndirty, *dev_ndirty))
	int32_t x0, y0;                   // the target
	uint32_t width, height, tiles_w;
	uint32_t* tile_bits;              // the caller's bitmap
	uint64_t* mesh_prefix;            // [ndirty + 1] exclusive scan of the listed entries' mesh counts (context scratch, as the next)
	uint32_t* flags;                  // one word, zeroed: != 0 once an entry was invalid
	uint32_t* status;                 // the caller's dev_status or null
};
void vgx_launch_damage_meshes(const VgxDamageArgs& a, hipStream_t s);
void vgx_launch_damage_instances(const VgxDamageArgs& a, void* partial /* [VGX_SCAN_BLOCKS] Sum3 */, hipStream_t s);

#endif
