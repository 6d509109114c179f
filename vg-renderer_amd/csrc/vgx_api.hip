// vgx_api.hip -- implementation of the C-ABI declared in include/vgx.h.
//
// The host side of every entry point: the context (grow-only device scratch, options, what the last count chose), the scan operators
// and three small kernels of no stage, and per entry the argument checks, the scratch sizing and the launch sequence over the kernels
// of the other .hip files. Lengths that are results of earlier kernels stay in device memory (VgxTotals); the asynchronous entries never
// synchronise with the host. In order: pipeline pieces (run*), context and path set, flatten, partition, template mode, tessellate with
// immediate mode (rules: vgx_route_plan.h), stroker level, dashes, shape cache, culling, picking, raster, damage, updates, concave fills, text, gather.
#include "vgx_internal.h"
#include "vgx_scan.h"
#include "vgx_scan_ops.h"
#include "vgx_pathsim.h"
#include "vgx_inst.h"
#include "vgx_flat1.h"
#include "vgx_thin.h"
#include "vgx_pathset_dev.h"
#include "vgx_tile.h"
#include "vgx_mscan.h"
#include "vgx_dash.h"
#include "vgx_update.h"
#include "vgx_raster.h"
#include "vgx_raster_cmds.h"
#include "vgx_damage.h"
#include "vgx_pick.h"
#include "vgx_pick_cmds.h"
#include "vgx_pick_rect.h"
#include "vgx_cmd_bounds.h"
#include "vgx_concave_lane.h"
#include "vgx_scratch.h"
#include "vgx_route_plan.h"
#include <vector>
#include <algorithm>
#include <atomic>
#include <string.h>
#include <math.h>
#include <new>
#include <stdlib.h>

#define VGX_GRID_BLOCKS 32768 // one-wave workgroups, each owning a contiguous run of segments (>> resident waves: no tail)

// Grid of the element kernels for a batch whose element count is at most `maxElements` (a bound the host knows: the
// caller's vertex capacity -- every element emits at least one vertex). Frame-sized batches should not pay for
// dispatching 32768 workgroups that exit at once (~8 us per kernel).
static int vgxElementGrid(uint64_t maxElements)
{
	const uint64_t want = maxElements / (2 * 64) + 1; // >= 2 chunks per wave
	const uint64_t full = (uint64_t)VGX_GRID_BLOCKS;
	return (int)(want < 256 ? 256 : (want > full ? full : want));
}

struct vgx_pathset
{
	VgxPathSetDev dev;
	void* blob; // single device allocation holding every array
	size_t blobBytes;
	uint32_t maxCmdsPerPath;
	bool hasSerial; // some path takes the exact serial builder (ARC / ARC_TO / closed shapes)
	bool hasEmpty;  // some path has no commands
	uint32_t numSubs; // sub-paths of the set (entries of sub_last_cmd / thin_sub)
	bool thinStatic; // every path is MOVE_TO / LINE_TO / CLOSE only and the static layout tables are filled (vgx_thin.h): k_flatten_thin builds its batches
	uint64_t gen; // unique per vgx_pathset_create (process-wide counter): identifies the path set where an address could be reused
};

#define VGX_PS_POOL 8
#define VGX_PS_POOL_MAX ((size_t)8 << 20)

// A small pinned host block that follows a device value without the host ever waiting for it: a call pushes a copy and an event
// behind its work, a later call reads the block only once the event says the copy has landed (else it goes without)
template<class T> struct HostMirror
{
	T* host; // [n]
	uint32_t n;
	hipEvent_t ev;
	bool pending;
	int create(vgx_ctx* ctx, uint32_t count); // at first use (zeroed); no-op afterwards
	void push(vgx_ctx* ctx, const void* dev, hipStream_t s); // copy of the n device elements + event record
	bool landed(); // true once per push, when its copy has arrived
	void release();
};

struct VgxGatherWire { vgx_rank_sizes z; uint64_t chunk; }; // vgx_gather_sizes: what every rank tells the others

// The template the last vgx_tessellate_count built (tryTemplate). The scalar part is filled in a local value and committed to the
// context in ONE assignment; the buffers stay where they are (a Buf is on the context's list by address).
struct VgxTemplateState
{
	bool on;                 // a step may use it (tmplFor). Everything below is only read with `on` set, or by the build itself
	bool isBatch;            // batch-wide: the whole draw list = one instance (vgx_set_static_batches)
	const vgx_pathset* ps;
	uint64_t psGen;          // generation id of ps when the template was built (an address can be reused by a later path set)
	uint32_t period;
	uint32_t classes;        // 1: every instance repeats the first period
	VgxTmplKernel kernel;    // which emit kernel it needs (vgx_tmpl_plan.h)
	uint32_t tileSize;       // slots per tile of the element table = the most elements a tile holds
	uint32_t tilesPerInst;   // one class: tiles of one instance (k_tmpl_classes' count: boundaries avoid the short meshes, vgx_tmpl_plan.h)
	vgx_sizes inst;          // sizes of one instance (of the first class)
	vgx_sizes total;         // sizes of the whole batch
	uint64_t numWg, nDraws;  // several classes: workgroups of one step; the batch size the per-instance table was built for
	uint32_t round;          // Round-join stroke meshes per instance: their sizes, and every place behind them, are counted per step
	uint32_t roundElems;     // their elements per instance
	uint32_t roundLds;       // Round-join meshes of the largest class (several classes; else = round)
	uint64_t relemWords;     // several classes: table words of the whole batch (sum over the instances of their class's Round-join elements)
};
struct VgxTemplate : VgxTemplateState
{
	Buf<VgxTmplTile> tile;   // [tiles]
	Buf<float2> poly; Buf<VgxTmplMesh> mesh; Buf<vgx_mesh> mtab; Buf<VgxTmplElem> elem; Buf<vgx_draw> draws;
	// several classes: one template over the concatenated class representatives, a per-instance table of output places, a
	// per-workgroup table (instance, tile)
	Buf<unsigned long long> hash, clsSum; Buf<uint32_t> instCls, clsRep; Buf<VgxTmplClass> cls; Buf<uint32_t> clsLmax; Buf<uint64_t> tbound; Buf<VgxTmplInst> iinfo; Buf<uint2> wg;
	Buf<VgxTmplRoundMesh> trmesh; Buf<uint2> tmsz; // the Round-join meshes (mesh, first element among the Round-join elements); per mesh its sizes (VgxTmplArgs::tmsz)
	Buf<unsigned long long> rsz, itot, iplace; Buf<uint2> relem; Buf<VgxTmplMeshPlace> mplace; // the per-step tables of a Round-join template (VgxTmplArgs)
};
static_assert(sizeof(VgxTmplWg) == sizeof(uint2) && offsetof(VgxTmplWg, inst) == offsetof(uint2, x) && offsetof(VgxTmplWg, tile) == offsetof(uint2, y), "the host's workgroup table is uploaded as uint2");
static_assert(sizeof(VgxTmplClass) == 40 && offsetof(VgxTmplClass, round) == 32 && sizeof(VgxTmplClass().round) == 8, "VgxTmplClass: the named words lie where the padding did");
static_assert(sizeof(VgxTmplMesh) == 64 && offsetof(VgxTmplMesh, fringe_bits) == 56 && offsetof(VgxTmplMesh, round_no) == 60, "VgxTmplMesh: the named words lie where the padding did");

// The ordinary pipeline's state between calls. `chosen`: what the last count (or the immediate call under way) chose; the rest: what the tables hold
struct VgxRouteState
{
	VgxRoute chosen;
	const vgx_pathset* f1Ps; uint64_t f1PsGen;               // one-walk: the path set the look-back tables were sized for
	uint64_t instPaths, instKeys, instTasks, instDraws;      // grouped mode: what the sort buffers hold (ensureInstGroup)
	uint64_t capDraws;                                       // draws the per-draw buffers hold (ensureDrawBuffers)
	bool tileHint;                                           // the last ordinary vgx_tessellate_count saw fills and closed Miter AA / Thin strokes only (the tile kernel's batches)
};
// state of the last *_count call (what _emit continues from)
enum VgxCountedStage { VGX_COUNTED_NONE = 0, VGX_COUNTED_FLATTEN, VGX_COUNTED_TESSELLATE, VGX_COUNTED_STROKE };
struct VgxCounted { const vgx_pathset* ps; const vgx_draw* draws; uint64_t ndraws /* (the stroker-level count: vertex lists) */; VgxCountedStage stage; };
// vgx_tessellate_immediate: pinned mirror of the last call's totals (read only once its copy has landed), the batch it belongs to (tag, draw
// count, was the detection pass run), and what the host learned from the last mirror it read: the batch and, in `facts`, its sizes, period, paths
struct VgxImmState
{
	HostMirror<VgxTotals> mirror; uint64_t pendTag, pendNDraws; bool pendDetect, known; uint64_t tag; VgxRouteFacts facts;
};

struct vgx_ctx
{
	int device;
	int lastHipError;
	int pendingHipError; // first failure of an asynchronous helper call (memset) inside the current entry point
	// grow-only device scratch (vgx_scratch.h). A new buffer is declared Buf<T> and grown with ensure(ctx, buf, items): that is all --
	// it joins `scratch`, which vgx_destroy frees and vgx_scratch_bytes sums. A buffer seen under several types stays a DevBuf, its
	// views named at the declaration
	DevBufList scratch;
	Buf<uint32_t> asmJump0, asmJump1, asmStart, meshBase; // draw-command assembly scratch (only when armed)
	vgx_assembly asmCfg;
	bool asmArmed;
	Buf<uint64_t> subPrefix; // exclusive scan of the draws' static sub-path counts
	DevBuf cmdPrefix;                    // views: uint64_t[ndraws + 1] command prefix (vgx_partition: the weight prefix), 3 x uint64_t[ninst + 1] (vgx_cache_submit), uint32_t order (vgx_merge)
	DevBuf poly;                         // views: float[2 x vertices] / float2 polyline heap, behind it the pieces of vgx_tessellate_dashed
	DevBuf partial;                      // views: the slice sums of whichever scan runs (Sum3[VGX_SCAN_BLOCKS] sizes it)
	Buf<uint32_t> cmdCnt, serialList;
	Buf<VgxSubRec> subFirst;
	Buf<float> leafOverflow;
	Buf<vgx_draw_info> dinfo;
	Buf<vgx_subpath> subs;
	Buf<VgxMeshDesc> mdesc;
	Buf<uint64_t> elemPrefix, elemPrefixS;
	Buf<VgxMeshPrep> mprep;
	Buf<vgx_mesh> mtab;
	Buf<uint64_t> contourPrefix;         // vgx_concave_contours: two exclusive prefixes over the draws (contour vertices, output vertices), [ndraws + 1] each
	// vgx_concave_triangulate (vgx_triangulate.hip): per draw its route; its ring's vertex count and three exclusive prefixes, [ndraws + 1]
	// each (VgxTriArgs); the clipping's ring-local triangles, three indices per vertex of the caller's vertex capacity
	Buf<uint32_t> triRoute; Buf<uint64_t> triPrefix; Buf<uint16_t> triIdx;
	Buf<uint32_t> triGroups;             // vgx_concave_triangulate_nested alone: per draw its group count, [ndraws + 1]
	Buf<VgxTotals> totals;
	Buf<uint32_t> textTiles;             // vgx_text_quads: first run of every tile of quads (vgx_text.hip)
	Buf<uint8_t> cullFlags; DevBuf cullPartial; // vgx_cache_cull (vgx_bounds.hip): kept flag per instance, the compaction scan's slice sums (views: as `partial`). Its own: a counted state survives the call
	Buf<uint64_t> pickKeys, pickPrefix, pickTotals; Buf<uint32_t> pickTris, pickCand; Buf<float> pickBounds; DevBuf pickPartial; // vgx_pick (vgx_pick.hip); pickPartial: slice sums (views: as `partial`). Its own: a counted state survives the call
	// vgx_pick_frame (vgx_pick.hip): per mesh of the range its state under its draw; per candidate its mesh, its covered bits (8 words) and its
	// place among the triangle / contour candidates; the triangle prefix; the totals; boxes when the caller gives none; slice sums (views: as
	// `partial`). Its own: a counted state survives the call, and vgx_pick's tables are not touched
	Buf<VgxPickfMesh> pickfState; Buf<uint32_t> pickfCand, pickfTriCand, pickfConCand, pickfCover; Buf<uint64_t> pickfPrefix, pickfTotals; Buf<float> pickfBounds; DevBuf pickfPartial;
	// vgx_pick_rect (vgx_pick_rect.hip): per mesh three words of one bit per query, its triangle count, its place among the candidates with
	// the triangle prefix, its run, per run its first mesh and two words, per block of 64 meshes two counts per query (VgxPickrArgs): 72 bytes
	// per mesh; boxes when the caller gives none; slice sums (views: as `partial`). Its own: a counted state survives the call, and the tables
	// of vgx_pick and vgx_pick_frame are not touched
	Buf<uint64_t> pickrCand, pickrInside, pickrTouch, pickrPrefix, pickrRunTouch, pickrRunInside, pickrTotals; Buf<uint32_t> pickrTris, pickrCandMesh, pickrRunOf, pickrRunFirst, pickrBlockCount, pickrBlockTop;
	Buf<float> pickrBounds; DevBuf pickrPartial;
	DevBuf updPrefix, updPartial;        // vgx_cache_layout / vgx_cache_update (vgx_update.hip); views: updPrefix = uint32_t flag word in 16 bytes, then 2 x uint64_t[ndirty + 1] prefix sums of the listed entries; updPartial = slice sums, as `partial`. Their own: a counted state survives the calls
	// vgx_raster (vgx_raster.hip): per mesh of the range its bin entries and its first entry; the (tile, mesh) entries in mesh order and
	// in tile order; the sort's temporary storage; status and entry count of the last call with their pinned mirror (as `dash`: a call
	// whose entries outgrew the tables ends with VGX_E_GROWN and the next one grows first). Its own: a counted state survives the call
	Buf<uint32_t> rasMeshEntries, rasKeys, rasVals, rasSortedKeys, rasSortedVals; Buf<uint64_t> rasMeshFirst; Buf<unsigned long long> rasState; Buf<float> rasBounds;
	Buf<VgxRasterMeshState> rasFrameMesh; // the frame-level calls: what every mesh of the range does under its draw (vgx_raster.h)
	Buf<uint32_t> rasTileTex;             // vgx_raster_textured and the levels above it: one bit per tile of the image, "a sampled mesh reaches it"
	Buf<uint32_t> rasTilePaint;           // vgx_raster_painted and vgx_raster_concave: the same for "a painted mesh reaches it"
	Buf<uint32_t> rasTileContour;         // vgx_raster_concave alone: the same for "a contour mesh reaches it"
	DevBuf rasSortTemp, rasPartial;      // rasPartial: slice sums (views: as `partial`)
	HostMirror<unsigned long long> ras;
	// vgx_raster_damaged: the frame calls' tables, but a mirror of its own -- status and entry count of the last DAMAGED call -- and what
	// the host learned from it (VgxDamageWindow, vgx_damage.h). A full render in between touches neither
	HostMirror<unsigned long long> rasDmg; VgxDamageWindow rasDmgWindow;
	// vgx_raster_commands (vgx_raster_cmds.hip): per command its state and its first chunk; per chunk its rectangle of tiles, its command
	// and its first entry; the (tile, chunk) entries in chunk order and in tile order; one bit per tile a painted command reaches; the
	// state words (VGX_RASC_*) with their pinned mirror. The capacities the kernels are told are the ones asked for with their 12.5 %,
	// not what the allocator's rounding left behind. The sort's storage and the slice sums are vgx_raster's. Its own: a counted state
	// survives the call. rascFlag: the one word of vgx_raster_cmds_from_assembly
	Buf<VgxRasterMeshState> rascCmdState; Buf<uint64_t> rascCmdFirst, rascChunkFirst; Buf<VgxRasterRect> rascChunkRect;
	Buf<uint32_t> rascChunkCmd, rascKeys, rascVals, rascSortedKeys, rascSortedVals, rascTilePaint, rascFlag; Buf<unsigned long long> rascState;
	uint64_t rascChunkCap, rascEntryCap;
	HostMirror<unsigned long long> rasc;
	// vgx_raster_commands_damaged: the same pair for the commands calls. Neither a full vgx_raster_commands nor a vgx_raster_damaged touches them
	HostMirror<unsigned long long> rascDmg; VgxDamageWindow rascDmgWindow;
	// vgx_pick_commands (vgx_pick_cmds.hip): per command its state and its first chunk; per (query, command) the largest hit triangle;
	// the state words (VGX_PICKC_*); slice sums (views: as `partial`). Its own: a counted state survives the call, and the tables of
	// vgx_pick, vgx_pick_frame and vgx_raster_commands are not touched
	Buf<VgxPickfMesh> pickcState; Buf<uint64_t> pickcFirst, pickcWords; Buf<uint32_t> pickcTop; DevBuf pickcPartial;
	// vgx_command_bounds (vgx_cmd_bounds.hip): the first chunk of every command of the range, the state words (VGX_CMDB_*), slice sums
	// (views: as `partial`). Its own: a counted state survives the call, and the tables of the calls that take the boxes are not touched
	Buf<uint64_t> cmdbFirst, cmdbWords; DevBuf cmdbPartial;
	// vgx_damage_instances (vgx_damage.hip): the flag word (in 16 bytes) and the mesh prefix of the listed entries, the scan's slice sums
	// (views: as `partial`). Its own: a counted state, and a vgx_cache_update in flight, survive the call
	DevBuf dmgPrefix, dmgPartial;
	// vgx_dash (vgx_dash.hip): per-draw patterns, per-list records, per-segment prefix sums (S and the overflow guard), per-range sums; the
	// segment count of the last call in pinned memory (copied behind the call, read by the next call once its event has passed: a call
	// whose lists outgrew dashG ends with VGX_E_GROWN and the next one grows first, as vgx_tessellate_immediate does)
	Buf<VgxDashPat> dashPat; Buf<VgxDashListRec> dashLists; Buf<uint64_t> dashG, dashGhi;
	DevBuf dashRange;                    // views: uint64_t range sums, range offsets [2 x VGX_DASH_RANGES each], totals [4]
	HostMirror<unsigned long long> dash;
	// vgx_tessellate_dashed (vgx_dashframe.hip): the second set of mesh tables (the flatten stage writes one set, the frame's meshes go to the
	// other; the two swap roles behind the call), per source mesh the list of the dash pass and D(m), the pieces' records, the dash pass's
	// totals, and the need of the last call (pieces, their vertices, source meshes) with its pinned mirror, as `imm`. The pieces' vertices
	// lie BEHIND the flatten stage's heap in `poly`: pieceVerts of its vertices are theirs (ensureMeshBuffers keeps them out of caps)
	Buf<VgxMeshDesc> mdesc2; Buf<VgxMeshPrep> mprep2; Buf<vgx_mesh> mtab2; Buf<vgx_subpath> dfLists, dfPieceSubs; Buf<uint32_t> dfListDraw, dfPieceDraw, dfPieceSrc;
	Buf<uint64_t> dfDashedBefore, dfNeed; Buf<VgxTotals> dfTotals;
	uint64_t pieceVerts;
	HostMirror<unsigned long long> df;
	Buf<VgxTileRec> tileTab;             // k_emit_tiles (vgx_tile.hip): the tile table of the current call
	DevBuf psTemp;                       // vgx_pathset_create: temporaries of the device-side build (vgx_pathset.hip); views: VgxPsTotals, uint32_t words, VgxPsM and Sum3 slice sums at byte offsets
	hipStream_t psStream;                // ... its stream (created at the first call)
	struct VgxPsTotals* hostPs;          // ... pinned: what the build reports
	void* psImage; size_t psImageCap;    // ... pinned: the raw part of a frame-sized set, assembled here and uploaded in one copy
	DevBuf psPool[VGX_PS_POOL];          // ... blobs of dropped frame-sized sets, recycled (hipFree synchronises). Not scratch: never grown, not on the list
	Buf<uint64_t> f1SegDraw; Buf<VgxF1Seg> f1Segs; // vgx_flatten (vgx_flat1.hip): segment table, look-back records
	// what the last vgx_flatten call produced (copied to pinned memory behind the call, read by the next call WITHOUT waiting for
	// it): polyline vertices per command instance decide how many commands a segment may hold before its leaves overflow the list
	unsigned long long* hostF1;          // pinned: [0] vertices, [1] command instances, [2] tag of the batch they belong to
	uint64_t f1Tag;
	Buf<VgxGatherWire> gatherSizes;      // vgx_gather_sizes: one record per rank
	DevBuf partBounds;                   // vgx_partition; views: uint64_t [nparts + 1] bounds, behind them [nparts] weights
	struct VgxRccl* rccl;                // RCCL entry points, bound at the first vgx_gather* call
	VgxOptions opt;                      // read from the environment ONCE at vgx_create (vgx_route_plan.h)
	VgxRouteState route;                 // the ordinary pipeline's flatten route and what its tables hold
	// instanced batches (vgx_inst.hip), grouped mode: every vgx_tessellate sorts the draws by path first (k_inst_hist / k_inst_plan / k_inst_scatter)
	Buf<uint32_t> instHist, instCursor, instTaskPath, instOrder; Buf<uint64_t> instKeyStart, instStart, instTaskStart;
	Buf<uint32_t> instPerm, instPermHist; // periodic mode, instances of different scales: the instances sorted by tolerance class (vgx_launch_inst_perm)
	// template mode (vgx_tmpl.hip): the first period of an instanced batch whose instances differ in transform / colours only,
	// flattened once in local space by the last vgx_tessellate_count
	VgxTemplate tmpl;                    // the current template
	// element capacities of the buffers above. Never lifted: only ensureMeshBuffers and ensureCmdScratch write it, from the buffers'
	// capacities, so every launch may trust it; a launch that needs other bounds (a sizing pass, the caller's capacities) is given them
	VgxCaps caps;
	VgxTotals* hostTotals; // pinned
	VgxImmState imm;
	VgxCounted counted;
	// profiling
	int profiling;
	// a ring of event sets, one per profiled call: vgx_get_stage_times reads the last call's, vgx_get_stage_times_avg the average over
	// the last calls (a caller that times K back-to-back calls gets per-kernel durations of THOSE calls, without a sync in between)
	hipEvent_t ev[VGX_PROF_RING][VGX_MAX_STAGES + 1];
	const char* evName[VGX_PROF_RING][VGX_MAX_STAGES];
	uint32_t numEv[VGX_PROF_RING];
	uint64_t profCalls; // profiled calls since profiling was switched on
	uint32_t evSet;     // set of the current call
	bool evCreated;
};

static void vgx_rccl_release(vgx_ctx* ctx);
// Every call that takes the ground from under the current template (its scratch, its path set, its mode) ends it here: the next
// vgx_tessellate wants a count again
static void tmplDrop(vgx_ctx* ctx) { ctx->tmpl.on = false; }

namespace {

#define HIPCHK(ctx, call)                                 \
	do {                                                  \
		hipError_t e_ = (call);                           \
		if (e_ != hipSuccess) {                           \
			(ctx)->lastHipError = (int)e_;                \
			return VGX_E_HIP;                             \
		}                                                 \
	} while (0)

// the context's scratch grows here (vgx_scratch.h): a raw buffer by bytes, a typed one by elements
int ensure(vgx_ctx* ctx, DevBuf& b, size_t bytes) { return vgx_scratch_grow(ctx->scratch, b, bytes, &ctx->lastHipError); }
template<class T> int ensure(vgx_ctx* ctx, Buf<T>& b, uint64_t items) { return b.grow(ctx->scratch, items, &ctx->lastHipError); }

// Every entry point that takes a context runs on the context's device, whatever device is current on the calling
// thread (a torch rank, another context), and leaves the caller's current device as it found it.
struct DeviceGuard
{
	int prev;
	bool switched;
	explicit DeviceGuard(const vgx_ctx* ctx) : prev(-1), switched(false)
	{
		if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device) { switched = hipSetDevice(ctx->device) == hipSuccess; }
	}
	~DeviceGuard() { if (switched) { (void)hipSetDevice(prev); } }
};

// The alignment every entry that writes a vgx_mesh_out asks of it (include/vgx.h): that of the element types -- the emit kernels
// store whole elements, never less. A pointer below it is refused on the host, before anything is enqueued.
static bool meshOutMisaligned(const vgx_mesh_out* out)
{
	return ((uintptr_t)out->pos & 7u) || ((uintptr_t)out->color & 3u) || ((uintptr_t)out->idx & 1u) || ((uintptr_t)out->meshes & 7u);
}

// Launch failures (bad configuration, device lost) surface as hipGetLastError: every entry point that enqueues kernels
// ends with this instead of pretending success.
int launchStatus(vgx_ctx* ctx)
{
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) {
		ctx->lastHipError = (int)e;
		return VGX_E_HIP;
	}
	if (ctx->pendingHipError) { // an asynchronous memset of this call failed
		ctx->lastHipError = ctx->pendingHipError;
		ctx->pendingHipError = 0;
		return VGX_E_HIP;
	}
	return VGX_OK;
}

void noteHip(vgx_ctx* ctx, hipError_t e)
{
	if (e != hipSuccess && !ctx->pendingHipError) { ctx->pendingHipError = (int)e; }
}

} // namespace

template<class T> int HostMirror<T>::create(vgx_ctx* ctx, uint32_t count)
{
	if (host) { return VGX_OK; }
	HIPCHK(ctx, hipHostMalloc((void**)&host, count * sizeof(T), hipHostMallocDefault));
	const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
	if (e != hipSuccess) { (void)hipHostFree(host); host = nullptr; ctx->lastHipError = (int)e; return VGX_E_HIP; }
	memset(host, 0, count * sizeof(T));
	n = count;
	pending = false;
	return VGX_OK;
}

template<class T> void HostMirror<T>::push(vgx_ctx* ctx, const void* dev, hipStream_t s)
{
	noteHip(ctx, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
	noteHip(ctx, hipEventRecord(ev, s));
	pending = true;
}

template<class T> bool HostMirror<T>::landed()
{
	if (!pending || hipEventQuery(ev) != hipSuccess) { return false; }
	pending = false;
	return true;
}

template<class T> void HostMirror<T>::release()
{
	if (host) { (void)hipHostFree(host); (void)hipEventDestroy(ev); }
}

namespace {

void mark(vgx_ctx* ctx, hipStream_t s, const char* name)
{
	const uint32_t k = ctx->evSet;
	if (!ctx->profiling || ctx->numEv[k] >= VGX_MAX_STAGES) {
		return;
	}
	ctx->evName[k][ctx->numEv[k]] = name;
	++ctx->numEv[k];
	(void)hipEventRecord(ctx->ev[k][ctx->numEv[k]], s);
}

void markBegin(vgx_ctx* ctx, hipStream_t s)
{
	if (!ctx->profiling) {
		return;
	}
	if (!ctx->evCreated) {
		for (int r = 0; r < VGX_PROF_RING; ++r) { for (int i = 0; i <= VGX_MAX_STAGES; ++i) { (void)hipEventCreate(&ctx->ev[r][i]); } }
		ctx->evCreated = true;
	}
	ctx->evSet = (uint32_t)(ctx->profCalls % VGX_PROF_RING);
	++ctx->profCalls;
	ctx->numEv[ctx->evSet] = 0;
	(void)hipEventRecord(ctx->ev[ctx->evSet][0], s);
}

struct OpCacheInst // shape cache: vertices / indices / meshes of every instance's mesh range -> output offsets
{
	vgx_cache_desc cache;
	const vgx_cache_instance* inst;
	uint64_t ninst;
	uint64_t* meshPrefix;
	uint64_t* vertPrefix;
	uint64_t* idxPrefix;
	VgxTotals* totals;
	VgxCaps caps;
	__device__ uint64_t size() const { return ninst; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		VgxRangeCounts n; // the per-instance rule vgx_cache_layout shares (vgx_update.h)
		const vgx_cache_instance in = inst[i];
		if (!vgx_cache_range_counts(cache, in, &n)) { set_status(totals, VGX_E_INVALID_ARG); return r; }
		r.a = n.meshes; r.b = n.vertices; r.c = n.indices;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const { meshPrefix[i] = e.a; vertPrefix[i] = e.b; idxPrefix[i] = e.c; }
	__device__ void finish(Sum3 t) const
	{
		meshPrefix[ninst] = t.a; vertPrefix[ninst] = t.b; idxPrefix[ninst] = t.c;
		totals->sizes.num_meshes = t.a;
		totals->sizes.num_vertices = t.b;
		totals->sizes.num_indices = t.c;
		if (t.a > caps.meshes || t.b > caps.vertices || t.c > caps.indices) { set_status(totals, VGX_E_NOSPACE); }
	}
};

struct OpConcaveFills // concave fills: vertices / indices of every fill's mesh -> offsets + mesh records
{
	const vgx_contour* contours;
	uint64_t ncontours;
	const vgx_concave_fill* fills;
	uint64_t nfills;
	vgx_mesh* mtab;
	vgx_mesh* meshesOut; // caller's table (may be null)
	VgxTotals* totals;
	VgxCaps caps;
	__device__ uint64_t size() const { return nfills; }
	__device__ bool counts(uint64_t i, uint64_t* nv, uint64_t* ni) const
	{
		const vgx_concave_fill f = fills[i];
		*nv = 0; *ni = 0;
		if (f.first_contour > ncontours || (uint64_t)f.num_contours > ncontours - f.first_contour) { return false; }
		uint64_t cv = 0; // contour vertices of the fill (its contours are stored back to back)
		if (f.num_contours) {
			const vgx_contour c0 = contours[f.first_contour], c1 = contours[f.first_contour + f.num_contours - 1];
			if (c1.first_vertex < c0.first_vertex) { return false; }
			cv = c1.first_vertex + c1.num_vertices - c0.first_vertex;
		}
		*nv = 2 * cv + f.num_tess_vertices;
		*ni = 6 * cv + f.num_tess_indices;
		return true;
	}
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		uint64_t nv, ni;
		if (!counts(i, &nv, &ni)) { set_status(totals, VGX_E_INVALID_ARG); return r; }
		if (nv > 65536u) { set_status(totals, VGX_E_MESH_TOO_LARGE); } // uint16 indices
		r.a = nv; r.b = ni;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		uint64_t nv, ni;
		(void)counts(i, &nv, &ni);
		vgx_mesh m;
		m.first_vertex = e.a; m.first_index = e.b;
		m.num_vertices = (uint32_t)nv; m.num_indices = (uint32_t)ni;
		m.draw = (uint32_t)i;
		m.subpath_kind = (uint32_t)VGX_MESH_CONCAVE_FILL_AA << 28;
		mtab[i] = m;
		if (meshesOut && i < caps.meshes) { meshesOut[i] = m; }
	}
	__device__ void finish(Sum3 t) const
	{
		totals->sizes.num_meshes = nfills;
		totals->sizes.num_vertices = t.a;
		totals->sizes.num_indices = t.b;
		if (t.a > caps.vertices || t.b > caps.indices || nfills > caps.meshes) { set_status(totals, VGX_E_NOSPACE); }
	}
};

struct OpContourDraws // vgx_concave_contours: per draw its contour vertices, output vertices and meshes -> offsets + mesh records
{
	const vgx_subpath* subs;
	const vgx_draw_info* dinfo;
	const vgx_draw* draws;
	uint64_t ndraws;
	uint64_t* contourPrefix; // [ndraws + 1]
	uint64_t* vertexPrefix;  // [ndraws + 1]
	vgx_mesh* meshesOut;     // caller's table (may be null)
	VgxTotals* totals;
	VgxCaps caps;
	__device__ uint64_t size() const { return ndraws; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const vgx_draw d = draws[i];
		uint64_t V;
		const int made = contours_draw_counts(d, dinfo[i], subs, &V);
		if (made < 0) { set_status(totals, VGX_E_INVALID_ARG); }
		if (made <= 0) { return r; }
		const bool aa = (d.fill_flags & VGX_FILL_AA) != 0u;
		if ((aa ? 2 * V : V) > 65536u) { set_status(totals, VGX_E_MESH_TOO_LARGE); } // uint16 indices
		r.a = V; r.b = aa ? 3 * V : V; r.c = aa ? 2u : 1u;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		contourPrefix[i] = e.a; vertexPrefix[i] = e.b;
		const vgx_draw d = draws[i];
		uint64_t V;
		if (contours_draw_counts(d, dinfo[i], subs, &V) <= 0 || !meshesOut) { return; }
		vgx_mesh m[2];
		const uint32_t n = contours_draw_meshes(d, (uint32_t)i, V, e.b, 2 * e.a + 3 * (e.b - e.a), m);
		for (uint32_t k = 0; k < n; ++k) { if (e.c + k < caps.meshes) { meshesOut[e.c + k] = m[k]; } }
	}
	__device__ void finish(Sum3 t) const
	{
		contourPrefix[ndraws] = t.a; vertexPrefix[ndraws] = t.b;
		const uint64_t indices = 2 * t.a + 3 * (t.b - t.a);
		totals->sizes.num_meshes = t.c;
		totals->sizes.num_vertices = t.b;
		totals->sizes.num_indices = indices;
		if (t.b > caps.vertices || indices > caps.indices || t.c > caps.meshes) { set_status(totals, VGX_E_NOSPACE); }
	}
};

struct OpSubMeshes // stroker-level entry: one or two meshes per vertex list -> mesh descriptors + closed-form sizes
{
	const vgx_subpath* subs;
	const uint32_t* subDraw;
	const vgx_draw* draws;
	uint64_t nsubs, ndraws;
	VgxMeshDesc* mdesc;
	vgx_mesh* mtab;
	VgxTotals* totals;
	__device__ uint64_t size() const { return nsubs; }
	__device__ Sum3 load(uint64_t i) const
	{
		Sum3 r = sum3_zero();
		const uint32_t di = subDraw[i];
		if (di >= ndraws) { set_status(totals, VGX_E_INVALID_ARG); return r; }
		const vgx_draw* d = draws + di;
		const uint32_t n = subs[i].num_vertices;
		const uint32_t sf = d->stroke_flags;
		if ((sf & VGX_STROKE_ENABLE) && (VGX_STROKE_CAP(sf) > 2u || VGX_STROKE_JOIN(sf) > 2u)) { set_status(totals, VGX_E_INVALID_ARG); return r; }
		r.a = (((d->fill_flags & VGX_FILL_ENABLE) && n >= 3) ? 1u : 0u) + (((sf & VGX_STROKE_ENABLE) && n >= 2) ? 1u : 0u);
		r.b = n;
		return r;
	}
	__device__ void store(uint64_t i, Sum3 e) const
	{
		const uint32_t di = subDraw[i];
		if (di >= ndraws) { return; }
		const vgx_draw* d = draws + di;
		const vgx_subpath sp = subs[i];
		const bool closed = (sp.flags & 1u) != 0;
		uint64_t m = e.a;
		if ((d->fill_flags & VGX_FILL_ENABLE) && sp.num_vertices >= 3) {
			vgx_write_mesh(mdesc, mtab, m, d, di, (uint32_t)i, (d->fill_flags & VGX_FILL_AA) ? VGX_MESH_FILL_AA : VGX_MESH_FILL, closed, sp.first_vertex, sp.num_vertices);
			++m;
		}
		const uint32_t sf = d->stroke_flags;
		if ((sf & VGX_STROKE_ENABLE) && sp.num_vertices >= 2) {
			const uint32_t k = !(sf & VGX_STROKE_AA) ? VGX_MESH_STROKE : ((sf & VGX_STROKE_THIN) ? VGX_MESH_STROKE_AA_THIN : VGX_MESH_STROKE_AA);
			if (vgx_write_mesh(mdesc, mtab, m, d, di, (uint32_t)i, k, closed, sp.first_vertex, sp.num_vertices)) { atomicAdd(&totals->num_round_meshes, 1u); }
		}
	}
	__device__ void finish(Sum3 t) const
	{
		totals->sizes.num_meshes = t.a;
		totals->sizes.num_poly_vertices = t.b;
		totals->sizes.num_subpaths = nsubs;
	}
};

__global__ void k_tmpl_nospace(VgxTotals* t, vgx_sizes need, uint32_t aux)
{
	t->sizes = need;
	t->status = VGX_E_NOSPACE;
	t->fail_reason = VGX_FAIL_OUT_CAPACITY;
	t->fail_aux = aux;
}

__global__ void k_publish(const VgxTotals* t, vgx_sizes* devSizes, uint32_t* devStatus)
{
	if (devSizes) { *devSizes = t->sizes; }
	if (devStatus) { *devStatus = t->status; }
}

// ---- pipeline pieces ----------------------------------------------------------------------------------
VgxFlattenArgs flattenArgs(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int applyTransform)
{
	VgxFlattenArgs a;
	a.ps = ps->dev;
	a.draws = draws;
	a.ndraws = ndraws;
	a.cmd_prefix = (const uint64_t*)ctx->cmdPrefix.p;
	a.sub_prefix = ctx->subPrefix.ptr();
	a.cmd_cnt = ctx->cmdCnt.ptr();
	a.dinfo = ctx->dinfo.ptr();
	a.poly = (float*)ctx->poly.p;
	a.subs = ctx->subs.ptr();
	a.mdesc = ctx->mdesc.ptr();
	a.mprep = nullptr;
	a.mtab = ctx->mtab.ptr();
	a.totals = ctx->totals.ptr();
	a.caps = ctx->caps;
	a.apply_transform = applyTransform;
	a.sub_rec = ctx->subFirst.ptr();
	a.build_mode = 0;
	a.thin_static = ps->thinStatic ? ctx->opt.thinStatic : 0;
	a.leaf_overflow = ctx->leafOverflow.ptr();
	a.serial_list = ctx->serialList.ptr();
	a.inst_period = 0; a.inst_block = ctx->opt.instBlock; a.inst_waves = ctx->opt.instWaves; a.inst_perm = nullptr;
	a.inst_order = nullptr; a.inst_start = nullptr; a.inst_task_start = nullptr; a.inst_task_path = nullptr;
	return a;
}

// Period the instanced kernel may assume for `ndraws` draws (0: command-parallel kernel); the device re-checks it on every call (OpCmdPrefix)
uint32_t instPeriodFor(const vgx_ctx* ctx, uint64_t ndraws) { return vgx_period_usable(ctx->opt, ctx->route.chosen.period, ndraws) ? ctx->route.chosen.period : 0; }

// The flatten route and the template the last count chose no longer hold
void forgetRoutes(vgx_ctx* ctx) { ctx->route.chosen = vgx_route_none(); tmplDrop(ctx); }

// Grouped mode for this call: the count pass chose it and the sort buffers hold a batch of this size over this path set.
bool instGroupedFor(const vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws)
{
	const VgxRouteState& r = ctx->route;
	return r.chosen.kind == VGX_ROUTE_GROUPED && !instPeriodFor(ctx, ndraws) && ndraws > VGX_SMALL_DRAWS && ndraws <= r.instDraws
		&& ps->dev.npaths <= r.instPaths && (uint64_t)ps->dev.npaths * r.chosen.classes <= r.instKeys && ndraws < 0xFFFFFFFFull;
}

// The one-walk route for this call: what the last count decided and sized, for this path set
bool oneWalkFor(const vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws)
{
	const VgxRouteState& r = ctx->route;
	return r.chosen.kind == VGX_ROUTE_ONE_WALK && ps == r.f1Ps && ps->gen == r.f1PsGen && !instPeriodFor(ctx, ndraws)
		&& vgx_f1_route_segments(ps->maxCmdsPerPath, ndraws, r.chosen.f1SegMax) <= r.chosen.f1SegBound;
}

// does an _emit follow its count (ctx->counted) on the same batch?
bool followsCount(const vgx_ctx* ctx, VgxCountedStage stage, const vgx_pathset* ps, const vgx_draw* draws, uint64_t n)
{
	const VgxCounted& c = ctx->counted;
	return c.stage == stage && c.ps == ps && c.draws == draws && c.ndraws == n;
}

// the smallest of several capacities: what a group of buffers that are indexed alike holds
uint64_t minOf(std::initializer_list<uint64_t> caps) { return std::min(caps); }

// scratch of the grouped mode: histogram / cursor / ranges per path, task table, draw order
int ensureInstGroup(vgx_ctx* ctx, uint32_t npaths, uint32_t nc, uint64_t ndraws, bool full)
{
	int st;
	const size_t nkeys = (size_t)npaths * nc;
	if ((st = ensure(ctx, ctx->instHist, nkeys + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->instStart, (size_t)npaths + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->instTaskStart, (size_t)npaths + 1)) != VGX_OK) { return st; }
	if (full) {
		const uint64_t tasks = ndraws / 64 + (uint64_t)npaths + 2; // every used path rounds up once
		if ((st = ensure(ctx, ctx->instCursor, nkeys + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->instKeyStart, nkeys + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->instTaskPath, tasks)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->instOrder, ndraws + 1)) != VGX_OK) { return st; }
		ctx->route.instTasks = ctx->instTaskPath.items();
		ctx->route.instDraws = ctx->instOrder.items() - 1;
		ctx->route.instKeys = minOf({ ctx->instHist.items() - 1, ctx->instCursor.items() - 1, ctx->instKeyStart.items() - 1 });
		ctx->route.instPaths = minOf({ ctx->instStart.items() - 1, ctx->instTaskStart.items() - 1 });
	}
	return VGX_OK;
}

void setInstArgs(vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws, VgxFlattenArgs& a)
{
	a.inst_period = instPeriodFor(ctx, ndraws);
	a.inst_perm = nullptr;
	if (a.inst_period && ctx->route.chosen.permute && ndraws / a.inst_period <= ctx->instPerm.items()) { a.inst_perm = ctx->instPerm.ptr(); }
	if (instGroupedFor(ctx, ps, ndraws)) {
		a.inst_order = ctx->instOrder.ptr(); a.inst_start = ctx->instStart.ptr();
		a.inst_task_start = ctx->instTaskStart.ptr(); a.inst_task_path = ctx->instTaskPath.ptr();
	}
}

int ensureDrawBuffers(vgx_ctx* ctx, uint64_t ndraws)
{
	int st;
	if ((st = ensure(ctx, ctx->cmdPrefix, (ndraws + 1) * sizeof(uint64_t))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->subPrefix, ndraws + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dinfo, ndraws + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->serialList, ndraws + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	// what the grow-only buffers hold, not the last batch's size
	ctx->route.capDraws = minOf({ ctx->cmdPrefix.cap / sizeof(uint64_t) - 1, ctx->dinfo.items() - 1, ctx->serialList.items() - 1, ctx->subPrefix.items() - 1 });
	return VGX_OK;
}

int readTotals(vgx_ctx* ctx, hipStream_t s)
{
	HIPCHK(ctx, hipMemcpyAsync(ctx->hostTotals, ctx->totals.p, sizeof(VgxTotals), hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipStreamSynchronize(s));
	return VGX_OK;
}

// the command-instance scan; `cmdCap`: the command instances the per-command scratch holds for this launch (~0: not checked)
OpCmdPrefix cmdPrefixOp(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, uint64_t cmdCap, uint32_t instPeriod)
{
	OpCmdPrefix op;
	op.draws = draws; op.pathCmdBegin = ps->dev.path_cmd_begin; op.npaths = ps->dev.npaths; op.ndraws = ndraws;
	op.prefix = (uint64_t*)ctx->cmdPrefix.p; op.totals = ctx->totals.ptr(); op.cap = cmdCap;
	op.pathSubBegin = ps->dev.path_sub_begin; op.subPrefix = ctx->subPrefix.ptr();
	op.period = instPeriod;
	return op;
}

// stage 1: command-instance prefix
void runCmdPrefix(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, uint64_t cmdCap, hipStream_t s, uint32_t instPeriod = 0)
{
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	vgx_device_scan(cmdPrefixOp(ctx, ps, draws, ndraws, cmdCap, instPeriod), (Sum3*)ctx->partial.p, s, ndraws);
	mark(ctx, s, "scan_cmd_prefix");
}

// stage 2: flatten count + draw scan, both checked against `caps`
void runFlattenCount(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const VgxCaps& caps, hipStream_t s)
{
	noteHip(ctx, hipMemsetAsync(ctx->dinfo.p, 0, ndraws * sizeof(vgx_draw_info), s));
	VgxFlattenArgs a = flattenArgs(ctx, ps, draws, ndraws, 1);
	a.caps = caps;
	vgx_launch_flatten(false, a, VGX_GRID_BLOCKS, s);
	mark(ctx, s, "flatten_count");
	OpDrawInfo op;
	op.dinfo = ctx->dinfo.ptr(); op.ndraws = ndraws; op.totals = ctx->totals.ptr(); op.caps = caps; op.keepPolyBase = 0;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ndraws);
	mark(ctx, s, "scan_draws");
}

// single-pass flatten of the steady-state entry point: build (subdivide once, polyline -> heap) -> scan -> gather
void runFlattenBuild(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, hipStream_t s)
{
	noteHip(ctx, hipMemsetAsync(ctx->dinfo.p, 0, ndraws * sizeof(vgx_draw_info), s));
	VgxFlattenArgs a = flattenArgs(ctx, ps, draws, ndraws, 1);
	a.build_mode = 1;
	setInstArgs(ctx, ps, ndraws, a); // periodic: the same value runCmdPrefix checked the draws against
	if (a.inst_perm) { // periodic mode, instances of different scales: this batch's instances sorted by tolerance class
		vgx_launch_inst_perm(draws, ndraws / a.inst_period, a.inst_period, ctx->route.chosen.classes, ctx->instPermHist.ptr(), ctx->instPerm.ptr(), ctx->totals.ptr(), ctx->opt.instPerm == 2, s);
		mark(ctx, s, "inst_group");
	}
	if (a.inst_order) { // grouped mode: this batch's draws sorted by path
		vgx_launch_inst_group(draws, ndraws, ps->dev.npaths, ctx->route.chosen.classes, ctx->instHist.ptr(), ctx->instCursor.ptr(), ctx->instKeyStart.ptr(),
			ctx->instStart.ptr(), ctx->instTaskStart.ptr(), ctx->instTaskPath.ptr(), ctx->route.instTasks, ctx->instOrder.ptr(),
			ctx->totals.ptr(), ctx->partial.p, s);
		mark(ctx, s, "inst_group");
	}
	a.mprep = ctx->mprep.ptr(); // k_flatten_gather / k_flatten_serial write the per-mesh constants with the descriptors
	vgx_launch_flatten_build(a, ctx->opt.buildWaves, s);
	mark(ctx, s, "flatten_build");
	OpDrawInfo op;
	op.dinfo = ctx->dinfo.ptr(); op.ndraws = ndraws; op.totals = ctx->totals.ptr(); op.caps = ctx->caps; op.keepPolyBase = 1;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ndraws);
	mark(ctx, s, "scan_draws");
	vgx_launch_flatten_gather(a, s);
	mark(ctx, s, "flatten_gather");
}

// flattenArgs for a call that writes the caller's ordered outputs: no mesh tables, no bounds
VgxFlattenArgs flattenOutArgs(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int applyTransform, float* poly, vgx_subpath* subs)
{
	VgxFlattenArgs a = flattenArgs(ctx, ps, draws, ndraws, applyTransform);
	a.poly = poly; a.subs = subs;
	a.mdesc = nullptr; a.mtab = nullptr;
	a.caps.poly_vertices = ~0ull; a.caps.subpaths = ~0ull; a.caps.meshes = ~0ull;
	return a;
}

// The one-walk launch sequence (vgx_flat1.hip) behind the command prefix, over the outputs of `a`: the exact builder's count, k_flat1, its draws,
// the totals (+ the caller's device words). `x`: capacities, bucket size and tag, from the caller; tables of `segBound` segments; `cap`: the kernel instance
void runOneWalk(vgx_ctx* ctx, const vgx_pathset* ps, const VgxFlattenArgs& a, VgxF1Args x, uint64_t segBound, int cap, vgx_sizes* dev_sizes, uint32_t* dev_status, hipStream_t s)
{
	x.seg_draw = ctx->f1SegDraw.ptr(); x.segs = ctx->f1Segs.ptr(); x.grps = x.segs + segBound;
	x.pass = 0; x.read_flags = 0; x.has_empty = ps->hasEmpty ? 1 : 0;
	if (ps->hasSerial) { // statically serial paths: the exact builder counts their draws first (it marks them in dinfo)
		noteHip(ctx, hipMemsetAsync(ctx->dinfo.p, 0, a.ndraws * sizeof(vgx_draw_info), s));
		VgxFlattenArgs ac = a;
		ac.mdesc = nullptr; ac.mtab = nullptr; ac.mprep = nullptr;
		vgx_launch_flatten_serial(false, ac, s);
	}
	vgx_launch_flat1(a, x, ctx->opt.f1Waves ? ctx->opt.f1Waves : 2048, cap, ps->hasSerial, s);
	// the exact builder's draws (mesh descriptors too where `a` has them): every draw when the set has serial paths, else those the kernel listed
	VgxFlattenArgs ae = a;
	ae.build_mode = ps->hasSerial ? 0 : 1;
	vgx_launch_flatten_serial(true, ae, s);
	vgx_launch_flat1_publish(a, x, dev_sizes, dev_status, s);
	mark(ctx, s, "flatten_one_walk");
}

// The flatten stage of an asynchronous call (vgx_tessellate, the immediate and the dashed call), by the route the context holds. One-walk (vgx_flat1.hip),
// for batches of LONG curves, where k_flatten_build's lanes spill their leaves past the LDS slots: command prefix -> k_flat1 (the polyline lands dense and
// in draw order, the per-draw and sub-path records complete) -> the exact builder's draws -> totals -> mesh descriptors. No heap, no scan over the draws
void runFlattenStage(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, hipStream_t s)
{
	if (!oneWalkFor(ctx, ps, ndraws)) { // command prefix (the period re-checked) -> k_flatten_build's sequence
		runCmdPrefix(ctx, ps, draws, ndraws, ctx->caps.cmd_instances, s, instPeriodFor(ctx, ndraws));
		runFlattenBuild(ctx, ps, draws, ndraws, s);
		return;
	}
	runCmdPrefix(ctx, ps, draws, ndraws, ~0ull, s); // k_flat1 needs no per-command scratch
	VgxFlattenArgs a = flattenArgs(ctx, ps, draws, ndraws, 1);
	a.mprep = ctx->mprep.ptr(); // k_flatten_serial / the gather write the per-mesh constants with the descriptors
	const VgxRoute& r = ctx->route.chosen;
	VgxF1Args x;
	x.cap_poly = ctx->caps.poly_vertices; x.cap_subs = ctx->caps.subpaths; x.cap_meshes = ctx->caps.meshes; x.seg_max = r.f1SegMax; x.tag = 0;
	runOneWalk(ctx, ps, a, x, r.f1SegBound, r.f1Cap, nullptr, nullptr, s);
	vgx_launch_flatten_gather_ordered(a, s);
	mark(ctx, s, "flatten_gather");
}

// the stroke / fill kernels' arguments over the context's scratch, no output buffers yet
VgxStrokeArgs strokeArgs(vgx_ctx* ctx, const vgx_draw* draws, const float* poly, const VgxCaps& caps)
{
	VgxStrokeArgs a;
	a.draws = draws; a.poly = poly ? poly : (const float*)ctx->poly.p; a.mdesc = ctx->mdesc.ptr();
	a.elem_prefix = nullptr; a.elem_prefix_fill = ctx->elemPrefix.ptr(); a.elem_prefix_stroke = ctx->elemPrefixS.ptr();
	a.mprep = ctx->mprep.ptr(); a.mtab = ctx->mtab.ptr();
	a.pos = nullptr; a.color = nullptr; a.idx = nullptr; a.meshes_out = nullptr; a.mesh_base = nullptr;
	a.totals = ctx->totals.ptr(); a.caps = caps; a.tile_mode = 0; a.no_long = 0;
	return a;
}

// The bounds of a count: the context's scratch, no output capacities
VgxCaps sizingCaps(const vgx_ctx* ctx) { VgxCaps c = ctx->caps; c.vertices = ~0ull; c.indices = ~0ull; return c; }
// The bounds of a call that writes into `out`: the context's scratch, the caller's vertex / index / mesh-table capacities
VgxCaps outCapsFor(const vgx_ctx* ctx, const vgx_mesh_out* out)
{
	VgxCaps c = ctx->caps;
	c.vertices = out->cap_vertices;
	c.indices = out->cap_indices;
	if (out->meshes && out->cap_meshes < c.meshes) { c.meshes = out->cap_meshes; }
	return c;
}

// the call's totals into the caller's device words, if it asked for them
void publish(vgx_ctx* ctx, vgx_sizes* dev_sizes, uint32_t* dev_status, hipStream_t s)
{
	if (dev_sizes || dev_status) { hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, s, ctx->totals.ptr(), dev_sizes, dev_status); }
}

// prepDone: the flatten stage already wrote the per-mesh constants (single-pass pipeline), no k_mesh_prepare pass
void runStrokeCount(vgx_ctx* ctx, const vgx_draw* draws, const VgxCaps& outCaps, int checkCaps, hipStream_t s, const float* poly = nullptr, bool prepDone = false, vgx_mesh* meshesOut = nullptr)
{
	VgxStrokeArgs a = strokeArgs(ctx, draws, poly, outCaps);
	if (!prepDone) { vgx_launch_mesh_prepare(a, s); }
	vgx_launch_stroke(false, a, 32768, s); // k_round_sizes: Round-join mesh sizes (exits immediately without Round joins); one wave per mesh: 10 000 long polylines want more than 4 096 waves
	mark(ctx, s, "mesh_prepare");
	OpMeshAll op;
	op.mdesc = ctx->mdesc.ptr(); op.mtab = ctx->mtab.ptr();
	op.prefixFill = ctx->elemPrefix.ptr(); op.prefixStroke = ctx->elemPrefixS.ptr();
	op.totals = ctx->totals.ptr(); op.caps = outCaps; op.checkCaps = checkCaps;
	op.meshesOut = meshesOut; op.fixedSize = 0; op.fixedCount = 0;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ctx->caps.meshes);
	mark(ctx, s, "scan_meshes");
}

// Draw-command assembly (armed by vgx_set_assembly): partition of the mesh sequence into vertex buffers, per-mesh index
// base, draw-command table. Runs between the scan over meshes and the emit kernels, which add the base to every index.
int runAssemble(vgx_ctx* ctx, const vgx_mesh_out* out, hipStream_t s, const vgx_draw* draws = nullptr)
{
	const uint32_t maxVB = ctx->asmCfg.max_vb_vertices ? ctx->asmCfg.max_vb_vertices : 65536u;
	const uint64_t meshCap = ctx->mtab.items();
	uint64_t need = 2 * (out->cap_vertices / maxVB) + 4; // two consecutive vertex buffers always hold > maxVB vertices
	if (need > meshCap + 1) { need = meshCap + 1; }
	if (meshCap >= 0xFFFFFFFFull) { return VGX_E_RANGE; } // the jump tables hold 32-bit mesh indices
	uint64_t capStart = 2;
	while (capStart < need) { capStart <<= 1; }
	int st;
	if ((st = ensure(ctx, ctx->asmJump0, meshCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->asmJump1, meshCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->asmStart, capStart)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->meshBase, meshCap + 1)) != VGX_OK) { return st; }
	VgxAsmArgs a;
	a.mtab = ctx->mtab.ptr();
	a.jump0 = ctx->asmJump0.ptr(); a.jump1 = ctx->asmJump1.ptr();
	a.start = ctx->asmStart.ptr(); a.cap_start = capStart;
	a.mesh_base = ctx->meshBase.ptr();
	a.drawcmds = ctx->asmCfg.drawcmds; a.cap_drawcmds = ctx->asmCfg.cap_drawcmds; a.dev_num_drawcmds = ctx->asmCfg.dev_num_drawcmds;
	a.max_vb = maxVB;
	a.totals = ctx->totals.ptr();
	a.flags = draws ? ctx->asmCfg.flags : 0u; // no draw records at this level (shape cache): one state
	a.mdesc = ctx->mdesc.ptr(); a.draws = draws;
	a.mesh_cmd = a.jump0;
	a.partial = ctx->partial.p;
	a.max_meshes = meshCap;
	a.scan_bound = (out->meshes && out->cap_meshes && out->cap_meshes < meshCap) ? out->cap_meshes : meshCap; // (more meshes than the caller's table holds: VGX_E_NOSPACE was set by the scan over the meshes, the scan here covers nothing)
	a.uv = ctx->asmCfg.uv; a.uv_bytes = ctx->asmCfg.uv ? ctx->asmCfg.uv_bytes : 0u; a.uv_value[0] = ctx->asmCfg.uv_value[0]; a.uv_value[1] = ctx->asmCfg.uv_value[1];
	vgx_launch_assemble(a, s);
	mark(ctx, s, "assemble");
	return VGX_OK;
}

// tableDone: the scan over the meshes already wrote the caller's mesh table
int runStrokeEmit(vgx_ctx* ctx, const vgx_draw* draws, const vgx_mesh_out* out, hipStream_t s, const float* poly = nullptr, bool tableDone = false)
{
	if (ctx->asmArmed) {
		const int st = runAssemble(ctx, out, s, draws);
		if (st != VGX_OK) { return st; }
	}
	VgxStrokeArgs a = strokeArgs(ctx, draws, poly, ctx->caps);
	a.mesh_base = ctx->asmArmed ? ctx->meshBase.ptr() : nullptr;
	a.pos = out->pos; a.color = out->color; a.idx = out->idx; a.meshes_out = tableDone ? nullptr : out->meshes;
	a.no_long = out->cap_vertices < ctx->opt.bigEmitMin ? 1 : 0; // frame-sized: one stroke kernel less to launch
	// Batches of fills and closed Miter AA / Thin strokes (the scan over the meshes decides, on the device): one draw-ordered tile
	// kernel instead of k_fill + k_stroke_simple (vgx_tile.hip). Not for frame-sized calls (two more launches than they are worth).
	uint64_t capTiles = 0;
	if (ctx->opt.tileEmit && ctx->route.tileHint && out->cap_vertices >= ctx->opt.bigEmitMin && out->cap_vertices / VGX_TILE_ELEMS + 2 < 0x7FFFFFFFull) {
		capTiles = out->cap_vertices / VGX_TILE_ELEMS + 2; // every element emits at least one vertex
		const int st = ensure(ctx, ctx->tileTab, capTiles);
		if (st != VGX_OK) { return st; }
		a.tile_mode = 1;
	}
	a.elem_prefix = a.elem_prefix_fill;
	vgx_launch_fill(a, vgxElementGrid(out->cap_vertices), s); // (tile mode: the mesh-table copy, and the kernel exits at once for the batches the tile kernel takes)
	mark(ctx, s, "fill_emit");
	a.elem_prefix = a.elem_prefix_stroke;
	vgx_launch_stroke(true, a, vgxElementGrid(out->cap_vertices), s);
	mark(ctx, s, "stroke_emit");
	if (a.tile_mode) {
		a.elem_prefix = nullptr;
		vgx_launch_emit_tiles(a, ctx->tileTab.ptr(), capTiles, s);
		mark(ctx, s, "tile_emit");
	}
	return launchStatus(ctx);
}

int ensureMeshBuffers(vgx_ctx* ctx, uint64_t polyVerts, uint64_t subpaths, uint64_t meshes)
{
	int st;
	if ((st = ensure(ctx, ctx->poly, (polyVerts + 1 + ctx->pieceVerts) * 2 * sizeof(float))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->subs, subpaths + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mdesc, meshes + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->elemPrefix, meshes + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->elemPrefixS, meshes + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mprep, meshes + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mtab, meshes + 1)) != VGX_OK) { return st; }
	ctx->caps.poly_vertices = ctx->poly.cap / (2 * sizeof(float)) - 1 - ctx->pieceVerts; // (the tail belongs to vgx_tessellate_dashed's pieces)
	ctx->caps.subpaths = ctx->subs.items() - 1;
	ctx->caps.meshes = minOf({ ctx->mdesc.items() - 1, ctx->elemPrefix.items() - 2, ctx->elemPrefixS.items() - 2, ctx->mprep.items() - 1, ctx->mtab.items() - 1 });
	return VGX_OK;
}

// per-command scratch of the flatten kernels for `ncmd` command instances (+ the leaf overflow area of k_flatten_build)
int ensureCmdScratch(vgx_ctx* ctx, uint64_t ncmd)
{
	int st;
	if ((st = ensure(ctx, ctx->cmdCnt, ncmd + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->subFirst, ncmd + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->leafOverflow, (size_t)VGX_BUILD_WAVES * VGX_BUILD_OVERFLOW * 64 * 2)) != VGX_OK) { return st; }
	ctx->caps.cmd_instances = minOf({ ctx->cmdCnt.items() - 1, ctx->subFirst.items() - 1 });
	return VGX_OK;
}

// look-back tables of the one-walk kernel for `segBound` segments: segment table, records (+ one group record per 64)
int ensureF1Tables(vgx_ctx* ctx, uint64_t segBound)
{
	const int st = ensure(ctx, ctx->f1SegDraw, segBound + 1);
	return st != VGX_OK ? st : ensure(ctx, ctx->f1Segs, segBound + segBound / 64 + 2);
}

// The context takes the route `r` (vgx_route_choose) for a batch of `ndraws` draws on `ps`: the tables it needs, then the state
int adoptRoute(vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws, const VgxRoute& r)
{
	int st;
	if (r.permute) {
		if ((st = ensure(ctx, ctx->instPerm, ndraws / r.period + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->instPermHist, (size_t)r.classes + 2)) != VGX_OK) { return st; }
	}
	if (r.kind == VGX_ROUTE_GROUPED && (st = ensureInstGroup(ctx, ps->dev.npaths, r.classes, ndraws, true)) != VGX_OK) { return st; }
	if (r.kind == VGX_ROUTE_ONE_WALK && (st = ensureF1Tables(ctx, r.f1SegBound)) != VGX_OK) { return st; }
	if (r.kind == VGX_ROUTE_ONE_WALK) { ctx->route.f1Ps = ps; ctx->route.f1PsGen = ps->gen; }
	ctx->route.chosen = r;
	return VGX_OK;
}

// what every route decision reads about the path set and the batch's size, on top of `known` (what is known of its content)
VgxRouteFacts routeFacts(VgxRouteFacts f, const vgx_pathset* ps, uint64_t ndraws)
{
	f.ndraws = ndraws; f.npaths = ps->dev.npaths; f.maxCmdsPerPath = ps->maxCmdsPerPath; f.thinStatic = ps->thinStatic;
	return f;
}

// A frame-sized batch (ndraws <= VGX_SMALL_DRAWS): five launches instead of seventeen (vgx_flatten.hip, "Frame-sized batches") --
// small_front -> flatten_build -> small_middle (which publishes its verdict to dev_sizes / dev_status) -> the emit kernels.
// markScratch: the scan over the draws flags a batch that outgrew the context's tables (vgx_tessellate_immediate).
int runFrameSized(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, int markScratch,
                  vgx_sizes* dev_sizes, uint32_t* dev_status, hipStream_t s)
{
	const VgxCaps outCaps = outCapsFor(ctx, out);
	const OpCmdPrefix opC = cmdPrefixOp(ctx, ps, draws, ndraws, ctx->caps.cmd_instances, 0);
	vgx_launch_small_front(&opC, ctx->dinfo.ptr(), s);
	mark(ctx, s, "small_front");
	VgxFlattenArgs f = flattenArgs(ctx, ps, draws, ndraws, 1);
	f.build_mode = 1;
	f.mprep = ctx->mprep.ptr();
	vgx_launch_flatten_build(f, ctx->opt.buildWaves, s, false);
	mark(ctx, s, "flatten_build");
	VgxStrokeArgs sa = strokeArgs(ctx, draws, nullptr, outCaps);
	sa.no_long = 1;
	OpDrawInfo opD;
	opD.dinfo = ctx->dinfo.ptr(); opD.ndraws = ndraws; opD.totals = ctx->totals.ptr(); opD.caps = ctx->caps; opD.keepPolyBase = 1; opD.markScratch = markScratch;
	OpMeshAll opM;
	opM.mdesc = ctx->mdesc.ptr(); opM.mtab = ctx->mtab.ptr(); opM.meshesOut = out->meshes;
	opM.prefixFill = ctx->elemPrefix.ptr(); opM.prefixStroke = ctx->elemPrefixS.ptr();
	opM.totals = ctx->totals.ptr(); opM.caps = outCaps; opM.checkCaps = 1; opM.fixedSize = 0; opM.fixedCount = 0;
	vgx_launch_small_middle(f, sa, &opD, &opM, dev_sizes, dev_status, s);
	mark(ctx, s, "small_middle");
	return runStrokeEmit(ctx, draws, out, s, nullptr, true);
}

} // namespace

extern "C" {

uint32_t vgx_version(void) { return VGX_VERSION; }

const char* vgx_status_string(int status)
{
	switch (status) {
	case VGX_OK: return "VGX_OK";
	case VGX_E_INVALID_ARG: return "VGX_E_INVALID_ARG";
	case VGX_E_INVALID_PATH: return "VGX_E_INVALID_PATH";
	case VGX_E_NONFINITE: return "VGX_E_NONFINITE";
	case VGX_E_NOSPACE: return "VGX_E_NOSPACE";
	case VGX_E_MESH_TOO_LARGE: return "VGX_E_MESH_TOO_LARGE";
	case VGX_E_HIP: return "VGX_E_HIP";
	case VGX_E_NO_DEVICE: return "VGX_E_NO_DEVICE";
	case VGX_E_RANGE: return "VGX_E_RANGE";
	case VGX_E_INTERNAL: return "VGX_E_INTERNAL";
	case VGX_E_STALE: return "VGX_E_STALE";
	case VGX_E_GROWN: return "VGX_E_GROWN";
	default: return "VGX_E_UNKNOWN";
	}
}

int vgx_create(int device, vgx_ctx** out_ctx)
{
	if (!out_ctx) {
		return VGX_E_INVALID_ARG;
	}
	*out_ctx = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
		return VGX_E_NO_DEVICE;
	}
	vgx_ctx* ctx = new (std::nothrow) vgx_ctx();
	if (!ctx) {
		return VGX_E_INVALID_ARG;
	}
	memset(ctx, 0, sizeof(*ctx));
	ctx->device = device;
	DeviceGuard guard(ctx); // the caller's current device is restored on return
	int cur = -1;
	if (hipGetDevice(&cur) != hipSuccess || cur != device) {
		delete ctx;
		return VGX_E_NO_DEVICE;
	}
	if (hipHostMalloc((void**)&ctx->hostTotals, sizeof(VgxTotals), hipHostMallocDefault) != hipSuccess) {
		delete ctx;
		return VGX_E_HIP;
	}
	ctx->opt = vgx_options_read(getenv); // tuning / testing knobs: read once here, never on the call path
	forgetRoutes(ctx);
	*out_ctx = ctx;
	return VGX_OK;
}

int vgx_destroy(vgx_ctx* ctx)
{
	if (!ctx) {
		return VGX_E_INVALID_ARG;
	}
	DeviceGuard guard(ctx);
	vgx_scratch_release(ctx->scratch);
	if (ctx->hostTotals) { (void)hipHostFree(ctx->hostTotals); }
	if (ctx->hostF1) { (void)hipHostFree(ctx->hostF1); }
	ctx->imm.mirror.release(); ctx->dash.release(); ctx->df.release(); ctx->ras.release(); ctx->rasDmg.release(); ctx->rasc.release(); ctx->rascDmg.release();
	if (ctx->hostPs) { (void)hipHostFree(ctx->hostPs); }
	if (ctx->psImage) { (void)hipHostFree(ctx->psImage); }
	for (int i = 0; i < VGX_PS_POOL; ++i) { if (ctx->psPool[i].p) { (void)hipFree(ctx->psPool[i].p); } }
	if (ctx->psStream) { (void)hipStreamDestroy(ctx->psStream); }
	vgx_rccl_release(ctx);
	if (ctx->evCreated) {
		for (int r = 0; r < VGX_PROF_RING; ++r) { for (int i = 0; i <= VGX_MAX_STAGES; ++i) { (void)hipEventDestroy(ctx->ev[r][i]); } }
	}
	delete ctx;
	return VGX_OK;
}

int vgx_last_hip_error(const vgx_ctx* ctx) { return ctx ? ctx->lastHipError : 0; }

uint64_t vgx_scratch_bytes(const vgx_ctx* ctx)
{
	if (!ctx) {
		return 0;
	}
	return vgx_scratch_bytes(ctx->scratch);
}

// ---- path set ---------------------------------------------------------------------------------------
// Host-side validation of the command grammar (see include/vgx.h) and derivation of the static
// per-command structure the kernels use (sub-path heads / tails, serial-path flag).
} // extern "C"

#include "vgx_pathset_host.h"

extern "C" {

int vgx_pathset_validate(const vgx_pathset_desc* desc)
{
	std::vector<uint8_t> cmdFlags, pathFlags;
	std::vector<uint32_t> spStart;
	uint32_t maxCmds = 0;
	return vgx_pathset_validate_host(desc, &cmdFlags, &spStart, &pathFlags, &maxCmds);
}

// The caller's arrays are ordinary host memory: hipMemcpyAsync moves them (the runtime pins pageable ranges in place for large
// copies: 22 GB/s cold, 55 GB/s for a range it has seen, profiles/micro/h2d_probe.hip).
static int psUpload(vgx_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s)
{
	if (bytes) { HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); }
	return VGX_OK;
}

struct VgxPsLayout
{
	size_t oArgs, oArgOff, oPathBegin, oType, rawEnd, oSpStart, oFlags, oPathFlags, oRec, oSubBegin, oSubLast, oThin, oThinPath, oThinSub, total;
};
// One blob: the four raw arrays first, back to back ([args (2 floats of padding in front: the start-point gather of command 0
// reads args[-2..-1])] [arg offsets] [path begins] [opcodes] -- a frame-sized set goes up as ONE image of this part), the derived
// tables behind them. The sub-path tables are sized for the most sub-paths `ncmd` commands can hold (every command ends one): what
// the set really has is known only after the scan, and 12 bytes per command of head room are nothing against 288 GB.
static VgxPsLayout psLayout(uint32_t ncmd, uint32_t npaths, uint32_t nargs)
{
	auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
	VgxPsLayout L;
	L.oArgs = 0;
	L.oArgOff = align(L.oArgs + ((size_t)nargs + 4) * sizeof(float));
	L.oPathBegin = align(L.oArgOff + ((size_t)ncmd + 1) * sizeof(uint32_t));
	L.oType = align(L.oPathBegin + ((size_t)npaths + 1) * sizeof(uint32_t));
	L.rawEnd = align(L.oType + ncmd + 1);
	L.oSpStart = L.rawEnd;
	L.oFlags = align(L.oSpStart + ((size_t)ncmd + 1) * sizeof(uint32_t));
	L.oPathFlags = align(L.oFlags + ncmd + 1);
	L.oRec = align(L.oPathFlags + npaths + 4);
	L.oSubBegin = align(L.oRec + ((size_t)ncmd + 1) * sizeof(VgxCmdRec));
	L.oSubLast = align(L.oSubBegin + ((size_t)npaths + 1) * sizeof(uint32_t));
	L.oThin = align(L.oSubLast + ((size_t)ncmd + 1) * sizeof(uint32_t));
	L.oThinPath = align(L.oThin + ((size_t)ncmd + 3) * sizeof(VgxCmdThin));
	L.oThinSub = align(L.oThinPath + ((size_t)npaths + 1) * sizeof(VgxThinPath));
	L.total = align(L.oThinSub + ((size_t)ncmd + 1) * sizeof(VgxThinSub));
	return L;
}

// Blobs of frame-sized sets are recycled through the context (hipFree synchronises the device; a renderer makes and drops one
// such set per frame): up to VGX_PS_POOL blobs of at most VGX_PS_POOL_MAX bytes wait here for the next vgx_pathset_create.
static void* psPoolTake(vgx_ctx* ctx, size_t need, size_t* got)
{
	int best = -1;
	for (int i = 0; i < VGX_PS_POOL; ++i) {
		if (ctx->psPool[i].p && ctx->psPool[i].cap >= need && (best < 0 || ctx->psPool[i].cap < ctx->psPool[best].cap)) { best = i; }
	}
	if (best < 0) { return nullptr; }
	void* p = ctx->psPool[best].p;
	*got = ctx->psPool[best].cap;
	ctx->psPool[best].p = nullptr; ctx->psPool[best].cap = 0;
	return p;
}
static bool psPoolGive(vgx_ctx* ctx, void* p, size_t cap)
{
	if (cap > VGX_PS_POOL_MAX) { return false; }
	for (int i = 0; i < VGX_PS_POOL; ++i) {
		if (!ctx->psPool[i].p) { ctx->psPool[i].p = p; ctx->psPool[i].cap = cap; return true; }
	}
	return false;
}

// Round 6: the raw arrays go up as they are and the derived tables are built by kernels (vgx_pathset.hip): grammar checks as a
// flagged reduction, sub-path heads / path of a command / sub-path ordinals by ONE scan over the commands, the 64-byte command
// records and the thin records by a lane per command, the static polyline layout of lineTo-only sets by a second scan. The host
// reads 32 bytes at the end. An invalid set takes the slow path: the host validator names the status.
int vgx_pathset_create(vgx_ctx* ctx, const vgx_pathset_desc* desc, vgx_pathset** out_ps)
{
	DeviceGuard guard(ctx);
	if (!ctx || !desc || !out_ps) {
		return VGX_E_INVALID_ARG;
	}
	*out_ps = nullptr;
	// the O(1) checks of the validator's head (vgx_pathset_host.h): everything the layout below depends on
	if (!desc->path_cmd_begin || !desc->cmd_arg_off || (desc->ncmd && !desc->cmd_type)) { return VGX_E_INVALID_ARG; }
	if (desc->path_cmd_begin[0] != 0 || desc->path_cmd_begin[desc->npaths] != desc->ncmd || desc->cmd_arg_off[0] != 0) { return VGX_E_INVALID_ARG; }
	if (desc->ncmd >= 0x7FFFFFFFu) { return VGX_E_INVALID_ARG; } // bit 31 of a command index carries a flag in the draw window
	const uint32_t ncmd = desc->ncmd, npaths = desc->npaths;
	const uint32_t nargs = desc->cmd_arg_off[ncmd];
	if (nargs && !desc->args) { return VGX_E_INVALID_ARG; }
	const VgxPsLayout L = psLayout(ncmd, npaths, nargs);
	int st;
	// temporaries of the build (grow-only context scratch): four words per command, the scans' partials, the totals
	auto a256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
	// layout: [totals (256 B) | pathAt] (cleared by ONE memset) | pathOf | lastSubEx | nvEx | partials
	const size_t words = a256(((size_t)ncmd + 1) * sizeof(uint32_t));
	const size_t tTot = 0, tW = 256, tPartA = tW + 4 * words, tPartB = tPartA + a256(VGX_MSCAN_BLOCKS * sizeof(VgxPsM)), tEnd = tPartB + a256(VGX_SCAN_BLOCKS * sizeof(Sum3));
	if ((st = ensure(ctx, ctx->psTemp, tEnd)) != VGX_OK) { return st; }
	if (!ctx->psStream) { HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->psStream, hipStreamNonBlocking)); }
	if (!ctx->hostPs) { HIPCHK(ctx, hipHostMalloc((void**)&ctx->hostPs, sizeof(VgxPsTotals), hipHostMallocDefault)); }
	hipStream_t s = ctx->psStream;

	vgx_pathset* ps = new (std::nothrow) vgx_pathset();
	if (!ps) {
		return VGX_E_INVALID_ARG;
	}
	const bool small = !ctx->opt.psNoSmall && vgx_pathset_is_small(ncmd, npaths, nargs);
	ps->blob = nullptr;
	ps->blobBytes = L.total;
	if (small) { ps->blob = psPoolTake(ctx, L.total, &ps->blobBytes); }
	hipError_t e = ps->blob ? hipSuccess : hipMalloc(&ps->blob, L.total);
	if (e != hipSuccess) {
		ctx->lastHipError = (int)e;
		delete ps;
		return VGX_E_HIP;
	}
	uint8_t* b = (uint8_t*)ps->blob;
	uint8_t* t = (uint8_t*)ctx->psTemp.p;
	auto fail = [&](int code) { (void)hipStreamSynchronize(s); (void)hipFree(ps->blob); delete ps; return code; };
	// totals and path marks start from zero (one memset: they are neighbours); what the passes OR into inside the blob and the padding
	// records the flatten kernels read past the ends are cleared by the first kernel -- no memset of the blob (1 GB for configs[3])
	e = hipMemsetAsync(t + tTot, 0, tW + words, s);
	if (e != hipSuccess) { ctx->lastHipError = (int)e; return fail(VGX_E_HIP); }
	bool maybeThin = true;
	if (small) {
		for (uint32_t c = 0; c < ncmd && maybeThin; ++c) { const uint8_t ty = desc->cmd_type[c]; maybeThin = ty == VGX_CMD_MOVE_TO || ty == VGX_CMD_LINE_TO || ty == VGX_CMD_CLOSE; }
		// ONE image of the raw part, filled in pinned memory, one copy
		if (L.rawEnd > ctx->psImageCap) {
			if (ctx->psImage) { (void)hipHostFree(ctx->psImage); ctx->psImage = nullptr; ctx->psImageCap = 0; }
			const size_t want = L.rawEnd * 2 > ((size_t)1 << 16) ? L.rawEnd * 2 : ((size_t)1 << 16);
			e = hipHostMalloc(&ctx->psImage, want, hipHostMallocDefault);
			if (e != hipSuccess) { ctx->lastHipError = (int)e; return fail(VGX_E_HIP); }
			ctx->psImageCap = want;
		}
		uint8_t* im = (uint8_t*)ctx->psImage;
		memset(im + L.oArgs, 0, 2 * sizeof(float));
		if (nargs) { memcpy(im + L.oArgs + 2 * sizeof(float), desc->args, (size_t)nargs * sizeof(float)); }
		memcpy(im + L.oArgOff, desc->cmd_arg_off, ((size_t)ncmd + 1) * sizeof(uint32_t));
		memcpy(im + L.oPathBegin, desc->path_cmd_begin, ((size_t)npaths + 1) * sizeof(uint32_t));
		if (ncmd) { memcpy(im + L.oType, desc->cmd_type, ncmd); }
		im[L.oType + ncmd] = 0;
		e = hipMemcpyAsync(b, im, L.rawEnd, hipMemcpyHostToDevice, s);
		if (e != hipSuccess) { ctx->lastHipError = (int)e; return fail(VGX_E_HIP); }
	} else {
		if ((st = psUpload(ctx, b + L.oArgs + 2 * sizeof(float), desc->args, (size_t)nargs * sizeof(float), s)) != VGX_OK) { return fail(st); }
		if ((st = psUpload(ctx, b + L.oArgOff, desc->cmd_arg_off, ((size_t)ncmd + 1) * sizeof(uint32_t), s)) != VGX_OK) { return fail(st); }
		if ((st = psUpload(ctx, b + L.oType, desc->cmd_type, ncmd, s)) != VGX_OK) { return fail(st); }
		if ((st = psUpload(ctx, b + L.oPathBegin, desc->path_cmd_begin, ((size_t)npaths + 1) * sizeof(uint32_t), s)) != VGX_OK) { return fail(st); }
	}
	VgxPsBuild B;
	B.type = b + L.oType; B.argOff = (const uint32_t*)(b + L.oArgOff); B.args = (const float*)(b + L.oArgs) + 2; B.pcb = (const uint32_t*)(b + L.oPathBegin);
	B.ncmd = ncmd; B.npaths = npaths; B.nargs = nargs;
	B.spStart = (uint32_t*)(b + L.oSpStart); B.flags = b + L.oFlags; B.pathFlags = b + L.oPathFlags; B.rec = (VgxCmdRec*)(b + L.oRec);
	B.thin = (VgxCmdThin*)(b + L.oThin) + 1; // thin[-1]: padding record
	B.subBegin = (uint32_t*)(b + L.oSubBegin); B.subLast = (uint32_t*)(b + L.oSubLast); B.tp = (VgxThinPath*)(b + L.oThinPath); B.ts = (VgxThinSub*)(b + L.oThinSub);
	B.pathAt = (uint32_t*)(t + tW); B.pathOf = (uint32_t*)(t + tW + words); B.lastSubEx = (uint32_t*)(t + tW + 2 * words); B.nvEx = (uint32_t*)(t + tW + 3 * words);
	B.partialA = (VgxPsM*)(t + tPartA); B.partialB = (Sum3*)(t + tPartB); B.tot = (VgxPsTotals*)(t + tTot);
	vgx_launch_pathset_build(B, maybeThin, s);
	e = hipGetLastError();
	if (e == hipSuccess) { e = hipMemcpyAsync(ctx->hostPs, B.tot, sizeof(VgxPsTotals), hipMemcpyDeviceToHost, s); }
	if (e == hipSuccess) { e = hipStreamSynchronize(s); }
	if (e != hipSuccess) { ctx->lastHipError = (int)e; return fail(VGX_E_HIP); }
	const VgxPsTotals T = *ctx->hostPs;
	if (T.err) {
		(void)hipFree(ps->blob);
		delete ps;
		const int vst = vgx_pathset_validate(desc); // the slow path of an invalid set: which status it is
		return vst != VGX_OK ? vst : VGX_E_INTERNAL;
	}
	ps->maxCmdsPerPath = T.maxCmds;
	ps->hasSerial = T.hasSerial != 0;
	ps->hasEmpty = T.hasEmpty != 0;
	ps->numSubs = T.nsubs;
	ps->thinStatic = npaths != 0 && ncmd != 0 && !T.notThin && !T.hasSerial && !T.hasEmpty && !T.thinIneligible;
	ps->dev.args = (const float*)(b + L.oArgs) + 2;
	ps->dev.cmd_arg_off = (const uint32_t*)(b + L.oArgOff);
	ps->dev.cmd_sp_start = (const uint32_t*)(b + L.oSpStart);
	ps->dev.path_cmd_begin = (const uint32_t*)(b + L.oPathBegin);
	ps->dev.cmd_type = b + L.oType;
	ps->dev.cmd_flags = b + L.oFlags;
	ps->dev.path_flags = b + L.oPathFlags;
	ps->dev.cmdrec = (const VgxCmdRec*)(b + L.oRec);
	ps->dev.cmdthin = (const VgxCmdThin*)(b + L.oThin) + 1;
	ps->dev.thin_path = (const VgxThinPath*)(b + L.oThinPath);
	ps->dev.thin_sub = (const VgxThinSub*)(b + L.oThinSub);
	ps->dev.path_sub_begin = (const uint32_t*)(b + L.oSubBegin);
	ps->dev.sub_last_cmd = (const uint32_t*)(b + L.oSubLast);
	ps->dev.npaths = npaths;
	ps->dev.ncmd = ncmd;
	static std::atomic<uint64_t> s_pathsetGen{0};
	ps->gen = ++s_pathsetGen;
	*out_ps = ps;
	return VGX_OK;
}

// Testing / inspection: copies one of the set's device tables to host memory (tests/test_gpu_pathset_build.py compares every table
// with the host restatement of csrc/vgx_pathset_host.h, byte for byte). `bytes` receives the table's size; dst may be NULL to ask.
int vgx_pathset_read_table(vgx_ctx* ctx, const vgx_pathset* ps, int which, void* dst, uint64_t cap_bytes, uint64_t* bytes)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || !bytes) { return VGX_E_INVALID_ARG; }
	const VgxPathSetDev& d = ps->dev;
	const void* src = nullptr; uint64_t n = 0;
	uint32_t scal[8] = { ps->maxCmdsPerPath, ps->hasSerial ? 1u : 0u, ps->hasEmpty ? 1u : 0u, ps->thinStatic ? 1u : 0u, ps->numSubs, d.npaths, d.ncmd, 0u };
	switch (which) {
	case VGX_PS_TABLE_CMD_FLAGS: src = d.cmd_flags; n = d.ncmd; break;
	case VGX_PS_TABLE_SP_START: src = d.cmd_sp_start; n = (uint64_t)d.ncmd * 4; break;
	case VGX_PS_TABLE_PATH_FLAGS: src = d.path_flags; n = d.npaths; break;
	case VGX_PS_TABLE_CMDREC: src = d.cmdrec; n = (uint64_t)d.ncmd * sizeof(VgxCmdRec); break;
	case VGX_PS_TABLE_PATH_SUB_BEGIN: src = d.path_sub_begin; n = ((uint64_t)d.npaths + 1) * 4; break;
	case VGX_PS_TABLE_SUB_LAST_CMD: src = d.sub_last_cmd; n = (uint64_t)ps->numSubs * 4; break;
	case VGX_PS_TABLE_CMDTHIN: src = d.cmdthin; n = (uint64_t)d.ncmd * sizeof(VgxCmdThin); break;
	case VGX_PS_TABLE_THIN_PATH: src = d.thin_path; n = ps->thinStatic ? (uint64_t)d.npaths * sizeof(VgxThinPath) : 0; break;
	case VGX_PS_TABLE_THIN_SUB: src = d.thin_sub; n = ps->thinStatic ? (uint64_t)ps->numSubs * sizeof(VgxThinSub) : 0; break;
	case VGX_PS_TABLE_SCALARS: n = sizeof(scal); break;
	default: return VGX_E_INVALID_ARG;
	}
	*bytes = n;
	if (!dst) { return VGX_OK; }
	if (cap_bytes < n) { return VGX_E_NOSPACE; }
	if (which == VGX_PS_TABLE_SCALARS) { memcpy(dst, scal, sizeof(scal)); return VGX_OK; }
	if (n) { HIPCHK(ctx, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost)); }
	return VGX_OK;
}

int vgx_pathset_destroy(vgx_ctx* ctx, vgx_pathset* ps)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps) {
		return VGX_E_INVALID_ARG;
	}
	if (ctx->counted.ps == ps) { ctx->counted.ps = nullptr; ctx->counted.stage = VGX_COUNTED_NONE; }
	if (ctx->tmpl.ps == ps) { tmplDrop(ctx); ctx->tmpl.ps = nullptr; ctx->tmpl.psGen = 0; } // a later path set at the same address must not match the template
	// hipFree waits for everything in flight (a caller may drop a set right behind an asynchronous call that reads it); a blob that
	// goes back to the pool instead must be as idle: the same wait, without the allocator's work
	if (ps->blob && ps->blobBytes <= VGX_PS_POOL_MAX) { (void)hipDeviceSynchronize(); }
	if (ps->blob && !psPoolGive(ctx, ps->blob, ps->blobBytes)) { (void)hipFree(ps->blob); }
	delete ps;
	return VGX_OK;
}

// ---- flatten ------------------------------------------------------------------------------------------
// facts: vgx_tessellate_count's -- look for reused paths (vgx_tessellate's instanced flatten) and report them; nullptr: a flatten-only entry
static int flattenCountBody(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, hipStream_t s, VgxRouteFacts* facts)
{
	int st;
	if ((st = ensureDrawBuffers(ctx, ndraws)) != VGX_OK) { return st; }
	forgetRoutes(ctx); // the scratch is re-sized for this batch; a template belongs to the count call that built it
	// pass 1: command instances (sizes the per-command scratch; not known yet: no bound)
	runCmdPrefix(ctx, ps, draws, ndraws, ~0ull, s);
	if (facts && ctx->opt.inst && ndraws > VGX_SMALL_DRAWS) {
		vgx_launch_inst_detect(draws, ndraws, ctx->totals.ptr(), s);
		// ... and how many different paths the draws use (grouped mode, when the sequence does not repeat)
		if ((st = ensureInstGroup(ctx, ps->dev.npaths, 1, ndraws, false)) != VGX_OK) { return st; }
		vgx_launch_inst_group(draws, ndraws, ps->dev.npaths, 1, ctx->instHist.ptr(), nullptr, nullptr, ctx->instStart.ptr(), ctx->instTaskStart.ptr(),
			nullptr, 0, nullptr, ctx->totals.ptr(), ctx->partial.p, s);
	}
	if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	if (facts) { // (without the detection pass the totals' words are zero: no period, no reuse)
		const VgxTotals& ht = *ctx->hostTotals;
		*facts = routeFacts(VgxRouteFacts(), ps, ndraws);
		facts->period = vgx_period_decode(ht.inst_detect_inv, ht.inst_detect_bad);
		facts->distinct = ht.inst_distinct;
		facts->tolKnown = true; facts->tolVariesPeriodic = ht.inst_tol_varies != 0; facts->tolVariesAny = (uint32_t)~ht.inst_tol_lo_inv != ht.inst_tol_hi;
	}
	if ((st = ensureCmdScratch(ctx, ctx->hostTotals->sizes.num_cmd_instances)) != VGX_OK) { return st; }
	// pass 2: per-draw counts (sizes polyline / sub-path / mesh scratch: no bound on those)
	VgxCaps sizing = ctx->caps;
	sizing.poly_vertices = ~0ull; sizing.subpaths = ~0ull; sizing.meshes = ~0ull;
	runFlattenCount(ctx, ps, draws, ndraws, sizing, s);
	if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	if (ctx->hostTotals->sizes.num_poly_vertices > 0xFFFFFFF0ull) { return VGX_E_RANGE; }
	return VGX_OK;
}

int vgx_flatten_count(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || (!draws && ndraws) || !out_sizes) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	const int st = flattenCountBody(ctx, ps, draws, ndraws, s, nullptr);
	if (st != VGX_OK) { return st; }
	*out_sizes = ctx->hostTotals->sizes;
	out_sizes->num_vertices = 0;
	out_sizes->num_indices = 0;
	ctx->counted = VgxCounted{ ps, draws, ndraws, VGX_COUNTED_FLATTEN };
	return VGX_OK;
}

int vgx_flatten_emit(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int apply_transform, const vgx_flat_out* out, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || !out || (!draws && ndraws)) {
		return VGX_E_INVALID_ARG;
	}
	if (!followsCount(ctx, VGX_COUNTED_FLATTEN, ps, draws, ndraws)) {
		return VGX_E_INVALID_ARG; // must follow vgx_flatten_count on the same batch (not vgx_tessellate_count: its polyline scratch is live)
	}
	const vgx_sizes& sz = ctx->hostTotals->sizes;
	if ((out->poly && out->cap_poly_vertices < sz.num_poly_vertices) || (out->subpaths && out->cap_subpaths < sz.num_subpaths)) {
		return VGX_E_NOSPACE;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	int st;
	// outputs the caller does not want still need somewhere to go
	if (!out->poly) { if ((st = ensure(ctx, ctx->poly, (sz.num_poly_vertices + 1) * 2 * sizeof(float))) != VGX_OK) { return st; } }
	if (!out->subpaths) { if ((st = ensure(ctx, ctx->subs, sz.num_subpaths + 1)) != VGX_OK) { return st; } }
	const VgxFlattenArgs a = flattenOutArgs(ctx, ps, draws, ndraws, apply_transform, out->poly ? out->poly : (float*)ctx->poly.p, out->subpaths ? out->subpaths : ctx->subs.ptr());
	vgx_launch_flatten(true, a, VGX_GRID_BLOCKS, s);
	mark(ctx, s, "flatten_emit");
	if (out->draw_info && ndraws) {
		HIPCHK(ctx, hipMemcpyAsync(out->draw_info, ctx->dinfo.p, ndraws * sizeof(vgx_draw_info), hipMemcpyDeviceToDevice, s));
	}
	return VGX_OK;
}

// ---- vgx_flatten: the ordered one-walk flatten (vgx_flat1.hip), asynchronous ---------------------------------------------
// What both routes of vgx_flatten end with: vertices and command instances to hostF1, for the next call's choice (never waited for; one-walk: the tag
// lands behind the two values -- the two-walk route runs on a tag that is known already), and the caller's copy of the per-draw records
static int flattenDone(vgx_ctx* ctx, uint64_t tag, bool withTag, const vgx_flat_out* out, uint64_t ndraws, hipStream_t s)
{
	if (ctx->hostF1) {
		VgxTotals* T = ctx->totals.ptr();
		ctx->f1Tag = tag;
		noteHip(ctx, hipMemcpyAsync(&ctx->hostF1[0], &T->sizes.num_poly_vertices, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		noteHip(ctx, hipMemcpyAsync(&ctx->hostF1[1], &T->sizes.num_cmd_instances, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		if (withTag) { noteHip(ctx, hipMemcpyAsync(&ctx->hostF1[2], &T->flat_tag, sizeof(unsigned long long), hipMemcpyDeviceToHost, s)); }
	}
	if (out->draw_info && ndraws) {
		HIPCHK(ctx, hipMemcpyAsync(out->draw_info, ctx->dinfo.p, ndraws * sizeof(vgx_draw_info), hipMemcpyDeviceToDevice, s));
	}
	return launchStatus(ctx);
}
int vgx_flatten(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int apply_transform, const vgx_flat_out* out,
                vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || !out || !out->poly || !out->subpaths || (!draws && ndraws)) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	tmplDrop(ctx);
	int st;
	if ((st = ensureDrawBuffers(ctx, ndraws)) != VGX_OK) { return st; }
	// The kernel instance and segment bucket (vgx_f1_shape) from the batch's leaves per command, taken from the LAST call on this context with
	// the same path set and draw count, when that call's result has arrived.
	const uint64_t tag = vgx_batch_tag(ps->gen, ndraws);
	if (!ctx->hostF1) {
		if (hipHostMalloc((void**)&ctx->hostF1, 4 * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess) { ctx->hostF1[0] = 0; ctx->hostF1[1] = 0; ctx->hostF1[2] = 0; ctx->hostF1[3] = 0; }
		else { ctx->hostF1 = nullptr; }
	}
	const bool known = ctx->hostF1 && ctx->f1Tag == tag && ctx->hostF1[1] != 0 && ctx->hostF1[2] == tag;
	int cap; uint32_t segMax;
	vgx_f1_shape(ctx->opt, known ? ctx->hostF1[0] : 0, known ? ctx->hostF1[1] : 0, &cap, &segMax);
	// Very short curves (a handful of segments per cubic: a chunk of 64 commands yields a few hundred vertices) are bound by what
	// a SEGMENT costs in the one-walk kernel -- its dependent loads and its place in the order, ~40 000 cycles whatever it holds --
	// not by the walk: the two-walk kernels (count -> scan over draws -> emit, vgx_flatten.hip) are faster there (1 M cubics of
	// ~5 segments: 0.43 against 0.63 ms), and they need no host round trip either once the batch's command total is known from
	// the last call. Same output.
	// The per-command words of the two walks are sized for ndraws x (longest path): what ANY draw list of this size can need on this path
	// set (the tag only says that the set and the number of draws are the last call's -- the draws' paths may have changed).
	// A set whose longest path is far above its mean (the bound above twice the last call's total) takes the one-walk route instead.
	const uint64_t cmdBoundAll = ndraws * (uint64_t)(ps->maxCmdsPerPath ? ps->maxCmdsPerPath : 1);
	if (known && !ctx->opt.f1Cap && !ctx->opt.f1Seg && !ps->hasEmpty
		&& (double)ctx->hostF1[0] / (double)ctx->hostF1[1] * 64.0 <= 384.0 && cmdBoundAll <= 2 * ctx->hostF1[1] + 4096) {
		if ((st = ensure(ctx, ctx->cmdCnt, cmdBoundAll + 1)) != VGX_OK) { return st; }
		// The device-side guard of THIS call only (a batch that grew: VGX_E_NOSPACE). The two-walk kernels write per-command words
		// only -- no sub-path records: cmdCnt alone bounds this launch. ctx->caps stays what vgx_tessellate relies on.
		runCmdPrefix(ctx, ps, draws, ndraws, ctx->cmdCnt.items() - 1, s);
		VgxCaps countCaps = ctx->caps; // the scan over the draws compares the totals with the caller's capacities
		countCaps.poly_vertices = out->cap_poly_vertices; countCaps.subpaths = out->cap_subpaths; countCaps.meshes = ~0ull;
		runFlattenCount(ctx, ps, draws, ndraws, countCaps, s);
		vgx_launch_flatten(true, flattenOutArgs(ctx, ps, draws, ndraws, apply_transform, out->poly, out->subpaths), VGX_GRID_BLOCKS, s);
		mark(ctx, s, "flatten_emit");
		publish(ctx, dev_sizes, dev_status, s);
		return flattenDone(ctx, tag, false, out, ndraws, s);
	}
	// Segments: buckets of at least min(32, segMax) command instances. The command total is not known on the host without a round
	// trip; ndraws x (longest path) bounds it (a batch whose bound is absurdly far above its real size asks once, synchronously).
	const uint64_t minItems = segMax < 32 ? segMax : 32;
	uint64_t cmdBound = cmdBoundAll;
	runCmdPrefix(ctx, ps, draws, ndraws, ~0ull, s); // k_flat1 needs no per-command scratch: no guard for this launch
	if (cmdBound / minItems > (1ull << 26)) {
		if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
		if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
		cmdBound = ctx->hostTotals->sizes.num_cmd_instances;
	}
	const uint64_t segBound = cmdBound / minItems + 2;
	if ((st = ensureF1Tables(ctx, segBound)) != VGX_OK) { return st; }
	VgxF1Args x;
	x.cap_poly = out->cap_poly_vertices; x.cap_subs = out->cap_subpaths; x.cap_meshes = ~0ull; x.seg_max = segMax; x.tag = tag;
	runOneWalk(ctx, ps, flattenOutArgs(ctx, ps, draws, ndraws, apply_transform, out->poly, out->subpaths), x, segBound, cap, dev_sizes, dev_status, s);
	return flattenDone(ctx, tag, true, out, ndraws, s);
}

// ---- partition (contiguous ranges per GPU, balanced on the count pass for heterogeneous batches) -------------
namespace {
// cut k of nparts: the first draw whose weight prefix reaches k / nparts of the total; `align` > 1 (the draws repeat a sequence of
// `align` paths: a drawing submitted for many instances): rounded to the nearest whole instance, so that every part stays a batch
// of whole instances (what the instanced / template paths of vgx_tessellate need)
__device__ __forceinline__ uint64_t partition_cut(const uint64_t* prefix, uint64_t ndraws, uint32_t nparts, uint32_t k, uint64_t align)
{
	if (k >= nparts) { return ndraws; }
	const uint64_t total = prefix[ndraws];
	const uint64_t target = (uint64_t)(((unsigned __int128)total * k) / nparts);
	uint64_t lo = 0, hi = ndraws;
	while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (prefix[mid] < target) { lo = mid + 1; } else { hi = mid; } }
	if (align > 1) { lo = (lo + align / 2) / align * align; if (lo > ndraws) { lo = ndraws; } }
	return lo;
}
__global__ void k_partition_bounds(const uint64_t* prefix, uint64_t ndraws, uint32_t nparts, uint64_t align, uint64_t* bounds, uint64_t* weights)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k > nparts) { return; }
	const uint64_t b = partition_cut(prefix, ndraws, nparts, k, align);
	bounds[k] = b;
	if (weights && k < nparts) { weights[k] = prefix[partition_cut(prefix, ndraws, nparts, k + 1, align)] - prefix[b]; }
}
}

int vgx_partition(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, uint32_t nparts, uint64_t* out_bounds, uint64_t* out_weights, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || (!draws && ndraws) || !out_bounds || nparts == 0 || nparts > 65536u) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	uint64_t align = 1;
	if (ctx->opt.inst && ndraws > VGX_SMALL_DRAWS) { // a drawing submitted for many instances? Then the cuts fall between instances
		if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
		noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
		vgx_launch_inst_detect(draws, ndraws, ctx->totals.ptr(), s);
		if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
		if (ctx->hostTotals->inst_detect_inv != 0 && !ctx->hostTotals->inst_detect_bad) {
			const unsigned long long P = ~0ull - ctx->hostTotals->inst_detect_inv;
			if (P > 1 && ndraws % P == 0 && ndraws / P >= nparts) { align = P; }
		}
	}
	st = flattenCountBody(ctx, ps, draws, ndraws, s, nullptr); // per-draw polyline vertex counts in dinfo
	if (st != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partBounds, ((size_t)nparts + 1) * 2 * sizeof(uint64_t))) != VGX_OK) { return st; }
	OpPartWeight op;
	op.draws = draws; op.dinfo = ctx->dinfo.ptr(); op.ndraws = ndraws; op.prefix = (uint64_t*)ctx->cmdPrefix.p; // the command prefix is not needed any more
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ndraws);
	uint64_t* dBounds = (uint64_t*)ctx->partBounds.p;
	uint64_t* dWeights = dBounds + nparts + 1;
	hipLaunchKernelGGL(k_partition_bounds, dim3((nparts + 1 + 255) / 256), dim3(256), 0, s, (const uint64_t*)ctx->cmdPrefix.p, ndraws, nparts, align, dBounds, dWeights);
	HIPCHK(ctx, hipMemcpyAsync(out_bounds, dBounds, ((size_t)nparts + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
	if (out_weights) { HIPCHK(ctx, hipMemcpyAsync(out_weights, dWeights, (size_t)nparts * sizeof(uint64_t), hipMemcpyDeviceToHost, s)); }
	HIPCHK(ctx, hipStreamSynchronize(s));
	return VGX_OK;
}

// ---- template mode (vgx_tmpl.hip) ---------------------------------------------------------------------
// One step in template mode: verify every draw against the saved first period, emit. No scratch besides the template.
// Round-join templates: the per-step tables (sized for this batch) and the kernels that fill them -- sizes of every Round-join mesh of
// every instance, places of meshes and instances, the batch totals in totals->sizes, VGX_E_NOSPACE against a.caps.
static int tmplRoundSizes(vgx_ctx* ctx, VgxTmplArgs& a, hipStream_t s)
{
	int st;
	const uint64_t n = a.ninst;
	a.num_round = ctx->tmpl.round; a.num_round_elems = ctx->tmpl.roundElems;
	a.trmesh = ctx->tmpl.trmesh.ptr(); a.tmsz = ctx->tmpl.tmsz.ptr();
	if (n * a.num_round >= (1ull << 31)) { return VGX_E_RANGE; } // one wave (long meshes: one workgroup) per (instance, Round-join mesh)
	const bool classes = a.cls != nullptr; // several classes: the tables' rows are the instances' own (VgxTmplInst::m / ::rel), the sizes stay in LDS
	if (!classes && (st = ensure(ctx, ctx->tmpl.rsz, (n * a.num_round + 1) * 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.relem, (classes ? ctx->tmpl.relemWords : n * a.num_round_elems) + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.mplace, (classes ? a.total.num_meshes : n * a.inst.num_meshes) + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	a.rsz = classes ? nullptr : ctx->tmpl.rsz.ptr(); a.relem = ctx->tmpl.relem.ptr();
	a.mplace = ctx->tmpl.mplace.ptr();
	if (vgx_tmpl_round_per_instance(a)) {
		if ((st = ensure(ctx, ctx->tmpl.itot, (n + 1) * 2)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->tmpl.iplace, (n + 1) * 2)) != VGX_OK) { return st; }
		a.itot = ctx->tmpl.itot.ptr(); a.iplace = ctx->tmpl.iplace.ptr();
	}
	vgx_launch_tmpl_round_sizes(a, (Sum3*)ctx->partial.p, s);
	mark(ctx, s, "tmpl_round_sizes");
	return VGX_OK;
}

// the step's arguments but the caller's buffers
static void tmplArgs(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, VgxTmplArgs& a)
{
	a.draws = draws; a.ndraws = ndraws; a.period = ctx->tmpl.period; a.ninst = ndraws / ctx->tmpl.period; a.npaths = ps->dev.npaths;
	a.tdraws = ctx->tmpl.draws.ptr(); a.tpoly = ctx->tmpl.poly.ptr(); a.tmesh = ctx->tmpl.mesh.ptr();
	a.tmtab = ctx->tmpl.mtab.ptr(); a.telem = ctx->tmpl.elem.ptr();
	a.inst = ctx->tmpl.inst;
	a.ttile = ctx->tmpl.tile.ptr();
	a.tile = ctx->tmpl.tileSize;
	a.tiles_per_inst = ctx->tmpl.tilesPerInst;
	a.caps = ctx->caps;
	a.totals = ctx->totals.ptr();
	a.kernel = ctx->tmpl.kernel;
	if (ctx->tmpl.classes > 1) {
		a.iinfo = ctx->tmpl.iinfo.ptr(); a.wg = ctx->tmpl.wg.ptr(); a.num_wg = ctx->tmpl.numWg;
		a.cls = ctx->tmpl.cls.ptr(); a.round_lds = ctx->tmpl.roundLds;
		a.total = ctx->tmpl.total;
	} else {
		memset(&a.total, 0, sizeof(a.total));
		vgx_tmpl_add_instances(a.total, a.ninst, ctx->tmpl.inst);
		a.num_wg = a.ninst * (uint64_t)a.tiles_per_inst;
	}
}

static int runTmpl(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, hipStream_t s)
{
	VgxTmplArgs a;
	memset(&a, 0, sizeof(a));
	tmplArgs(ctx, ps, draws, ndraws, a);
	a.pos = out->pos; a.color = out->color; a.idx = out->idx; a.meshes_out = out->meshes;
	a.caps.vertices = out->cap_vertices; a.caps.indices = out->cap_indices; a.caps.meshes = out->cap_meshes;
	if (a.num_wg > 0x7FFFFFFFull) { return VGX_E_RANGE; } // one workgroup per (instance, tile)
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	if (vgx_tmpl_kernel_is_round(a.kernel)) {
		// Round joins: vertices / indices are the instances' own -- counted on the device, checked against the capacities there
		a.total.num_vertices = 0; a.total.num_indices = 0;
		int st;
		if ((st = tmplRoundSizes(ctx, a, s)) != VGX_OK) { return st; }
	} else {
		// every size is known on the host: a batch that does not fit the caller's buffers ends here, with the need in dev_sizes
		const uint64_t nv = a.total.num_vertices, ni = a.total.num_indices, nm = a.total.num_meshes;
		const uint32_t aux = (nv > out->cap_vertices ? 1u : 0u) | (ni > out->cap_indices ? 2u : 0u) | ((out->meshes && nm > out->cap_meshes) ? 4u : 0u);
		if (aux) {
			const vgx_sizes z = a.total;
			hipLaunchKernelGGL(k_tmpl_nospace, dim3(1), dim3(1), 0, s, ctx->totals.ptr(), z, aux);
			publish(ctx, dev_sizes, dev_status, s);
			return launchStatus(ctx);
		}
	}
	if (ctx->asmArmed) {
		// draw-command assembly: the partition kernels need the whole batch's mesh table and every mesh's draw in memory
		const uint64_t nm = a.total.num_meshes;
		int st;
		if ((st = ensure(ctx, ctx->mtab, nm + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->mdesc, nm + 1)) != VGX_OK) { return st; }
		vgx_launch_tmpl_mtab(a, ctx->mtab.ptr(), ctx->mdesc.ptr(), s);
		mark(ctx, s, "tmpl_mesh_table");
		if ((st = runAssemble(ctx, out, s, draws)) != VGX_OK) { return st; }
		a.mesh_base = ctx->meshBase.ptr();
	}
	vgx_launch_tmpl_emit(a, s);
	mark(ctx, s, "tmpl_emit");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

static bool tmplFor(const vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws)
{
	return ctx->tmpl.on && ctx->opt.tmpl && ps == ctx->tmpl.ps && ps->gen == ctx->tmpl.psGen && ctx->tmpl.period && ndraws % ctx->tmpl.period == 0 && ndraws >= ctx->tmpl.period
		&& (ctx->tmpl.classes == 1 || ndraws == ctx->tmpl.nDraws); // several classes: the per-instance table belongs to ONE batch size
}

// The ordinary count + two-phase flatten in LOCAL space (apply_transform = 0) + mesh sizing of `n` draws: what a template is built
// from. Sizes and the mesh-kind flags end up in ctx->hostTotals.
static int tmplPipeline(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* d, uint64_t n, hipStream_t s)
{
	int st;
	if ((st = flattenCountBody(ctx, ps, d, n, s, nullptr)) != VGX_OK) { return st; }
	const vgx_sizes fsz = ctx->hostTotals->sizes;
	if ((st = ensureMeshBuffers(ctx, fsz.num_poly_vertices, fsz.num_subpaths, fsz.num_meshes)) != VGX_OK) { return st; }
	{
		VgxFlattenArgs a = flattenArgs(ctx, ps, d, n, 0);
		vgx_launch_flatten(true, a, VGX_GRID_BLOCKS, s);
	}
	runStrokeCount(ctx, d, sizingCaps(ctx), 0, s);
	if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	return VGX_OK;
}
// ---- the template build: vgx_tessellate_count, first thing ---------------------------------------------------------------------
// Do the draws repeat their first period in everything but transform and colours -- or a FEW flavours of it ("classes": every
// instance equals one of at most VGX_TMPL_MAX_CLASSES representatives, e.g. one drawing at a handful of scales) --, and are the
// meshes all of the kinds the emit kernels write? Then the representatives are flattened ONCE, in local space, by the ordinary
// two-phase kernels and kept as the context's template. A sequence of stages (tryTemplate); the host's decisions between the
// kernels are vgx_tmpl_plan.h's.
// What a stage reports: go on (VGX_OK), not a template -- the caller continues with the ordinary count --, or an error.
struct TmplStage
{
	int st;
	bool ordinary;
	TmplStage(int status) : st(status), ordinary(false) {}
	static TmplStage notATemplate() { TmplStage r(VGX_OK); r.ordinary = true; return r; }
	bool stop() const { return st != VGX_OK || ordinary; }
};
static const TmplStage TMPL_ORDINARY = TmplStage::notATemplate();

struct TmplJob // what the stages hand on
{
	vgx_ctx* ctx; const vgx_pathset* ps; const vgx_draw* draws; uint64_t ndraws; hipStream_t s;
	VgxTemplateState t;                    // the template's scalar part, committed to the context in one piece
	uint64_t P, ninst;                     // period, instances
	uint32_t T;                            // classes
	std::vector<uint32_t> instCls, reps;   // several classes: class of every instance, first instance of every class
	vgx_sizes all;                         // sizes of the concatenated representatives
	VgxTmplBuild b;
	std::vector<VgxTmplClass> cls;         // [T + 1] the class table, read back
	std::vector<vgx_sizes> csz;            // sizes of one instance of every class
	std::vector<uint64_t> clsRelems;       // Round-join elements of one instance of every class
	VgxTmplPlan plan;
};

// The period the draws repeat with (k_inst_detect, k_tmpl_check), or the whole draw list as one batch-wide instance
static TmplStage tmplDetectPeriod(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), j.s));
	vgx_launch_inst_detect(j.draws, j.ndraws, ctx->totals.ptr(), j.s);
	vgx_launch_tmpl_check(j.draws, j.ndraws, j.ps->dev.npaths, ctx->totals.ptr(), j.s);
	if ((st = readTotals(ctx, j.s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	unsigned long long P = (ctx->hostTotals->inst_detect_inv == 0 || ctx->hostTotals->inst_detect_bad) ? 0ull : ~0ull - ctx->hostTotals->inst_detect_inv;
	if (P == 0 || P > (1ull << 24) || j.ndraws % P != 0 || j.ndraws / P < VGX_INST_MIN_INSTANCES) {
		// no drawing repeated for many instances. A caller that keeps its batches' STRUCTURE from call to call (vgx_set_static_batches: the
		// same paths and styles in the same order, only transforms and colours move -- a static scene under a moving camera, a culled or
		// shuffled instanced scene) gets the whole draw list as ONE template of one instance: flattened once here, in local space; a step is
		// then the emit kernel alone, and any structural change ends it with VGX_E_STALE (the caller counts again)
		if (!ctx->opt.tmplBatch || j.ndraws >= (1ull << 31)) { return TMPL_ORDINARY; }
		P = j.ndraws;
		j.t.isBatch = true;
		ctx->hostTotals->tmpl_bad = 0;
	}
	j.P = P; j.ninst = j.ndraws / P;
	return VGX_OK;
}

// Not ONE period repeated: a few flavours of it? Candidates by hash of the template fields, then compared bit by bit.
static TmplStage tmplClassify(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint64_t ninst = j.ninst;
	j.T = 1; j.reps.assign(1, 0u);
	if (!ctx->hostTotals->tmpl_bad) { return VGX_OK; }
	if (!ctx->opt.tmplClasses || ninst > (1ull << 24)) { return TMPL_ORDINARY; } // (per-instance tables: 40 bytes per instance and tile on host and device)
	int st;
	if ((st = ensure(ctx, ctx->tmpl.hash, ninst)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->tmpl.hash.p, 0, ninst * sizeof(unsigned long long), j.s));
	vgx_launch_tmpl_hash(j.draws, j.ndraws, j.P, ctx->tmpl.hash.ptr(), j.s);
	std::vector<unsigned long long> hashes(ninst);
	HIPCHK(ctx, hipMemcpyAsync(hashes.data(), ctx->tmpl.hash.p, ninst * sizeof(unsigned long long), hipMemcpyDeviceToHost, j.s));
	HIPCHK(ctx, hipStreamSynchronize(j.s));
	if (!vgx_tmpl_group_classes(hashes.data(), ninst, j.instCls, j.reps)) { return TMPL_ORDINARY; } // too many flavours
	j.T = (uint32_t)j.reps.size();
	if ((st = ensure(ctx, ctx->tmpl.instCls, ninst)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.clsRep, (size_t)j.T)) != VGX_OK) { return st; }
	HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.instCls.p, j.instCls.data(), ninst * sizeof(uint32_t), hipMemcpyHostToDevice, j.s));
	HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.clsRep.p, j.reps.data(), (size_t)j.T * sizeof(uint32_t), hipMemcpyHostToDevice, j.s));
	noteHip(ctx, hipMemsetAsync(&ctx->totals.ptr()->tmpl_bad, 0, sizeof(uint32_t), j.s));
	vgx_launch_tmpl_check_cls(j.draws, j.ndraws, j.P, ctx->tmpl.instCls.ptr(), ctx->tmpl.clsRep.ptr(), ctx->totals.ptr(), j.s);
	if ((st = readTotals(ctx, j.s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->tmpl_bad) { return TMPL_ORDINARY; } // equal hashes, different records
	return VGX_OK;
}

// The class representatives' draw records, back to back (the saved records every step verifies the batch against), and all of
// them through the count pipeline as ONE batch: the template. (Several classes: NOT one pipeline per representative -- their sizes
// are differences of the prefixes the one concatenated run leaves behind, k_tmpl_class_sums; the Tiger at seven scales = 18
// classes: count 4.2 -> ~1 ms)
static TmplStage tmplRepresentatives(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint64_t P = j.P, PT = P * j.T;
	int st;
	if ((st = ensure(ctx, ctx->tmpl.draws, (size_t)PT)) != VGX_OK) { return st; }
	for (uint32_t c = 0; c < j.T; ++c) {
		HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.draws.ptr() + (uint64_t)c * P, j.draws + (uint64_t)j.reps[c] * P, (size_t)P * sizeof(vgx_draw), hipMemcpyDeviceToDevice, j.s));
	}
	j.csz.assign(j.T, vgx_sizes());
	if ((st = tmplPipeline(ctx, j.ps, ctx->tmpl.draws.ptr(), PT, j.s)) != VGX_OK) { return st; }
	const VgxTotals& ht = *ctx->hostTotals;
	if (j.T == 1) {
		if (!vgx_tmpl_eligible(ht, ctx->opt.tmplRound != 0)) { return TMPL_ORDINARY; }
		j.csz[0] = ht.sizes;
	} else if ((ht.num_round_meshes && !ctx->opt.tmplRound) || ht.sizes.num_poly_vertices >= (1ull << 32) || ht.sizes.num_meshes >= (1ull << 32) || ht.sizes.num_elements >= (1ull << 36)) {
		return TMPL_ORDINARY; // (the limits of one instance: per class, tmplBuildTables)
	}
	j.all = ht.sizes;
	return VGX_OK;
}

// Which stroke styles does the template hold (k_tmpl_styles)? They decide the emit kernel and, with it, the tile size. Leaves the
// class table zeroed but for the style word.
static TmplStage tmplChooseKernel(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint32_t T = j.T;
	const bool general = ctx->hostTotals->has_general_stroke != 0;
	int st;
	if ((st = ensure(ctx, ctx->tmpl.cls, (size_t)T + 1)) != VGX_OK) { return st; }
	memset(&j.b, 0, sizeof(j.b));
	uint32_t styles = 0;
	noteHip(ctx, hipMemsetAsync(ctx->tmpl.cls.p, 0, ((size_t)T + 1) * sizeof(VgxTmplClass), j.s));
	if (general) {
		j.b.mdesc = ctx->mdesc.ptr(); j.b.num_meshes = j.all.num_meshes; j.b.nclasses = T; j.b.cls = ctx->tmpl.cls.ptr();
		vgx_launch_tmpl_styles(j.b, j.s);
		HIPCHK(ctx, hipMemcpyAsync(&styles, &VGX_TMPL_STYLES(ctx->tmpl.cls.ptr(), T), sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
		HIPCHK(ctx, hipStreamSynchronize(j.s));
	}
	j.t.kernel = vgx_tmpl_kernel_for(styles);
	// (Round joins in a template of several classes: the per-step tables are addressed per instance -- VgxTmplInst::m / ::rel --, the sizes
	// pass runs in its workgroup-per-instance shape; a batch that does not fit that shape takes the ordinary pipeline, tmplFirstRoundSizes)
	j.t.tileSize = vgx_tmpl_tile_for(j.t.kernel, ctx->opt.tmplTile);
	return VGX_OK;
}

// The class table (k_tmpl_classes) and the sizes of one instance of every class; then the template's tables (vgx_launch_tmpl_build)
static TmplStage tmplBuildTables(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint32_t T = j.T;
	const uint64_t M = j.all.num_meshes, V = j.all.num_poly_vertices;
	VgxTmplBuild& b = j.b;
	int st;
	b.draws = ctx->tmpl.draws.ptr(); b.poly = (const float2*)ctx->poly.p; b.mdesc = ctx->mdesc.ptr(); b.mprep = ctx->mprep.ptr(); b.mtab = ctx->mtab.ptr();
	b.prefix_fill = ctx->elemPrefix.ptr(); b.prefix_stroke = ctx->elemPrefixS.ptr();
	b.num_meshes = M; b.num_elems = j.all.num_elements; b.tile = j.t.tileSize; b.period = (uint32_t)j.P; b.nclasses = T;
	b.num_vertices = j.all.num_vertices; b.num_indices = j.all.num_indices; b.cls = ctx->tmpl.cls.ptr();
	if ((st = ensure(ctx, ctx->tmpl.clsLmax, (size_t)T + 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->tmpl.clsLmax.p, 0, ((size_t)T + 1) * sizeof(uint32_t), j.s));
	b.lmax = ctx->tmpl.clsLmax.ptr();
	if ((st = ensure(ctx, ctx->tmpl.tbound, (size_t)vgx_tmpl_max_tiles(j.all.num_elements, j.t.tileSize, T) + 1)) != VGX_OK) { return st; }
	b.tbound = ctx->tmpl.tbound.ptr();
	vgx_launch_tmpl_classes(b, j.s);
	j.cls.resize((size_t)T + 1);
	std::vector<unsigned long long> csum(((size_t)T + 1) * 5, 0ull);
	if (T > 1) {
		if ((st = ensure(ctx, ctx->tmpl.clsSum, ((size_t)T + 1) * 5)) != VGX_OK) { return st; }
		vgx_launch_tmpl_class_sums(b, ctx->dinfo.ptr(), (const uint64_t*)ctx->cmdPrefix.p, j.P * T, j.all, ctx->tmpl.clsSum.ptr(), j.s);
		HIPCHK(ctx, hipMemcpyAsync(csum.data(), ctx->tmpl.clsSum.p, csum.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, j.s));
	}
	HIPCHK(ctx, hipMemcpyAsync(j.cls.data(), ctx->tmpl.cls.p, ((size_t)T + 1) * sizeof(VgxTmplClass), hipMemcpyDeviceToHost, j.s));
	HIPCHK(ctx, hipStreamSynchronize(j.s));
	if (T > 1 && !vgx_tmpl_class_sizes(j.cls.data(), csum.data(), T, j.csz)) { return TMPL_ORDINARY; }
	const uint64_t tiles = j.cls[T].tile0;
	j.t.tilesPerInst = j.cls[1].tile0; // (one class: the grid of a step)
	if ((st = ensure(ctx, ctx->tmpl.poly, V + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.mesh, M + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.mtab, M + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.elem, tiles * j.t.tileSize + 64)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.tile, tiles + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.trmesh, M + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->tmpl.tmsz, M + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	b.tmsz = ctx->tmpl.tmsz.ptr(); b.trmesh = ctx->tmpl.trmesh.ptr();
	b.has_round = vgx_tmpl_kernel_is_round(j.t.kernel) ? 1u : 0u;
	b.partial = (Sum3*)ctx->partial.p;
	b.ttile = ctx->tmpl.tile.ptr();
	b.tmesh = ctx->tmpl.mesh.ptr(); b.tmtab = ctx->tmpl.mtab.ptr(); b.telem = ctx->tmpl.elem.ptr();
	vgx_launch_tmpl_build(b, j.s);
	HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.poly.p, ctx->poly.p, V * 2 * sizeof(float), hipMemcpyDeviceToDevice, j.s));
	return VGX_OK;
}

// Round joins: how many such meshes the template holds and their elements; several classes: where each class's begin (k_tmpl_round_classes)
static TmplStage tmplReadRoundLayout(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint32_t T = j.T;
	j.clsRelems.assign(T, 0);
	if (!vgx_tmpl_kernel_is_round(j.t.kernel)) { return VGX_OK; }
	HIPCHK(ctx, hipMemcpyAsync(j.cls.data(), ctx->tmpl.cls.p, ((size_t)T + 1) * sizeof(VgxTmplClass), hipMemcpyDeviceToHost, j.s));
	HIPCHK(ctx, hipStreamSynchronize(j.s));
	j.t.round = j.cls[T].round[VGX_TC_MESH0];
	if (j.t.round == 0) { return TMPL_ORDINARY; }
	VgxTmplRoundMesh last;
	HIPCHK(ctx, hipMemcpyAsync(&last, ctx->tmpl.trmesh.ptr() + j.t.round, sizeof(last), hipMemcpyDeviceToHost, j.s));
	HIPCHK(ctx, hipStreamSynchronize(j.s));
	j.t.roundElems = last.elem0;
	vgx_tmpl_round_layout(j.cls.data(), T, j.t.round, j.t.roundElems, j.clsRelems, j.t.roundLds);
	return VGX_OK;
}

// The batch: instances x their class's sizes; several classes: the per-instance and per-workgroup tables, uploaded
static TmplStage tmplPlanBatch(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	const uint64_t ninst = j.ninst;
	VgxTmplPlan& p = j.plan;
	int st;
	if (!vgx_tmpl_plan_batch(j.csz.data(), j.cls.data(), j.T, ninst, j.instCls.data(), vgx_tmpl_kernel_is_round(j.t.kernel) ? j.clsRelems.data() : nullptr, p)) { return TMPL_ORDINARY; }
	if (j.T > 1) {
		if ((st = ensure(ctx, ctx->tmpl.iinfo, ninst + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->tmpl.wg, (size_t)p.numWg + 1)) != VGX_OK) { return st; }
		HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.iinfo.p, p.inst.data(), (ninst + 1) * sizeof(VgxTmplInst), hipMemcpyHostToDevice, j.s));
		HIPCHK(ctx, hipMemcpyAsync(ctx->tmpl.wg.p, p.wg.data(), (size_t)p.numWg * sizeof(VgxTmplWg), hipMemcpyHostToDevice, j.s));
		HIPCHK(ctx, hipStreamSynchronize(j.s)); // the copies have read the host tables
	}
	HIPCHK(ctx, hipStreamSynchronize(j.s));
	if ((st = launchStatus(ctx)) != VGX_OK) { return st; }
	j.t.ps = j.ps; j.t.psGen = j.ps->gen; j.t.period = (uint32_t)j.P; j.t.classes = j.T; j.t.nDraws = j.ndraws;
	j.t.inst = j.csz[0]; j.t.total = p.total; j.t.numWg = p.numWg; j.t.relemWords = p.relemWords;
	return VGX_OK;
}

// Round joins: this batch's vertices / indices -- the count of one step (through the committed template, tmplArgs), read back
static TmplStage tmplFirstRoundSizes(TmplJob& j)
{
	vgx_ctx* ctx = j.ctx;
	int st;
	VgxTmplArgs a;
	memset(&a, 0, sizeof(a));
	tmplArgs(ctx, j.ps, j.draws, j.ndraws, a);
	a.caps.vertices = ~0ull; a.caps.indices = ~0ull; a.caps.meshes = ~0ull;
	a.total.num_vertices = 0; a.total.num_indices = 0;
	if (a.num_wg > 0x7FFFFFFFull || a.ninst * (uint64_t)j.t.round >= (1ull << 31)) { return TMPL_ORDINARY; } // beyond the sizes kernels' grids
	if (j.T > 1) { // several classes: only the workgroup-per-instance shape of the sizes pass addresses its tables per instance
		a.num_round = j.t.round; a.num_round_elems = j.t.roundElems;
		if (!vgx_tmpl_round_per_instance(a) || ctx->tmpl.relemWords >= (1ull << 40)) { return TMPL_ORDINARY; }
	}
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), j.s));
	if ((st = tmplRoundSizes(ctx, a, j.s)) != VGX_OK) { return st; }
	if ((st = readTotals(ctx, j.s)) != VGX_OK) { return st; }
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	ctx->tmpl.total = ctx->hostTotals->sizes;
	return VGX_OK;
}

// Returns VGX_OK with ctx->tmpl.on set (out_sizes filled), VGX_OK with it clear (not such a batch: the caller continues with the
// ordinary count), or an error.
static int tryTemplate(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, hipStream_t s)
{
	tmplDrop(ctx);
	if (!ctx->opt.tmpl || !ctx->opt.inst || (ndraws <= VGX_SMALL_DRAWS && !ctx->opt.tmplBatch) || ndraws == 0) { return VGX_OK; } // (static batches: frame-sized draw lists too)
	TmplJob j;
	j.ctx = ctx; j.ps = ps; j.draws = draws; j.ndraws = ndraws; j.s = s;
	memset(&j.t, 0, sizeof(j.t));
	TmplStage (*const build[])(TmplJob&) = { tmplDetectPeriod, tmplClassify, tmplRepresentatives, tmplChooseKernel, tmplBuildTables, tmplReadRoundLayout, tmplPlanBatch };
	for (auto stage : build) {
		const TmplStage r = stage(j);
		if (r.stop()) { return r.st; }
	}
	static_cast<VgxTemplateState&>(ctx->tmpl) = j.t; // the commit (`on` still clear)
	if (vgx_tmpl_kernel_is_round(j.t.kernel)) {
		const TmplStage r = tmplFirstRoundSizes(j);
		if (r.stop()) { return r.st; }
	}
	ctx->tmpl.on = true;
	*out_sizes = ctx->tmpl.total;
	ctx->hostTotals->sizes = ctx->tmpl.total; // what vgx_tessellate_emit checks the caller's capacities against
	return VGX_OK;
}

// ---- tessellate ---------------------------------------------------------------------------------------
int vgx_tessellate_count(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || (!draws && ndraws) || !out_sizes) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st = tryTemplate(ctx, ps, draws, ndraws, out_sizes, s);
	if (st != VGX_OK) { return st; }
	if (ctx->tmpl.on) {
		ctx->counted = VgxCounted{ ps, draws, ndraws, VGX_COUNTED_TESSELLATE };
		return VGX_OK;
	}
	VgxRouteFacts facts;
	if ((st = flattenCountBody(ctx, ps, draws, ndraws, s, &facts)) != VGX_OK) { return st; }
	// the sizes are known too: the route, its heap, its tables (one-walk: beyond frame size only, tables for whatever the draw buffers hold)
	const vgx_sizes sz = ctx->hostTotals->sizes;
	facts.sizesKnown = true; facts.V = sz.num_poly_vertices; facts.ncmd = sz.num_cmd_instances;
	facts.longKnown = true; facts.longV = ctx->hostTotals->long_subpath_vertices; facts.instLongV = ctx->hostTotals->inst_long_subpath_vertices;
	facts.f1Draws = ndraws <= VGX_SMALL_DRAWS ? 0 : (ctx->route.capDraws > ndraws ? ctx->route.capDraws : ndraws);
	const VgxRoute route = vgx_route_choose(facts, ctx->opt, VGX_NO_HEAP_LIMIT);
	if ((st = ensureMeshBuffers(ctx, route.heapVerts, sz.num_subpaths, sz.num_meshes)) != VGX_OK) { return st; }
	if ((st = adoptRoute(ctx, ps, ndraws, route)) != VGX_OK) { return st; }
	VgxFlattenArgs a = flattenArgs(ctx, ps, draws, ndraws, 1);
	vgx_launch_flatten(true, a, VGX_GRID_BLOCKS, s);
	mark(ctx, s, "flatten_emit");
	runStrokeCount(ctx, draws, sizingCaps(ctx), 0, s);
	if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
	*out_sizes = ctx->hostTotals->sizes;
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; } // _emit must not follow a failed count
	ctx->counted = VgxCounted{ ps, draws, ndraws, VGX_COUNTED_TESSELLATE };
	// what the scan over the counted meshes found: a batch with open / Bevel / Round / non-AA strokes is k_fill's and k_stroke's, and the
	// calls that follow a count like that do not launch the tile kernel at all (its 200 000 workgroups would only find that out again)
	ctx->route.tileHint = ctx->hostTotals->has_general_stroke == 0u;
	return VGX_OK;
}

int vgx_tessellate_emit(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || !out || (!draws && ndraws) || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)) {
		return VGX_E_INVALID_ARG;
	}
	if (!followsCount(ctx, VGX_COUNTED_TESSELLATE, ps, draws, ndraws)) {
		return VGX_E_INVALID_ARG; // must follow vgx_tessellate_count on the same batch
	}
	const vgx_sizes& sz = ctx->hostTotals->sizes;
	if (out->cap_vertices < sz.num_vertices || out->cap_indices < sz.num_indices || (out->meshes && out->cap_meshes < sz.num_meshes)) {
		return VGX_E_NOSPACE;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	if (tmplFor(ctx, ps, ndraws)) { return runTmpl(ctx, ps, draws, ndraws, out, nullptr, nullptr, s); }
	return runStrokeEmit(ctx, draws, out, s);
}

int vgx_tessellate(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !ps || !out || (!draws && ndraws) || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)) {
		return VGX_E_INVALID_ARG;
	}
	if (tmplFor(ctx, ps, ndraws)) {
		hipStream_t s = (hipStream_t)stream;
		markBegin(ctx, s);
		ctx->counted.stage = VGX_COUNTED_NONE;
		return runTmpl(ctx, ps, draws, ndraws, out, dev_sizes, dev_status, s);
	}
	if (ndraws > ctx->route.capDraws || !ctx->cmdCnt.p || !ctx->subFirst.p || !ctx->poly.p || !ctx->mtab.p) {
		return VGX_E_NOSPACE; // scratch was never sized for a batch like this: run vgx_tessellate_count once
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	if (ndraws <= VGX_SMALL_DRAWS && !ctx->opt.noSmall) { // (round 6: also with draw-command assembly armed -- runStrokeEmit runs the partition kernels in front of the emit either way)
		const int est = runFrameSized(ctx, ps, draws, ndraws, out, 0, dev_sizes, dev_status, s);
		if (est != VGX_OK) { return est; }
		if (ctx->asmArmed) { publish(ctx, dev_sizes, dev_status, s); } // the partition kernels may have ended the call (a mesh beyond any vertex buffer, the command table full): the verdict once more
		return launchStatus(ctx);
	}
	runFlattenStage(ctx, ps, draws, ndraws, s);
	runStrokeCount(ctx, draws, outCapsFor(ctx, out), 1, s, nullptr, true, out->meshes);
	{
		const int st = runStrokeEmit(ctx, draws, out, s, nullptr, true);
		if (st != VGX_OK) { return st; }
	}
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

// ---- immediate mode: vgx_tessellate_immediate / vgx_reserve -------------------------------------------------------------
// The mirror of the last immediate call, if its copy has landed (never waited for): what the batch was, and after VGX_E_GROWN the scratch it
// needs -- grown here, the instanced flatten's heap included when its draws reuse paths
static int immConsume(vgx_ctx* ctx, const vgx_pathset* ps)
{
	VgxImmState& im = ctx->imm;
	if (!im.mirror.landed()) { return VGX_OK; }
	const VgxTotals& h = *im.mirror.host;
	if (h.status != VGX_OK && h.status != VGX_E_NOSPACE && h.status != VGX_E_GROWN) { return VGX_OK; } // (no totals to learn from)
	const bool same = im.known && im.tag == im.pendTag;
	VgxRouteFacts& f = im.facts;
	if (im.pendDetect || !same) { // (else: the period and the paths of the batch are what an earlier call found)
		f.period = im.pendDetect ? vgx_period_decode(h.inst_detect_inv, h.inst_detect_bad) : 0;
		f.distinct = im.pendDetect ? h.inst_distinct : 0;
	}
	im.known = true; im.tag = im.pendTag;
	f.ndraws = im.pendNDraws; f.thinStatic = ps->thinStatic;
	f.sizesKnown = true; f.V = h.sizes.num_poly_vertices; f.ncmd = h.sizes.num_cmd_instances;
	if (h.status != VGX_E_GROWN || !h.scratch_short) { // (VGX_E_GROWN without the flag: vgx_tessellate_dashed's pieces outgrew their scratch, the flatten stage fitted)
		if (!same) { f.longKnown = false; }
		return VGX_OK;
	}
	f.longV = h.imm_long_subpath_vertices; f.instLongV = h.imm_inst_long_subpath_vertices; f.longKnown = true;
	if (h.sizes.num_poly_vertices > 0xFFFFFFF0ull) { return VGX_OK; } // (VGX_E_RANGE territory: nothing sensible to grow to)
	int st;
	if ((st = ensureCmdScratch(ctx, h.sizes.num_cmd_instances)) != VGX_OK) { return st; }
	return ensureMeshBuffers(ctx, vgx_route_heap_verts(f, ctx->opt), h.sizes.num_subpaths, h.sizes.num_meshes);
}

// What vgx_tessellate_immediate and vgx_tessellate_dashed begin with: counted state ends (the _emit pairing, the template, the chosen routes); the last
// call's need, when it has reached the mirror; the tables every route needs (a fresh context gets small ones and learns the need from VGX_E_GROWN)
static int immBegin(vgx_ctx* ctx, const vgx_pathset* ps, uint64_t ndraws)
{
	int st;
	if ((st = ctx->imm.mirror.create(ctx, 1)) != VGX_OK) { return st; }
	ctx->counted.stage = VGX_COUNTED_NONE;
	forgetRoutes(ctx);
	if ((st = immConsume(ctx, ps)) != VGX_OK) { return st; }
	if ((st = ensureDrawBuffers(ctx, ndraws)) != VGX_OK) { return st; }
	return ensureCmdScratch(ctx, 4096);
}

int vgx_reserve(vgx_ctx* ctx, uint64_t ndraws, const vgx_sizes* totals)
{
	if (!ctx || !totals) { // (before the context is touched)
		return VGX_E_INVALID_ARG;
	}
	DeviceGuard guard(ctx);
	if (totals->num_poly_vertices > 0xFFFFFFF0ull || totals->num_cmd_instances > 0xFFFFFFF0ull) { return VGX_E_RANGE; }
	int st;
	if ((st = ctx->imm.mirror.create(ctx, 1)) != VGX_OK) { return st; }
	if ((st = ensureDrawBuffers(ctx, ndraws)) != VGX_OK) { return st; }
	if ((st = ensureCmdScratch(ctx, totals->num_cmd_instances)) != VGX_OK) { return st; }
	// the long sub-paths are not known: every vertex counted as one of them (the heap then holds any batch within these totals)
	const uint64_t V = totals->num_poly_vertices;
	return ensureMeshBuffers(ctx, vgx_heap_build_verts(true, V, totals->num_cmd_instances, V), totals->num_subpaths, totals->num_meshes);
}

int vgx_tessellate_immediate(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out,
                             vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	if (!ctx || !ps || !out || (!draws && ndraws) || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)) { // (before the context is touched)
		return VGX_E_INVALID_ARG;
	}
	DeviceGuard guard(ctx);
	hipStream_t s = (hipStream_t)stream;
	int st;
	if ((st = immBegin(ctx, ps, ndraws)) != VGX_OK) { return st; }
	if ((st = ensureMeshBuffers(ctx, 4096, 1024, 1024)) != VGX_OK) { return st; }
	markBegin(ctx, s);
	const uint64_t tag = vgx_batch_tag(ps->gen, ndraws);
	const bool known = ctx->imm.known && ctx->imm.tag == tag;
	VgxTotals* T = ctx->totals.ptr();
	bool detect = false;
	// The route by vgx_tessellate_count's rules, from what the last immediate call on this batch found (a batch not seen before: only its size)
	VgxRouteFacts f = routeFacts(known ? ctx->imm.facts : VgxRouteFacts(), ps, ndraws);
	f.f1Draws = known ? ndraws : 0; f.oneBatch = true;
	const VgxRoute route = vgx_route_choose(f, ctx->opt, ctx->caps.poly_vertices);
	if (route.kind == VGX_ROUTE_FRAME) {
		// frame-sized: vgx_tessellate's five launches; the scan over the draws flags a batch that outgrew the context's tables
		mark(ctx, s, "route_frame"); // (a stage of no length: which route the call took, for the profile)
		if ((st = runFrameSized(ctx, ps, draws, ndraws, out, 1, nullptr, nullptr, s)) != VGX_OK) { return st; }
		vgx_launch_imm_size(ps->dev, draws, ndraws, T, 0, true, dev_sizes, dev_status, s); // (+ the verdict)
		mark(ctx, s, "imm_size");
	} else {
		if ((st = adoptRoute(ctx, ps, ndraws, route)) != VGX_OK) { return st; }
		mark(ctx, s, route.kind == VGX_ROUTE_PERIODIC ? "route_periodic" : (route.kind == VGX_ROUTE_GROUPED ? "route_grouped" : (route.kind == VGX_ROUTE_ONE_WALK ? "route_one_walk" : "route_build"))); // (no length)
		runFlattenStage(ctx, ps, draws, ndraws, s);
		if (route.kind == VGX_ROUTE_ONE_WALK) { ctx->route.chosen.kind = VGX_ROUTE_BUILD; } // (this call's alone: only a count leaves a one-walk route for vgx_tessellate)
		detect = !known && ctx->opt.inst; // the period of the paths and how many of them the draws use, for the next call on this batch
		if (detect) {
			vgx_launch_inst_detect(draws, ndraws, T, s);
			if ((st = ensureInstGroup(ctx, ps->dev.npaths, 1, ndraws, false)) != VGX_OK) { return st; }
			vgx_launch_inst_group(draws, ndraws, ps->dev.npaths, 1, ctx->instHist.ptr(), nullptr, nullptr, ctx->instStart.ptr(), ctx->instTaskStart.ptr(),
				nullptr, 0, nullptr, T, ctx->partial.p, s);
		}
		// the flatten stage checks the context's tables only: a VGX_E_NOSPACE here is the scratch's
		vgx_launch_imm_size(ps->dev, draws, ndraws, T, 1, false, nullptr, nullptr, s);
		mark(ctx, s, "imm_size");
		runStrokeCount(ctx, draws, outCapsFor(ctx, out), 1, s, nullptr, true, out->meshes);
		if ((st = runStrokeEmit(ctx, draws, out, s, nullptr, true)) != VGX_OK) { return st; }
		vgx_launch_imm_publish(T, dev_sizes, dev_status, s);
	}
	// the totals to the mirror, for the next call (never waited for)
	ctx->imm.mirror.push(ctx, T, s);
	ctx->imm.pendTag = tag; ctx->imm.pendNDraws = ndraws; ctx->imm.pendDetect = detect;
	return launchStatus(ctx);
}

// ---- stroker-level entry ------------------------------------------------------------------------------
// The mesh descriptors of the caller's vertex lists: at most two meshes per list, so the scratch is sized without a device round trip
static int scanSubpathMeshes(vgx_ctx* ctx, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws, hipStream_t s)
{
	int st;
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensureMeshBuffers(ctx, 0, 0, 2 * nsubpaths)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	OpSubMeshes op;
	op.subs = subpaths; op.subDraw = subpath_draw; op.draws = draws; op.nsubs = nsubpaths; op.ndraws = ndraws;
	op.mdesc = ctx->mdesc.ptr(); op.mtab = ctx->mtab.ptr(); op.totals = ctx->totals.ptr();
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, nsubpaths);
	mark(ctx, s, "scan_subpath_meshes");
	return VGX_OK;
}

int vgx_stroke_count(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out_sizes || (nsubpaths && (!poly || !subpaths || !subpath_draw || !draws))) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	if ((st = scanSubpathMeshes(ctx, subpaths, subpath_draw, nsubpaths, draws, ndraws, s)) != VGX_OK) { return st; }
	runStrokeCount(ctx, draws, sizingCaps(ctx), 0, s, poly);
	if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
	*out_sizes = ctx->hostTotals->sizes;
	if (ctx->hostTotals->status != VGX_OK) { return (int)ctx->hostTotals->status; }
	ctx->counted = VgxCounted{ nullptr, draws, nsubpaths, VGX_COUNTED_STROKE };
	return VGX_OK;
}

int vgx_stroke_emit(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* stream)
{
	DeviceGuard guard(ctx);
	(void)subpaths; (void)subpath_draw; (void)ndraws;
	if (!ctx || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)) {
		return VGX_E_INVALID_ARG;
	}
	if (!followsCount(ctx, VGX_COUNTED_STROKE, nullptr, draws, nsubpaths)) {
		return VGX_E_INVALID_ARG; // must follow vgx_stroke_count on the same batch
	}
	const vgx_sizes& sz = ctx->hostTotals->sizes;
	if (out->cap_vertices < sz.num_vertices || out->cap_indices < sz.num_indices || (out->meshes && out->cap_meshes < sz.num_meshes)) {
		return VGX_E_NOSPACE;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	return runStrokeEmit(ctx, draws, out, s, poly);
}

int vgx_stroke(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws,
               const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	if (!ctx || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out) || (nsubpaths && (!poly || !subpaths || !subpath_draw || !draws))) { // (before the context is touched)
		return VGX_E_INVALID_ARG;
	}
	DeviceGuard guard(ctx);
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE; // counted state ends here
	tmplDrop(ctx);
	int st;
	if ((st = scanSubpathMeshes(ctx, subpaths, subpath_draw, nsubpaths, draws, ndraws, s)) != VGX_OK) { return st; }
	runStrokeCount(ctx, draws, outCapsFor(ctx, out), 1, s, poly, false, out->meshes); // sizes, places, the caller's capacities, its mesh table
	if ((st = runStrokeEmit(ctx, draws, out, s, poly, true)) != VGX_OK) { return st; }
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

// ---- dashed strokes -----------------------------------------------------------------------------------
int vgx_dash_validate(const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern)
{
	if ((ndraws && !dashes) || (npattern && !pattern)) { return VGX_E_INVALID_ARG; }
	for (uint64_t k = 0; k < npattern; ++k) {
		if (!vgx_dash_entry_ok(pattern[k])) { return VGX_E_INVALID_ARG; }
	}
	for (uint64_t d = 0; d < ndraws; ++d) {
		VgxDashPat p;
		if (!vgx_dash_pat_build(dashes[d], pattern, npattern, &p)) { return VGX_E_INVALID_ARG; }
	}
	return VGX_OK;
}

namespace {

int dashEnsureSegments(vgx_ctx* ctx, uint64_t segments)
{
	int st;
	if ((st = ensure(ctx, ctx->dashG, segments + 1)) != VGX_OK) { return st; }
	return ensure(ctx, ctx->dashGhi, segments + 1);
}

// everything but the launch: argument checks, scratch, the argument block
int dashPrepare(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths,
                const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern, uint64_t segGuess, VgxDashArgs* a)
{
	if ((nsubpaths && (!poly || !subpaths || !subpath_draw || !dashes || !ndraws)) || (ndraws && !dashes) || (npattern && !pattern)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)subpath_draw & 3u) || ((uintptr_t)dashes & 3u) || ((uintptr_t)pattern & 3u)) { return VGX_E_INVALID_ARG; }
	if (nsubpaths > 0x7FFFFFFFull || ndraws > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	ctx->counted.stage = VGX_COUNTED_NONE;
	tmplDrop(ctx);
	int st;
	if ((st = ctx->dash.create(ctx, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dashPat, ndraws + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dashLists, nsubpaths + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dashRange, (4 * VGX_DASH_RANGES + 4) * sizeof(uint64_t))) != VGX_OK) { return st; }
	// the segment tables: what the last call measured (once that has arrived), else what they hold, else a guess
	uint64_t segments = segGuess;
	if (ctx->dash.landed() && *ctx->dash.host > segments) { segments = *ctx->dash.host; }
	if (ctx->dashG.cap == 0 || segments + 1 > ctx->dashG.items()) {
		if ((st = dashEnsureSegments(ctx, segments)) != VGX_OK) { return st; }
	}
	memset(a, 0, sizeof(*a));
	a->poly = poly; a->subs = subpaths; a->sub_draw = subpath_draw; a->nsubs = nsubpaths;
	a->dashes = dashes; a->ndraws = ndraws; a->pattern = pattern; a->npattern = npattern;
	a->pat = ctx->dashPat.ptr(); a->lists = ctx->dashLists.ptr();
	a->G = ctx->dashG.ptr(); a->Ghi = ctx->dashGhi.ptr();
	a->seg_cap = minOf({ ctx->dashG.items(), ctx->dashGhi.items() }) - 1;
	a->range_sum = (uint64_t*)ctx->dashRange.p; a->range_off = a->range_sum + 2 * VGX_DASH_RANGES; a->tot = a->range_off + 2 * VGX_DASH_RANGES;
	a->totals = ctx->totals.ptr(); a->partial = (Sum3*)ctx->partial.p;
	return VGX_OK;
}

void dashLaunch(vgx_ctx* ctx, const VgxDashArgs& a, bool emit, hipStream_t s)
{
	noteHip(ctx, hipMemsetAsync(a.totals, 0, sizeof(VgxTotals), s));
	noteHip(ctx, hipMemsetAsync(a.tot, 0, 4 * sizeof(uint64_t), s));
	vgx_launch_dash(a, emit, s);
	mark(ctx, s, emit ? "dash" : "dash_count");
	// the segment count to the mirror, for the next call (never waited for)
	ctx->dash.push(ctx, a.tot, s);
}

} // namespace

int vgx_dash_count(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths,
                   const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern, vgx_sizes* out_sizes, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out_sizes) { return VGX_E_INVALID_ARG; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	for (int attempt = 0; ; ++attempt) { // a second round only when the lists outgrew the segment tables (the first count of a larger batch)
		VgxDashArgs a;
		int st = dashPrepare(ctx, poly, subpaths, subpath_draw, nsubpaths, dashes, ndraws, pattern, npattern, 65536, &a);
		if (st != VGX_OK) { return st; }
		dashLaunch(ctx, a, false, s);
		if ((st = launchStatus(ctx)) != VGX_OK) { return st; }
		if ((st = readTotals(ctx, s)) != VGX_OK) { return st; }
		if (ctx->hostTotals->status == VGX_E_GROWN && attempt == 0) { continue; } // the mirror holds the need, dashPrepare grows from it
		*out_sizes = ctx->hostTotals->sizes;
		return (int)ctx->hostTotals->status;
	}
}

int vgx_dash(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths,
             const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern,
             const vgx_dash_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out || !out->poly || !out->subpaths || !out->subpath_draw) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)out->poly & 7u) || ((uintptr_t)out->subpaths & 7u) || ((uintptr_t)out->subpath_draw & 3u) || ((uintptr_t)out->subpath_src & 3u)) { return VGX_E_INVALID_ARG; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	VgxDashArgs a;
	const int st = dashPrepare(ctx, poly, subpaths, subpath_draw, nsubpaths, dashes, ndraws, pattern, npattern,
	                           out->cap_poly_vertices > 65536 ? out->cap_poly_vertices : 65536, &a);
	if (st != VGX_OK) { return st; }
	a.out_poly = out->poly; a.out_subs = out->subpaths; a.out_draw = out->subpath_draw; a.out_src = out->subpath_src;
	a.cap_poly = out->cap_poly_vertices; a.cap_subs = out->cap_subpaths; a.check_caps = 1;
	dashLaunch(ctx, a, true, s);
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

// ---- dashed strokes in frames: vgx_tessellate_dashed / vgx_reserve_dashed -------------------------------------------------------
namespace {

// The context's scratch for frames of `meshes` meshes (source meshes that stay + pieces), `pieces` pieces of `pieceVerts` vertices: the
// tail of the polyline scratch (the flatten stage's heap keeps the vertices it has), both sets of mesh tables, the per-mesh lists, the
// pieces' records. Grow-only, like every table of the context.
int dfEnsure(vgx_ctx* ctx, uint64_t meshes, uint64_t pieces, uint64_t pieceVerts)
{
	int st;
	const uint64_t heap = ctx->poly.cap ? ctx->caps.poly_vertices : 4096;
	if (pieceVerts > ctx->pieceVerts) { ctx->pieceVerts = pieceVerts + pieceVerts / 8; }
	if ((st = ensureMeshBuffers(ctx, heap, 1024, meshes > 1024 ? meshes : 1024)) != VGX_OK) { return st; }
	const uint64_t m = ctx->caps.meshes + 1;
	if ((st = ensure(ctx, ctx->mdesc2, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mprep2, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mtab2, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfLists, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfListDraw, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfDashedBefore, m)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfPieceSubs, pieces + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfPieceDraw, pieces + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfPieceSrc, pieces + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dfTotals, 1)) != VGX_OK) { return st; }
	return ensure(ctx, ctx->dfNeed, 4);
}

uint64_t dfPieceCap(const vgx_ctx* ctx)
{
	return minOf({ ctx->dfPieceSubs.items(), ctx->dfPieceDraw.items(), ctx->dfPieceSrc.items() }) - 1;
}

} // namespace

int vgx_reserve_dashed(vgx_ctx* ctx, uint64_t ndraws, const vgx_sizes* totals, const vgx_sizes* dash_totals)
{
	if (!ctx || !totals || !dash_totals) { return VGX_E_INVALID_ARG; }
	int st;
	if ((st = vgx_reserve(ctx, ndraws, totals)) != VGX_OK) { return st; }
	DeviceGuard guard(ctx);
	if ((st = ctx->df.create(ctx, 4)) != VGX_OK) { return st; }
	if ((st = ctx->dash.create(ctx, 1)) != VGX_OK) { return st; }
	// every source mesh may stay (the frame's meshes + at most one dashed mesh without pieces per sub-path) and every piece is a mesh; a list
	// has at most as many segments as vertices
	if ((st = dfEnsure(ctx, totals->num_meshes + totals->num_subpaths + dash_totals->num_subpaths, dash_totals->num_subpaths, dash_totals->num_poly_vertices)) != VGX_OK) { return st; }
	if (totals->num_poly_vertices + 1 > ctx->dashG.items() || totals->num_poly_vertices + 1 > ctx->dashGhi.items()) {
		if ((st = dashEnsureSegments(ctx, totals->num_poly_vertices)) != VGX_OK) { return st; }
	}
	return VGX_OK;
}

int vgx_tessellate_dashed(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const struct vgx_dash* dashes, const float* pattern, uint64_t npattern,
                          const vgx_mesh_out* out, vgx_sizes* dev_sizes, vgx_sizes* dev_dash_sizes, uint32_t* dev_status, void* stream)
{
	if (!ctx || !ps || !out || (!draws && ndraws) || !out->pos || !out->color || !out->idx || meshOutMisaligned(out) || (npattern && !pattern)) { // (before the context is touched)
		return VGX_E_INVALID_ARG;
	}
	if (((uintptr_t)dashes & 3u) || ((uintptr_t)pattern & 3u)) { return VGX_E_INVALID_ARG; }
	if (!dashes || !ndraws) { // no dash records: the immediate call itself
		const int st0 = vgx_tessellate_immediate(ctx, ps, draws, ndraws, out, dev_sizes, dev_status, stream);
		if (st0 != VGX_OK) { return st0; }
		DeviceGuard guard0(ctx);
		if (dev_dash_sizes) { noteHip(ctx, hipMemsetAsync(dev_dash_sizes, 0, sizeof(vgx_sizes), (hipStream_t)stream)); }
		return launchStatus(ctx);
	}
	DeviceGuard guard(ctx);
	hipStream_t s = (hipStream_t)stream;
	int st;
	if ((st = ctx->df.create(ctx, 4)) != VGX_OK) { return st; }
	if ((st = immBegin(ctx, ps, ndraws)) != VGX_OK) { return st; }
	uint64_t needMeshes = 1024, needPieces = 4096, needPieceVerts = 16384;
	if (ctx->df.landed() && ctx->df.host[3]) { needPieces = ctx->df.host[0]; needPieceVerts = ctx->df.host[1]; needMeshes = ctx->df.host[2] + ctx->df.host[0]; }
	if ((st = dfEnsure(ctx, needMeshes, needPieces, needPieceVerts)) != VGX_OK) { return st; }
	const uint64_t tag = vgx_batch_tag(ps->gen, ndraws);
	const uint64_t segGuess = (ctx->imm.known && ctx->imm.tag == tag && ctx->imm.facts.V > 65536) ? ctx->imm.facts.V : 65536; // (segments <= vertices of the source lists)
	VgxDashArgs a;
	if ((st = dashPrepare(ctx, (const float*)ctx->poly.p, ctx->dfLists.ptr(), ctx->dfListDraw.ptr(), ctx->caps.meshes,
	                      dashes, ndraws, pattern, npattern, segGuess, &a)) != VGX_OK) { return st; }
	markBegin(ctx, s);
	VgxTotals* T = ctx->totals.ptr();
	// the flatten stage: k_flatten_build for any number of draws (its descriptors are complete and in frame order, the exact builder's included)
	mark(ctx, s, "route_build");
	runFlattenStage(ctx, ps, draws, ndraws, s); // (no route chosen: the build route, period 0)
	vgx_launch_imm_size(ps->dev, draws, ndraws, T, 1, false, nullptr, nullptr, s); // (a VGX_E_NOSPACE here is the scratch's)
	mark(ctx, s, "imm_size");
	// the dash pass over the stroke meshes of the dashed draws, pieces into the tail of the polyline scratch
	VgxDashFrameArgs f;
	memset(&f, 0, sizeof(f));
	f.draws = draws; f.dashes = dashes;
	f.mdesc = ctx->mdesc.ptr(); f.mtab = ctx->mtab.ptr(); f.mprep = ctx->mprep.ptr();
	f.mdesc2 = ctx->mdesc2.ptr(); f.mtab2 = ctx->mtab2.ptr(); f.mprep2 = ctx->mprep2.ptr();
	f.lists = ctx->dfLists.ptr(); f.list_draw = ctx->dfListDraw.ptr(); f.dashed_before = ctx->dfDashedBefore.ptr();
	f.need = ctx->dfNeed.ptr(); f.nlists = f.need + 2; // (the join writes the same value there)
	f.piece_subs = ctx->dfPieceSubs.ptr(); f.piece_src = ctx->dfPieceSrc.ptr();
	f.piece_base = ctx->caps.poly_vertices + 1;
	f.cap_meshes = ctx->caps.meshes;
	f.totals = T; f.dash_totals = ctx->dfTotals.ptr();
	f.dev_dash_sizes = dev_dash_sizes;
	f.partial = (Sum3*)ctx->partial.p;
	vgx_launch_dashframe_lists(f, s);
	mark(ctx, s, "dashframe_lists");
	a.totals = f.dash_totals;
	a.nsubs_dev = f.nlists; a.frame = 1;
	a.out_poly = (float*)ctx->poly.p + 2 * f.piece_base; a.out_subs = ctx->dfPieceSubs.ptr();
	a.out_draw = ctx->dfPieceDraw.ptr(); a.out_src = ctx->dfPieceSrc.ptr();
	a.cap_poly = ctx->pieceVerts; a.cap_subs = dfPieceCap(ctx); a.check_caps = 1;
	dashLaunch(ctx, a, true, s);
	// the frame's meshes by slot; from here on the second set of tables is the context's
	vgx_launch_dashframe_place(f, s);
	mark(ctx, s, "dashframe_place");
	vgx_scratch_swap(ctx->scratch, ctx->mdesc, ctx->mdesc2);
	vgx_scratch_swap(ctx->scratch, ctx->mprep, ctx->mprep2);
	vgx_scratch_swap(ctx->scratch, ctx->mtab, ctx->mtab2);
	if ((st = ensureMeshBuffers(ctx, 0, 0, 0)) != VGX_OK) { return st; } // (caps from the swapped tables: the sets may differ in head room)
	runStrokeCount(ctx, draws, outCapsFor(ctx, out), 1, s, nullptr, true, out->meshes);
	if ((st = runStrokeEmit(ctx, draws, out, s, nullptr, true)) != VGX_OK) { return st; }
	vgx_launch_imm_publish(T, dev_sizes, dev_status, s);
	// the totals and the pieces' need to the mirrors, for the next call (never waited for)
	ctx->imm.mirror.push(ctx, T, s);
	ctx->imm.pendTag = tag; ctx->imm.pendNDraws = ndraws; ctx->imm.pendDetect = false;
	ctx->df.push(ctx, ctx->dfNeed.p, s);
	return launchStatus(ctx);
}

int vgx_subpath_draws(vgx_ctx* ctx, const vgx_draw_info* draw_info, uint64_t ndraws, uint32_t* subpath_draw, uint64_t nsubpaths, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (nsubpaths && (!draw_info || !subpath_draw || !ndraws)) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)subpath_draw & 3u)) { return VGX_E_INVALID_ARG; }
	if (nsubpaths) { vgx_launch_subpath_draws(draw_info, ndraws, subpath_draw, nsubpaths, (hipStream_t)stream); }
	return launchStatus(ctx);
}

// ---- shape cache ------------------------------------------------------------------------------------
int vgx_cache_localize(vgx_ctx* ctx, const vgx_draw* draws, uint64_t ndraws, float* pos, const vgx_mesh* meshes, uint64_t num_meshes, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (num_meshes && (!draws || !pos || !meshes))) {
		return VGX_E_INVALID_ARG;
	}
	if (num_meshes) {
		vgx_launch_cache_localize(draws, ndraws, pos, meshes, num_meshes, (hipStream_t)stream);
	}
	return VGX_OK;
}

int vgx_cache_submit(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* instances, uint64_t ninst, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !cache || !out || (!instances && ninst) || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)
		|| (cache->num_meshes && (!cache->pos || !cache->color || !cache->idx || !cache->meshes))) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	// the three instance prefix arrays share one scratch buffer; the output mesh table lives in the mesh-table scratch
	if ((st = ensure(ctx, ctx->cmdPrefix, 3 * (ninst + 1) * sizeof(uint64_t))) != VGX_OK) { return st; }
	// the internal mesh table must hold every output mesh even when the caller does not want the table
	uint64_t meshCap = out->meshes ? out->cap_meshes : cache->num_meshes * ninst;
	if (meshCap == 0) { meshCap = 1; }
	if ((st = ensure(ctx, ctx->mtab, meshCap + 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	uint64_t* prefix = (uint64_t*)ctx->cmdPrefix.p;
	OpCacheInst op;
	op.cache = *cache; op.inst = instances; op.ninst = ninst;
	op.meshPrefix = prefix; op.vertPrefix = prefix + (ninst + 1); op.idxPrefix = prefix + 2 * (ninst + 1);
	op.totals = ctx->totals.ptr();
	op.caps = ctx->caps;
	op.caps.meshes = ctx->mtab.items() - 1;
	if (out->meshes && out->cap_meshes < op.caps.meshes) { op.caps.meshes = out->cap_meshes; }
	op.caps.vertices = out->cap_vertices; op.caps.indices = out->cap_indices;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ninst);
	mark(ctx, s, "scan_instances");
	VgxCacheArgs a;
	a.cache = *cache; a.inst = instances; a.ninst = ninst;
	a.inst_mesh_prefix = op.meshPrefix; a.inst_vert_prefix = op.vertPrefix; a.inst_idx_prefix = op.idxPrefix;
	a.mtab = ctx->mtab.ptr(); a.meshes_out = out->meshes;
	a.pos = out->pos; a.color = out->color; a.idx = out->idx;
	a.mesh_base = nullptr;
	a.totals = ctx->totals.ptr();
	vgx_launch_cache_meshes(a, s);
	mark(ctx, s, "cache_meshes");
	if (ctx->asmArmed) {
		if ((st = runAssemble(ctx, out, s)) != VGX_OK) { return st; }
		a.mesh_base = ctx->meshBase.ptr();
	}
	vgx_launch_cache_copy(a, vgxElementGrid(out->cap_vertices), s);
	mark(ctx, s, "cache_copy");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

// ---- mesh bounds, view culling of cached instances (vgx_bounds.hip) -----------------------------------
// Neither call touches the totals, the mesh tables or the stage of a counted state: count -> these -> emit still works.
int vgx_mesh_bounds(vgx_ctx* ctx, const float* pos, const vgx_mesh* meshes, uint64_t num_meshes, float* bounds, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (num_meshes && (!pos || !meshes || !bounds)) || ((uintptr_t)pos & 7u) || ((uintptr_t)meshes & 7u) || ((uintptr_t)bounds & 15u)) {
		return VGX_E_INVALID_ARG;
	}
	if (num_meshes > 0xFFFFFFFFull * 256ull) { return VGX_E_RANGE; }
	if (num_meshes) { vgx_launch_mesh_bounds(pos, meshes, num_meshes, bounds, (hipStream_t)stream); }
	return launchStatus(ctx);
}

int vgx_cache_cull(vgx_ctx* ctx, const vgx_cache_desc* cache, const float* mesh_bounds, const vgx_cache_instance* inst, uint64_t ninst,
                   const float* views, uint32_t nviews, const uint32_t* inst_view, const vgx_cull_out* out, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !cache || !out || (ninst && (!inst || !out->inst || !views || !nviews)) || (cache->num_meshes && !mesh_bounds)) {
		return VGX_E_INVALID_ARG;
	}
	if (((uintptr_t)mesh_bounds & 15u) || ((uintptr_t)inst & 7u) || ((uintptr_t)out->inst & 7u) || ((uintptr_t)out->bounds & 15u) || ((uintptr_t)views & 3u)
		|| ((uintptr_t)inst_view & 3u) || ((uintptr_t)out->kept & 3u) || ((uintptr_t)out->num_kept & 7u) || ((uintptr_t)dev_status & 3u)) {
		return VGX_E_INVALID_ARG;
	}
	if (ninst > 0xFFFFFFFFull) { return VGX_E_RANGE; } // `kept` holds 32-bit indices
	hipStream_t s = (hipStream_t)stream;
	const bool compact = out->kept || out->num_kept;
	int st;
	if (compact) {
		if ((st = ensure(ctx, ctx->cullFlags, ninst + 1)) != VGX_OK) { return st; }
		if ((st = ensure(ctx, ctx->cullPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	}
	if (dev_status) { noteHip(ctx, hipMemsetAsync(dev_status, 0, sizeof(uint32_t), s)); } // VGX_OK
	VgxCullArgs a;
	memset(&a, 0, sizeof(a));
	a.cache_meshes = cache->num_meshes; a.mesh_bounds = mesh_bounds; a.inst = inst; a.ninst = ninst;
	a.views = views; a.nviews = nviews; a.inst_view = inst_view;
	a.out_inst = out->inst; a.out_bounds = out->bounds; a.flags = compact ? ctx->cullFlags.ptr() : nullptr; a.status = dev_status;
	vgx_launch_cache_cull(a, out->kept, out->num_kept, ctx->cullPartial.p, s);
	return launchStatus(ctx);
}

// ---- hit testing (vgx_pick.hip) ------------------------------------------------------------------------------------------
// Scratch of its own, like the culling call: count -> vgx_pick -> emit still works.
int vgx_pick(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_pick_query* queries, uint32_t nqueries,
             vgx_pick_hit* hits, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !frame || (nqueries && (!queries || !hits))) { return VGX_E_INVALID_ARG; }
	if (nqueries && frame->num_meshes && (!frame->pos || !frame->color || !frame->idx || !frame->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)queries & 15u) || ((uintptr_t)hits & 15u) || ((uintptr_t)mesh_bounds & 15u) || ((uintptr_t)frame->pos & 7u)
		|| ((uintptr_t)frame->color & 3u) || ((uintptr_t)frame->idx & 1u) || ((uintptr_t)frame->meshes & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (nqueries > VGX_PICK_MAX_QUERIES || frame->num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	if (!nqueries) { return VGX_OK; } // nothing to write
	hipStream_t s = (hipStream_t)stream;
	const uint64_t nm = frame->num_meshes;
	int st;
	if ((st = ensure(ctx, ctx->pickKeys, VGX_PICK_MAX_QUERIES)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickTris, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickCand, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickPrefix, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickTotals, 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if (!mesh_bounds && nm) {
		if ((st = ensure(ctx, ctx->pickBounds, nm * 4)) != VGX_OK) { return st; }
		vgx_launch_mesh_bounds(frame->pos, frame->meshes, nm, ctx->pickBounds.ptr(), s);
		mesh_bounds = ctx->pickBounds.ptr();
	}
	VgxPickArgs a;
	memset(&a, 0, sizeof(a));
	a.pos = frame->pos; a.color = frame->color; a.idx = frame->idx; a.meshes = frame->meshes; a.num_meshes = nm;
	a.mesh_bounds = mesh_bounds; a.queries = queries; a.nqueries = nqueries; a.hits = hits;
	a.keys = ctx->pickKeys.ptr(); a.cand_tris = ctx->pickTris.ptr(); a.cand_mesh = ctx->pickCand.ptr();
	a.cand_prefix = ctx->pickPrefix.ptr(); a.totals = ctx->pickTotals.ptr();
	vgx_launch_pick(a, ctx->pickPartial.p, ctx->opt.pickGrid, s);
	return launchStatus(ctx);
}

// ... under per-draw scissors, clip regions and contour fills. Scratch of its own: count -> vgx_pick_frame -> emit still works, and so does
// vgx_pick -> vgx_pick_frame -> vgx_pick.
int vgx_pick_frame(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                   const vgx_pick_query* queries, uint32_t nqueries, vgx_pick_hit* hits, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_pickf_check_args(frame, mesh_bounds, state, queries, nqueries, hits, dev_status);
	if (st != VGX_OK) { return st; }
	hipStream_t s = (hipStream_t)stream;
	const uint64_t end = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
	const uint64_t nrange = mesh_begin < end ? end - mesh_begin : 0;
	if ((st = ensure(ctx, ctx->pickfState, nrange + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfCand, nrange + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfTriCand, nrange + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfConCand, nrange + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfCover, 8 * (nrange + 1))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfPrefix, nrange + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfTotals, 4)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickfPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if (!mesh_bounds && nrange) {
		if ((st = ensure(ctx, ctx->pickfBounds, frame->num_meshes * 4)) != VGX_OK) { return st; }
		vgx_launch_mesh_bounds(frame->pos, frame->meshes + mesh_begin, nrange, ctx->pickfBounds.ptr() + 4 * mesh_begin, s); // the range's boxes only
		mesh_bounds = ctx->pickfBounds.ptr();
	}
	VgxPickfArgs a;
	memset(&a, 0, sizeof(a));
	a.pos = frame->pos; a.color = frame->color; a.idx = frame->idx; a.meshes = frame->meshes; a.mesh_bounds = mesh_bounds;
	a.mesh_begin = mesh_begin; a.nrange = nrange;
	a.draws = state->draws; a.draw_state = state->draw_state; a.num_draws = state->num_draws;
	a.queries = queries; a.nqueries = nqueries; a.hits = hits; a.status = dev_status;
	a.mesh_state = ctx->pickfState.ptr(); a.cand_mesh = ctx->pickfCand.ptr(); a.tri_cand = ctx->pickfTriCand.ptr(); a.tri_prefix = ctx->pickfPrefix.ptr();
	a.con_cand = ctx->pickfConCand.ptr(); a.cover = ctx->pickfCover.ptr(); a.totals = ctx->pickfTotals.ptr();
	vgx_launch_pick_frame(a, ctx->pickfPartial.p, ctx->opt.pickGrid, s);
	return launchStatus(ctx);
}

// ... of rectangles: pick tolerance and marquee selection (vgx_pick_rect.hip). Scratch of its own, sized by num_meshes alone: count ->
// vgx_pick_rect -> emit still works, and so does vgx_pick -> vgx_pick_rect -> vgx_pick.
int vgx_pick_rect(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_pick_rect_query* queries, uint32_t nqueries,
                  const vgx_pick_rect_out* out, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_pickr_check_args(frame, mesh_bounds, queries, nqueries, out);
	if (st != VGX_OK) { return st; }
	if (!nqueries) { return VGX_OK; } // nothing to write
	hipStream_t s = (hipStream_t)stream;
	const uint64_t nm = frame->num_meshes, words = (nm + 63) / 64 * 64; // blocks of 64 meshes x 64 queries
	if ((st = ensure(ctx, ctx->pickrCand, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrInside, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrTouch, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrTris, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrCandMesh, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrPrefix, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrRunOf, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrRunFirst, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrRunTouch, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrRunInside, nm + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrBlockCount, words + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrBlockTop, words + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrTotals, 3)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickrPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if (!mesh_bounds && nm) {
		if ((st = ensure(ctx, ctx->pickrBounds, nm * 4)) != VGX_OK) { return st; }
		vgx_launch_mesh_bounds(frame->pos, frame->meshes, nm, ctx->pickrBounds.ptr(), s);
		mesh_bounds = ctx->pickrBounds.ptr();
	}
	VgxPickrArgs a;
	memset(&a, 0, sizeof(a));
	a.pos = frame->pos; a.color = frame->color; a.idx = frame->idx; a.meshes = frame->meshes; a.num_meshes = nm;
	a.mesh_bounds = mesh_bounds; a.queries = queries; a.nqueries = nqueries;
	a.top = out->top; a.list = out->list; a.count = out->count; a.list_cap = out->list_cap;
	a.cand = ctx->pickrCand.ptr(); a.inside = ctx->pickrInside.ptr(); a.touch = ctx->pickrTouch.ptr(); a.cand_tris = ctx->pickrTris.ptr();
	a.cand_mesh = ctx->pickrCandMesh.ptr(); a.cand_prefix = ctx->pickrPrefix.ptr(); a.run_of = ctx->pickrRunOf.ptr(); a.run_first = ctx->pickrRunFirst.ptr();
	a.run_touch = ctx->pickrRunTouch.ptr(); a.run_inside = ctx->pickrRunInside.ptr(); a.block_count = ctx->pickrBlockCount.ptr();
	a.block_top = ctx->pickrBlockTop.ptr(); a.totals = ctx->pickrTotals.ptr();
	vgx_launch_pick_rect(a, ctx->pickrPartial.p, ctx->opt.pickGrid, s);
	return launchStatus(ctx);
}

// ... of a draw-command table: the assembled frame (vgx_pick_cmds.hip). Scratch of its own, sized by the table and the queries alone.
// The two calls are one body; cmd_bounds (vgx_pick_commands_boxed; else null) picks the kernels that look at the boxes
namespace {

int pickCommandsCall(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds, const float* cmd_bounds,
                     const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_pickc_check_args(streams, cmds, num_cmds, dev_num_cmds, owners, queries, nqueries, hits, dev_status);
	if (st != VGX_OK) { return st; }
	if ((uintptr_t)cmd_bounds & 15u) { return VGX_E_INVALID_ARG; }
	hipStream_t s = (hipStream_t)stream;
	if ((st = ensure(ctx, ctx->pickcState, (uint64_t)num_cmds + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickcFirst, (uint64_t)num_cmds + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickcTop, (uint64_t)num_cmds * nqueries + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickcWords, VGX_PICKC_WORDS)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->pickcPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	VgxPickcArgs a;
	memset(&a, 0, sizeof(a));
	a.pos = streams->pos; a.color = streams->color; a.idx = streams->idx; a.num_vertices = streams->num_vertices; a.num_indices = streams->num_indices;
	a.cmds = cmds; a.num_cmds = num_cmds; a.dev_num_cmds = dev_num_cmds;
	if (owners) { a.meshes = owners->meshes; a.num_meshes = owners->num_meshes; }
	a.queries = queries; a.nqueries = nqueries; a.hits = hits; a.status = dev_status;
	a.cmd_state = ctx->pickcState.ptr(); a.cmd_first = ctx->pickcFirst.ptr(); a.top = ctx->pickcTop.ptr(); a.state = ctx->pickcWords.ptr();
	a.cmd_bounds = num_cmds ? cmd_bounds : nullptr;
	vgx_launch_pick_commands(a, ctx->pickcPartial.p, ctx->opt.pickGrid, s);
	return launchStatus(ctx);
}

} // namespace

int vgx_pick_commands(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                      const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits, uint32_t* dev_status, void* stream)
{
	return pickCommandsCall(ctx, streams, cmds, num_cmds, dev_num_cmds, nullptr, owners, queries, nqueries, hits, dev_status, stream);
}

int vgx_pick_commands_boxed(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                            const float* cmd_bounds, const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits,
                            uint32_t* dev_status, void* stream)
{
	return pickCommandsCall(ctx, streams, cmds, num_cmds, dev_num_cmds, cmd_bounds, owners, queries, nqueries, hits, dev_status, stream);
}

// ---- per-command boxes of a draw-command table (vgx_cmd_bounds.hip) ------------------------------------------------------------------
// Scratch of its own, sized by the range alone: count -> vgx_command_bounds -> emit still works.
int vgx_command_bounds(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                       uint32_t cmd_begin, uint32_t cmd_end, float* bounds, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_cmdb_check_args(streams, cmds, num_cmds, dev_num_cmds, cmd_begin, cmd_end, bounds, dev_status);
	if (st != VGX_OK) { return st; }
	hipStream_t s = (hipStream_t)stream;
	const uint32_t range = vgx_cmdb_range(num_cmds, cmd_begin, cmd_end);
	if ((st = ensure(ctx, ctx->cmdbFirst, (uint64_t)range + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->cmdbWords, VGX_CMDB_WORDS)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->cmdbPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	VgxCmdBoundsArgs a;
	memset(&a, 0, sizeof(a));
	a.pos = streams->pos; a.idx = streams->idx; a.num_vertices = streams->num_vertices; a.num_indices = streams->num_indices;
	a.cmds = cmds; a.dev_num_cmds = dev_num_cmds; a.num_cmds = num_cmds; a.cmd_begin = cmd_begin; a.cmd_end = cmd_end;
	a.bounds = (uint32_t*)bounds; a.status = dev_status;
	a.cmd_first = ctx->cmdbFirst.ptr(); a.state = ctx->cmdbWords.ptr();
	vgx_launch_command_bounds(a, ctx->cmdbPartial.p, ctx->opt.pickGrid, s);
	return launchStatus(ctx);
}

// ---- rendering to an image (vgx_raster.hip) ---------------------------------------------------------------------------------
// Scratch of its own, like the picking call: count -> vgx_raster -> emit still works.
namespace {

int rasterEnsure(vgx_ctx* ctx, uint64_t meshes, uint64_t entries)
{
	int st;
	if ((st = ensure(ctx, ctx->rasState, 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasMeshEntries, meshes + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasMeshFirst, meshes + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasKeys, entries + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasVals, entries + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasSortedKeys, entries + 1)) != VGX_OK) { return st; }
	return ensure(ctx, ctx->rasSortedVals, entries + 1);
}

} // namespace

int vgx_raster_reserve(vgx_ctx* ctx, uint64_t num_meshes, uint64_t num_bin_entries)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	if (num_meshes >= 0xFFFFFFFFull || num_bin_entries > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	return rasterEnsure(ctx, num_meshes, num_bin_entries);
}

namespace {

// ---- what the frame calls (VgxRasterArgs) and the commands calls (VgxRasterCmdArgs) fill alike: the same-named fields of the two -----
// the scissor holds no pixel: the call writes VGX_OK and is over
bool rasterNothingToWrite(vgx_ctx* ctx, const vgx_raster_target& t, uint32_t* dev_status, hipStream_t s)
{
	if (t.scissor[0] != t.scissor[2] && t.scissor[1] != t.scissor[3]) { return false; }
	if (dev_status) { noteHip(ctx, hipMemsetAsync(dev_status, 0, sizeof(uint32_t), s)); } // VGX_OK
	return true;
}

extern "C++" { // templates, inside the C-ABI block
// the target as the kernels see it, and the plan of its tiles: the grid of the scissor's tiles, the sentinel key behind every tile
template <class Args>
void rasterTarget(Args& a, const vgx_raster_target& t)
{
	a.pixels = t.pixels; a.stride = t.stride; a.x0 = t.x0; a.y0 = t.y0;
	for (int k = 0; k < 4; ++k) { a.scissor[k] = t.scissor[k]; }
	a.flags = t.flags; a.clear_color = t.clear_color;
	a.tiles_w = (t.width + VGX_RASTER_TILE - 1) / VGX_RASTER_TILE;
	a.tile_x0 = t.scissor[0] / VGX_RASTER_TILE; a.tile_y0 = t.scissor[1] / VGX_RASTER_TILE;
	a.tiles_x = (t.scissor[2] - 1) / VGX_RASTER_TILE - a.tile_x0 + 1; a.tiles_y = (t.scissor[3] - 1) / VGX_RASTER_TILE - a.tile_y0 + 1;
	a.sentinel = a.tiles_w * ((t.height + VGX_RASTER_TILE - 1) / VGX_RASTER_TILE); // <= 2^20
	for (a.sort_bits = 1; (a.sentinel >> a.sort_bits) != 0; ++a.sort_bits) { }
}

// the sort's temporary storage for a.sort_n entries, in rasSortTemp
template <class Args>
int rasterSortStorage(vgx_ctx* ctx, const Args& a, size_t* sortBytes)
{
	*sortBytes = a.sort_n ? vgx_raster_sort_bytes(a.sort_n, a.sort_bits) : 0;
	if (!a.sort_n) { return VGX_OK; }
	return *sortBytes ? ensure(ctx, ctx->rasSortTemp, *sortBytes) : (int)VGX_E_INTERNAL;
}
} // extern "C++"

// The five calls are one body; `level` (VGX_RL_*, vgx_raster.h) says which pointers count and which kernel family runs. `damage`
// (vgx_raster_damaged, at VGX_RL_CONCAVE; else null) restricts the call to the marked tiles and gives it a sort window of its own
int rasterCall(int level, vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
               const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target, const vgx_raster_damage* damage,
               uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_raster_check_args(level, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, dev_status);
	if (st != VGX_OK) { return st; }
	if (damage && vgx_damage_record_check(damage) != VGX_OK) { return VGX_E_INVALID_ARG; }
	const vgx_raster_target& t = *target;
	hipStream_t s = (hipStream_t)stream;
	if (rasterNothingToWrite(ctx, t, dev_status, s)) { return launchStatus(ctx); }
	const uint64_t end = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
	const uint64_t nrange = mesh_begin < end ? end - mesh_begin : 0;
	VgxRasterArgs a;
	memset(&a, 0, sizeof(a));
	rasterTarget(a, t);
	HostMirror<unsigned long long>& mirror = damage ? ctx->rasDmg : ctx->ras;
	if ((st = mirror.create(ctx, 2)) != VGX_OK) { return st; }
	// no mesh has more entries than the scissor has tiles: the sort need not look further
	const uint64_t bound = nrange * ((uint64_t)a.tiles_x * a.tiles_y);
	// the entry tables: what the last call measured (once that has arrived), else what they hold, else one entry per mesh
	uint64_t entries = ctx->rasKeys.cap ? ctx->rasKeys.items() - 1 : nrange;
	uint64_t window = ~0ull;
	if (!damage) {
		if (ctx->ras.landed() && ctx->ras.host[0] == VGX_E_GROWN && ctx->ras.host[1] > entries) { entries = ctx->ras.host[1]; }
	} else {
		// The damaged call sorts a window, not what a full render left the tables at. max_entries is clipped to what the tables hold
		// (they grow by a measured need, never by a wish), and the tables grow to the window before it becomes the capacity
		if (mirror.landed()) { vgx_damage_learn(&ctx->rasDmgWindow, mirror.host[0], mirror.host[1]); }
		window = vgx_damage_window(ctx->rasDmgWindow, damage->max_entries, entries, bound);
		if (window > entries) { entries = window; }
	}
	if ((st = rasterEnsure(ctx, nrange, entries)) != VGX_OK) { return st; }
	a.entry_cap = minOf({ ctx->rasKeys.items(), ctx->rasVals.items(), ctx->rasSortedKeys.items(), ctx->rasSortedVals.items() }) - 1;
	if (window < a.entry_cap) { a.entry_cap = window; }
	a.sort_n = bound < a.entry_cap ? bound : a.entry_cap;
	size_t sortBytes;
	if ((st = rasterSortStorage(ctx, a, &sortBytes)) != VGX_OK) { return st; }
	if (!mesh_bounds && nrange) {
		if ((st = ensure(ctx, ctx->rasBounds, frame->num_meshes * 4)) != VGX_OK) { return st; }
		vgx_launch_mesh_bounds(frame->pos, frame->meshes + mesh_begin, nrange, ctx->rasBounds.ptr() + 4 * mesh_begin, s); // the range's boxes only
		mesh_bounds = ctx->rasBounds.ptr();
	}
	a.pos = frame->pos; a.color = frame->color; a.idx = frame->idx; a.meshes = frame->meshes; a.mesh_bounds = mesh_bounds;
	a.mesh_begin = mesh_begin; a.nrange = nrange;
	a.mesh_entries = ctx->rasMeshEntries.ptr(); a.mesh_first = ctx->rasMeshFirst.ptr();
	a.keys = ctx->rasKeys.ptr(); a.vals = ctx->rasVals.ptr(); a.sorted_keys = ctx->rasSortedKeys.ptr(); a.sorted_vals = ctx->rasSortedVals.ptr();
	a.state = ctx->rasState.ptr(); a.status = dev_status;
	if (level == VGX_RL_PLAIN) {
		noteHip(ctx, vgx_launch_raster(a, ctx->rasPartial.p, ctx->rasSortTemp.p, sortBytes, s));
	} else {
		if ((st = ensure(ctx, ctx->rasFrameMesh, nrange + 1)) != VGX_OK) { return st; }
		VgxRasterFrameArgs f;
		memset(&f, 0, sizeof(f));
		f.R = a; f.level = level;
		f.draws = state->draws; f.draw_state = state->draw_state; f.num_draws = state->num_draws; f.mesh_state = ctx->rasFrameMesh.ptr();
		// a tile bitmap exists, zeroed, at the levels that can set a bit in it; below them the pointer stays null: "no bit set"
		const uint64_t words = ((uint64_t)a.sentinel + 31u) / 32u;
		if (level >= VGX_RL_TEXTURED) {
			f.uv = tex->uv; f.images = tex->images; f.uv_bytes = tex->uv_bytes; f.num_images = tex->num_images;
			if ((st = ensure(ctx, ctx->rasTileTex, words + 1)) != VGX_OK) { return st; }
			noteHip(ctx, hipMemsetAsync(ctx->rasTileTex.p, 0, words * sizeof(uint32_t), s));
			f.tile_tex = ctx->rasTileTex.ptr();
		}
		if (level >= VGX_RL_PAINTED) {
			f.gradients = paints->gradients; f.patterns = paints->patterns; f.num_gradients = paints->num_gradients; f.num_patterns = paints->num_patterns;
			if ((st = ensure(ctx, ctx->rasTilePaint, words + 1)) != VGX_OK) { return st; }
			noteHip(ctx, hipMemsetAsync(ctx->rasTilePaint.p, 0, words * sizeof(uint32_t), s));
			f.tile_paint = ctx->rasTilePaint.ptr();
		}
		if (level >= VGX_RL_CONCAVE) {
			if ((st = ensure(ctx, ctx->rasTileContour, words + 1)) != VGX_OK) { return st; }
			noteHip(ctx, hipMemsetAsync(ctx->rasTileContour.p, 0, words * sizeof(uint32_t), s));
			f.tile_contour = ctx->rasTileContour.ptr();
		}
		if (damage) { f.damage = damage->tile_bits; }
		noteHip(ctx, vgx_launch_raster_frame(f, ctx->rasPartial.p, ctx->rasSortTemp.p, sortBytes, s));
	}
	// status and entry count to the mirror, for the next call (never waited for)
	mirror.push(ctx, a.state, s);
	return launchStatus(ctx);
}

} // namespace

int vgx_raster_damaged(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                       const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target,
                       const vgx_raster_damage* damage, uint32_t* dev_status, void* stream)
{
	if (!damage) { return VGX_E_INVALID_ARG; }
	return rasterCall(VGX_RL_CONCAVE, ctx, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, damage, dev_status, stream);
}

// ---- damage marks (vgx_damage.hip) --------------------------------------------------------------------------------------------
uint64_t vgx_damage_words(uint32_t width, uint32_t height)
{
	return ((uint64_t)vgx_damage_tiles_w(width) * vgx_damage_tiles_w(height) + 31u) / 32u;
}

namespace {

// what both mark calls ask of the target and the bitmap; fills the target's part of the arguments
static int damageTarget(const vgx_raster_target* t, const uint32_t* tile_bits, VgxDamageArgs* a)
{
	if (!t || !tile_bits || ((uintptr_t)tile_bits & 3u)) { return VGX_E_INVALID_ARG; }
	if (vgx_target_extent_check(*t) != VGX_OK) { return VGX_E_INVALID_ARG; }
	memset(a, 0, sizeof(*a));
	a->x0 = t->x0; a->y0 = t->y0; a->width = t->width; a->height = t->height; a->tiles_w = vgx_damage_tiles_w(t->width);
	a->tile_bits = const_cast<uint32_t*>(tile_bits);
	return VGX_OK;
}

} // namespace

// Neither call touches a counted state, nor the scratch of vgx_cache_update: the chain mark -> update -> mark runs on one stream
int vgx_damage_meshes(vgx_ctx* ctx, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, uint64_t num_meshes, const vgx_raster_target* target,
                      uint32_t* tile_bits, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (num_meshes && !mesh_bounds) || ((uintptr_t)mesh_bounds & 15u)) { return VGX_E_INVALID_ARG; }
	VgxDamageArgs a;
	const int st = damageTarget(target, tile_bits, &a);
	if (st != VGX_OK) { return st; }
	if (num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	const uint64_t end = mesh_end < num_meshes ? mesh_end : num_meshes;
	a.mesh_bounds = mesh_bounds; a.num_meshes = num_meshes; a.mesh_begin = mesh_begin; a.nrange = mesh_begin < end ? end - mesh_begin : 0;
	vgx_launch_damage_meshes(a, (hipStream_t)stream);
	return launchStatus(ctx);
}

int vgx_damage_instances(vgx_ctx* ctx, const float* mesh_bounds, uint64_t num_meshes, const vgx_cache_slot* slots, uint64_t ninst, const uint32_t* dirty,
                         uint64_t ndirty, const uint64_t* dev_ndirty, const vgx_raster_target* target, uint32_t* tile_bits, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (ndirty && (!dirty || !slots)) || (ndirty && num_meshes && !mesh_bounds)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)mesh_bounds & 15u) || ((uintptr_t)slots & 7u) || ((uintptr_t)dev_ndirty & 7u) || ((uintptr_t)dirty & 3u) || ((uintptr_t)dev_status & 3u)) {
		return VGX_E_INVALID_ARG;
	}
	VgxDamageArgs a;
	int st = damageTarget(target, tile_bits, &a);
	if (st != VGX_OK) { return st; }
	if (num_meshes >= 0xFFFFFFFFull || ninst > 0xFFFFFFFFull || ndirty > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	// [flag word, padded to 16 bytes][mesh prefix: ndirty + 1]
	if ((st = ensure(ctx, ctx->dmgPrefix, 16 + (ndirty + 1) * sizeof(uint64_t))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->dmgPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->dmgPrefix.p, 0, 16, s));
	a.mesh_bounds = mesh_bounds; a.num_meshes = num_meshes; a.slots = slots; a.ninst = ninst; a.dirty = dirty; a.ndirty = ndirty; a.dev_ndirty = dev_ndirty;
	a.flags = (uint32_t*)ctx->dmgPrefix.p; a.mesh_prefix = (uint64_t*)((char*)ctx->dmgPrefix.p + 16);
	a.status = dev_status;
	vgx_launch_damage_instances(a, ctx->dmgPartial.p, s);
	return launchStatus(ctx);
}

int vgx_raster(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
               const vgx_raster_target* target, uint32_t* dev_status, void* stream)
{
	return rasterCall(VGX_RL_PLAIN, ctx, frame, mesh_bounds, mesh_begin, mesh_end, nullptr, nullptr, nullptr, target, nullptr, dev_status, stream);
}

int vgx_raster_frame(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                     const vgx_raster_draws* state, const vgx_raster_target* target, uint32_t* dev_status, void* stream)
{
	return rasterCall(VGX_RL_FRAME, ctx, frame, mesh_bounds, mesh_begin, mesh_end, state, nullptr, nullptr, target, nullptr, dev_status, stream);
}

int vgx_raster_textured(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                        const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_target* target, uint32_t* dev_status, void* stream)
{
	return rasterCall(VGX_RL_TEXTURED, ctx, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, nullptr, target, nullptr, dev_status, stream);
}

int vgx_raster_painted(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                       const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target,
                       uint32_t* dev_status, void* stream)
{
	return rasterCall(VGX_RL_PAINTED, ctx, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, nullptr, dev_status, stream);
}

int vgx_raster_concave(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                       const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target,
                       uint32_t* dev_status, void* stream)
{
	return rasterCall(VGX_RL_CONCAVE, ctx, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, nullptr, dev_status, stream);
}

// ---- a draw-command table to an image (vgx_raster_cmds.hip) -------------------------------------------------------------------
namespace {

// chunks and entries the tables hold at least; the capacity the kernels see grows with them and never shrinks
int rasterCmdsEnsure(vgx_ctx* ctx, uint64_t cmds, uint64_t chunks, uint64_t entries)
{
	int st;
	const uint64_t chunkCap = chunks + chunks / 8, entryCap = entries + entries / 8;
	if (chunkCap > ctx->rascChunkCap) { ctx->rascChunkCap = chunkCap; }
	if (entryCap > ctx->rascEntryCap) { ctx->rascEntryCap = entryCap; }
	if ((st = ensure(ctx, ctx->rascState, VGX_RASC_WORDS)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rasPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascCmdState, cmds + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascCmdFirst, cmds + 2)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascChunkRect, ctx->rascChunkCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascChunkCmd, ctx->rascChunkCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascChunkFirst, ctx->rascChunkCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascKeys, ctx->rascEntryCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascVals, ctx->rascEntryCap + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->rascSortedKeys, ctx->rascEntryCap + 1)) != VGX_OK) { return st; }
	return ensure(ctx, ctx->rascSortedVals, ctx->rascEntryCap + 1);
}

} // namespace

int vgx_raster_commands_reserve(vgx_ctx* ctx, uint32_t num_cmds, uint64_t num_chunks, uint64_t num_bin_entries)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	if (num_chunks > 0xFFFFFFFFull || num_bin_entries > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	return rasterCmdsEnsure(ctx, num_cmds, num_chunks, num_bin_entries);
}

namespace {

// The two calls are one body. `damage` (vgx_raster_commands_damaged; else null) restricts the call to the marked tiles and gives it a
// sort window and a mirror of its own; cmd_bounds (with damage alone; may be null) lets a command whose box reaches no marked tile out
int rasterCommandsCall(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                       const float* cmd_bounds, const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target,
                       const vgx_raster_damage* damage, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx) { return VGX_E_INVALID_ARG; }
	int st = vgx_rasterc_check_args(streams, cmds, num_cmds, dev_num_cmds, images, num_images, paints, target, dev_status);
	if (st != VGX_OK) { return st; }
	if (damage && (vgx_damage_record_check(damage) != VGX_OK || ((uintptr_t)cmd_bounds & 15u))) { return VGX_E_INVALID_ARG; }
	const vgx_raster_target& t = *target;
	hipStream_t s = (hipStream_t)stream;
	if (rasterNothingToWrite(ctx, t, dev_status, s)) { return launchStatus(ctx); }
	VgxRasterCmdArgs a;
	memset(&a, 0, sizeof(a));
	rasterTarget(a, t);
	HostMirror<unsigned long long>& mirror = damage ? ctx->rascDmg : ctx->rasc;
	if ((st = mirror.create(ctx, VGX_RASC_WORDS)) != VGX_OK) { return st; }
	// the tables: what they hold, at least the first guess of one chunk per command and per 64 triangles of the index stream and as
	// many entries, and what the last call measured once that has arrived. The chunks of a damaged call follow the same protocol from
	// its own mirror; its entries are its window's, below
	uint64_t chunks = (uint64_t)num_cmds + streams->num_indices / (3u * VGX_RASTERC_CHUNK), entries = chunks;
	if (mirror.landed()) {
		const unsigned long long last = mirror.host[VGX_RASC_STATUS];
		if (last == VGX_E_GROWN && mirror.host[VGX_RASC_CHUNKS] > chunks) { chunks = mirror.host[VGX_RASC_CHUNKS]; }
		if (!damage && last == VGX_E_GROWN && mirror.host[VGX_RASC_ENTRIES] > entries) { entries = mirror.host[VGX_RASC_ENTRIES]; }
		if (damage) { vgx_damage_learn(&ctx->rascDmgWindow, last, mirror.host[VGX_RASC_ENTRIES]); }
	}
	if (chunks > 0xFFFFFFFFull) { chunks = 0xFFFFFFFFull; }
	if (entries > 0xFFFFFFFFull) { entries = 0xFFFFFFFFull; }
	if ((st = rasterCmdsEnsure(ctx, num_cmds, chunks, entries)) != VGX_OK) { return st; }
	a.chunk_cap = ctx->rascChunkCap < 0xFFFFFFFFull ? ctx->rascChunkCap : 0xFFFFFFFFull;
	// no chunk has more entries than the scissor has tiles: the sort need not look further
	const uint64_t bound = a.chunk_cap * ((uint64_t)a.tiles_x * a.tiles_y);
	uint64_t window = ~0ull;
	if (damage) {
		// The window, as in rasterCall. These tables keep a capacity apart from their size (rascEntryCap), so max_entries is clipped
		// to that, and the first guess grew them above already: only a window past the capacity grows them again
		window = vgx_damage_window(ctx->rascDmgWindow, damage->max_entries, ctx->rascEntryCap, bound);
		if (window > ctx->rascEntryCap && (st = rasterCmdsEnsure(ctx, num_cmds, chunks, window)) != VGX_OK) { return st; }
	}
	a.entry_cap = ctx->rascEntryCap < 0xFFFFFFFFull ? ctx->rascEntryCap : 0xFFFFFFFFull;
	if (window < a.entry_cap) { a.entry_cap = window; }
	a.sort_n = num_cmds ? (bound < a.entry_cap ? bound : a.entry_cap) : 0;
	size_t sortBytes;
	if ((st = rasterSortStorage(ctx, a, &sortBytes)) != VGX_OK) { return st; }
	const uint64_t words = ((uint64_t)a.sentinel + 31u) / 32u;
	if ((st = ensure(ctx, ctx->rascTilePaint, words + 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->rascTilePaint.p, 0, words * sizeof(uint32_t), s));
	a.pos = streams->pos; a.color = streams->color; a.uv = streams->uv; a.idx = streams->idx;
	a.num_vertices = streams->num_vertices; a.num_indices = streams->num_indices; a.uv_bytes = streams->uv_bytes;
	a.cmds = cmds; a.num_cmds = num_cmds; a.dev_num_cmds = dev_num_cmds;
	a.images = images; a.num_images = num_images;
	if (paints) { a.gradients = paints->gradients; a.patterns = paints->patterns; a.num_gradients = paints->num_gradients; a.num_patterns = paints->num_patterns; }
	a.cmd_state = ctx->rascCmdState.ptr(); a.cmd_first = ctx->rascCmdFirst.ptr();
	a.chunk_rect = ctx->rascChunkRect.ptr(); a.chunk_cmd = ctx->rascChunkCmd.ptr(); a.chunk_first = ctx->rascChunkFirst.ptr();
	a.keys = ctx->rascKeys.ptr(); a.vals = ctx->rascVals.ptr(); a.sorted_keys = ctx->rascSortedKeys.ptr(); a.sorted_vals = ctx->rascSortedVals.ptr();
	a.tile_paint = ctx->rascTilePaint.ptr();
	a.state = ctx->rascState.ptr(); a.status = dev_status;
	if (damage) { a.damage = damage->tile_bits; a.cmd_bounds = cmd_bounds; a.width = t.width; a.height = t.height; }
	noteHip(ctx, vgx_launch_raster_commands(a, ctx->rasPartial.p, ctx->rasSortTemp.p, sortBytes, s));
	// status and need to the mirror, for the next call (never waited for)
	mirror.push(ctx, a.state, s);
	return launchStatus(ctx);
}

} // namespace

int vgx_raster_commands(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                        const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target,
                        uint32_t* dev_status, void* stream)
{
	return rasterCommandsCall(ctx, streams, cmds, num_cmds, dev_num_cmds, nullptr, images, num_images, paints, target, nullptr, dev_status, stream);
}

int vgx_raster_commands_damaged(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* dev_num_cmds,
                                const float* cmd_bounds, const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints,
                                const vgx_raster_target* target, const vgx_raster_damage* damage, uint32_t* dev_status, void* stream)
{
	if (!damage) { return VGX_E_INVALID_ARG; }
	return rasterCommandsCall(ctx, streams, cmds, num_cmds, dev_num_cmds, cmd_bounds, images, num_images, paints, target, damage, dev_status, stream);
}

int vgx_raster_cmds_from_assembly(vgx_ctx* ctx, const vgx_drawcmd* drawcmds, uint64_t cap_drawcmds, const uint64_t* dev_num_drawcmds, const vgx_mesh* meshes,
                                  uint64_t num_meshes, const vgx_raster_draws* state, vgx_raster_cmd* out, uint32_t* dev_num_cmds, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !state || !dev_num_cmds || (cap_drawcmds && (!drawcmds || !out)) || (num_meshes && !meshes)) { return VGX_E_INVALID_ARG; }
	if (state->reserved != 0u || (state->num_draws && !state->draw_state)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)drawcmds & 7u) || ((uintptr_t)dev_num_drawcmds & 7u) || ((uintptr_t)meshes & 7u) || ((uintptr_t)out & 7u) || ((uintptr_t)state->draw_state & 3u)
		|| ((uintptr_t)dev_num_cmds & 3u) || ((uintptr_t)dev_status & 3u)) {
		return VGX_E_INVALID_ARG;
	}
	if (cap_drawcmds > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	int st;
	if ((st = ensure(ctx, ctx->rascFlag, 4)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->rascFlag.p, 0, sizeof(uint32_t), s));
	VgxCmdsFromAsmArgs a;
	memset(&a, 0, sizeof(a));
	a.drawcmds = drawcmds; a.cap_drawcmds = cap_drawcmds; a.dev_num_drawcmds = dev_num_drawcmds; a.meshes = meshes; a.num_meshes = num_meshes;
	a.draw_state = state->draw_state; a.num_draws = state->num_draws; a.out = out; a.dev_num_cmds = dev_num_cmds; a.flag = ctx->rascFlag.ptr(); a.status = dev_status;
	vgx_launch_cmds_from_assembly(a, s);
	return launchStatus(ctx);
}

// HOST only, no context (vgx_raster_cmds.h)
int vgx_submit_order(const vgx_raster_cmd* draw_cmds, uint32_t ndraw, const vgx_raster_cmd* clip_cmds, uint32_t nclip, vgx_raster_cmd* out, uint32_t cap,
                     uint32_t* num_out)
{
	return vgx_rasterc_submit_order(draw_cmds, ndraw, clip_cmds, nclip, out, cap, num_out);
}

// HOST only, no context: the decoder's paint list scattered by handle into the two tables vgx_raster_painted indexes; holes marked
int vgx_paint_tables(const vgx_paint* paints, uint32_t n, vgx_paint* gradients, uint32_t cap_gradients, vgx_paint* patterns, uint32_t cap_patterns)
{
	if ((n && !paints) || (cap_gradients && !gradients) || (cap_patterns && !patterns)) { return VGX_E_INVALID_ARG; }
	for (uint32_t k = 0; k < cap_gradients; ++k) { memset(&gradients[k], 0, sizeof(vgx_paint)); gradients[k].type = 0xFFFFFFFFu; }
	for (uint32_t k = 0; k < cap_patterns; ++k) { memset(&patterns[k], 0, sizeof(vgx_paint)); patterns[k].type = 0xFFFFFFFFu; }
	for (uint32_t k = 0; k < n; ++k) {
		const vgx_paint& p = paints[k];
		if (p.type != 1u && p.type != 2u) { return VGX_E_INVALID_ARG; }
		if (p.handle >= (p.type == 1u ? cap_gradients : cap_patterns)) { return VGX_E_NOSPACE; }
		(p.type == 1u ? gradients : patterns)[p.handle] = p;
	}
	return VGX_OK;
}

// ---- incremental update of a submitted frame (vgx_update.hip) -------------------------------------------------------------
// Scratch of their own, like the culling and picking calls: count -> vgx_cache_layout / vgx_cache_update -> emit still works.
int vgx_cache_layout(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst, vgx_cache_slot* slots,
                     uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !cache || !slots || (ninst && !inst) || (cache->num_meshes && !cache->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)inst & 7u) || ((uintptr_t)slots & 7u) || ((uintptr_t)cache->meshes & 7u) || ((uintptr_t)dev_status & 3u)) { return VGX_E_INVALID_ARG; }
	if (ninst > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	int st;
	if ((st = ensure(ctx, ctx->updPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if (dev_status) { noteHip(ctx, hipMemsetAsync(dev_status, 0, sizeof(uint32_t), s)); } // VGX_OK
	vgx_launch_cache_layout(*cache, inst, ninst, slots, dev_status, ctx->updPartial.p, s);
	return launchStatus(ctx);
}

int vgx_cache_update(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst, const vgx_cache_slot* slots,
                     const uint32_t* dirty, uint64_t ndirty, const uint64_t* dev_ndirty, const vgx_update_frame* frame, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !cache || !frame || (ndirty && (!dirty || !slots || !frame->pos || !frame->color)) || (ndirty && ninst && !inst)) { return VGX_E_INVALID_ARG; }
	if (ndirty && cache->num_meshes && (!cache->pos || !cache->meshes)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)inst & 7u) || ((uintptr_t)slots & 7u) || ((uintptr_t)dirty & 3u) || ((uintptr_t)dev_ndirty & 7u) || ((uintptr_t)frame->pos & 7u)
		|| ((uintptr_t)frame->color & 3u) || ((uintptr_t)frame->mesh_bounds & 15u) || ((uintptr_t)dev_status & 3u) || ((uintptr_t)cache->pos & 7u)
		|| ((uintptr_t)cache->meshes & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (ninst > 0xFFFFFFFFull || ndirty > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	int st;
	// [flag word, padded to 16 bytes][vertex prefix: ndirty + 1][mesh prefix: ndirty + 1]
	if ((st = ensure(ctx, ctx->updPrefix, 16 + 2 * (ndirty + 1) * sizeof(uint64_t))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->updPartial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->updPrefix.p, 0, 16, s));
	VgxUpdateArgs a;
	memset(&a, 0, sizeof(a));
	a.cache = *cache; a.inst = inst; a.ninst = ninst; a.slots = slots; a.dirty = dirty; a.ndirty = ndirty; a.dev_ndirty = dev_ndirty;
	a.pos = frame->pos; a.color = frame->color; a.frame_vertices = frame->num_vertices; a.frame_meshes = frame->num_meshes;
	a.mesh_bounds = frame->mesh_bounds;
	a.flags = (uint32_t*)ctx->updPrefix.p;
	a.vert_prefix = (uint64_t*)((char*)ctx->updPrefix.p + 16); a.mesh_prefix = a.vert_prefix + (ndirty + 1);
	a.status = dev_status;
	vgx_launch_cache_update(a, ctx->updPartial.p, s);
	return launchStatus(ctx);
}

int vgx_merge(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const vgx_draw* draws, uint64_t ndraws,
              const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	return vgx_merge_uv(ctx, a, b, b_draw, nullptr, draws, ndraws, out, dev_sizes, dev_status, stream);
}

namespace {

// vgx_merge_uv (out_uv == nullptr: b_uv goes into the armed assembly's UV stream) and vgx_merge_uv_stream (b_uv goes to out_uv, and the
// assembly's UV stream is left alone): one body
int mergeCall(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const void* b_uv, void* out_uv, uint32_t uv_bytes,
              const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	(void)ndraws;
	if (!ctx || !a || !b || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out)
		|| (a->num_meshes && (!a->pos || !a->color || !a->idx || !a->meshes)) || (b->num_meshes && (!b->pos || !b->color || !b->idx || !b->meshes))) {
		return VGX_E_INVALID_ARG;
	}
	const uint64_t n = a->num_meshes + b->num_meshes;
	if (n >= 0x7FFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	tmplDrop(ctx); // the mesh-table scratch is re-sized below
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mtab, n + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mdesc, n + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->cmdPrefix, (n + 1) * sizeof(uint64_t))) != VGX_OK) { return st; } // the merged order lives in the command-prefix scratch
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	VgxMergeArgs m;
	memset(&m, 0, sizeof(m));
	m.a = *a; m.b = *b; m.b_draw = b_draw;
	m.order = (uint32_t*)ctx->cmdPrefix.p; m.mtab = ctx->mtab.ptr(); m.mdesc = ctx->mdesc.ptr();
	m.meshes_out = out->meshes; m.pos = out->pos; m.color = out->color; m.idx = out->idx; m.mesh_base = nullptr;
	m.totals = ctx->totals.ptr();
	m.caps = ctx->caps; m.caps.vertices = out->cap_vertices; m.caps.indices = out->cap_indices; m.caps.meshes = out->cap_meshes;
	vgx_launch_merge_rank(m, s);
	vgx_launch_merge_scan(m, ctx->partial.p, s);
	mark(ctx, s, "merge_scan");
	if (ctx->asmArmed) {
		void* const asmUv = ctx->asmCfg.uv;
		if (out_uv) { ctx->asmCfg.uv = nullptr; } // the assembly step writes no UV stream of its own
		st = runAssemble(ctx, out, s, draws);
		ctx->asmCfg.uv = asmUv;
		if (st != VGX_OK) { return st; }
		m.mesh_base = ctx->meshBase.ptr();
		if (!out_uv && b_uv && ctx->asmCfg.uv && ctx->asmCfg.uv_bytes) { m.b_uv = b_uv; m.uv_out = ctx->asmCfg.uv; m.uv_bytes = ctx->asmCfg.uv_bytes; }
	}
	if (out_uv) { m.b_uv = b_uv; m.uv_out = out_uv; m.uv_bytes = uv_bytes; }
	vgx_launch_merge_copy(m, s);
	mark(ctx, s, "merge_copy");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

} // namespace

int vgx_merge_uv(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const void* b_uv, const vgx_draw* draws, uint64_t ndraws,
                 const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	return mergeCall(ctx, a, b, b_draw, b_uv, nullptr, 0u, draws, ndraws, out, dev_sizes, dev_status, stream);
}

int vgx_merge_uv_stream(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const void* b_uv, uint32_t uv_bytes,
                        const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* out_uv, vgx_sizes* dev_sizes, uint32_t* dev_status,
                        void* stream)
{
	if (!b_uv || !out_uv || (uv_bytes != 4u && uv_bytes != 8u) || ((uintptr_t)b_uv & 3u) || ((uintptr_t)out_uv & 3u)) { return VGX_E_INVALID_ARG; }
	return mergeCall(ctx, a, b, b_draw, b_uv, out_uv, uv_bytes, draws, ndraws, out, dev_sizes, dev_status, stream);
}

int vgx_set_assembly(vgx_ctx* ctx, const vgx_assembly* asm_)
{
	if (!ctx) {
		return VGX_E_INVALID_ARG;
	}
	if (!asm_) {
		ctx->asmArmed = false;
		return VGX_OK;
	}
	if (!asm_->drawcmds || asm_->cap_drawcmds == 0 || asm_->max_vb_vertices > 65536u) { // vg.cpp:734: indices are uint16
		return VGX_E_INVALID_ARG;
	}
	if ((asm_->flags & ~(uint32_t)VGX_ASM_SPLIT_STATE) || (asm_->uv && asm_->uv_bytes != 4 && asm_->uv_bytes != 8)) {
		return VGX_E_INVALID_ARG;
	}
	ctx->asmCfg = *asm_;
	ctx->asmArmed = true;
	return VGX_OK;
}

// ---- concave fills ------------------------------------------------------------------------------------
int vgx_concave_move(vgx_ctx* ctx, const float* contour_verts, uint64_t num_contour_vertices, const vgx_contour* contours, uint64_t ncontours,
                     const vgx_concave_fill* fills, uint64_t nfills, float* moved, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || (num_contour_vertices && (!contour_verts || !contours || !fills || !moved || !ncontours || !nfills))) {
		return VGX_E_INVALID_ARG;
	}
	if (!num_contour_vertices) { return VGX_OK; }
	VgxConcaveArgs a;
	memset(&a, 0, sizeof(a));
	a.contour_verts = contour_verts; a.contours = contours; a.ncontours = ncontours; a.num_contour_vertices = num_contour_vertices;
	a.fills = fills; a.nfills = nfills; a.moved = moved;
	vgx_launch_concave_move(a, (hipStream_t)stream);
	return launchStatus(ctx);
}

int vgx_concave_emit(vgx_ctx* ctx, const float* contour_verts, uint64_t num_contour_vertices, const vgx_contour* contours, uint64_t ncontours,
                     const vgx_concave_fill* fills, uint64_t nfills, const float* tess_pos, const uint16_t* tess_idx,
                     const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out) || (nfills && !fills) || (ncontours && (!contours || !contour_verts))) {
		return VGX_E_INVALID_ARG;
	}
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->mtab, nfills + 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	OpConcaveFills op;
	op.contours = contours; op.ncontours = ncontours; op.fills = fills; op.nfills = nfills;
	op.mtab = ctx->mtab.ptr(); op.meshesOut = out->meshes; op.totals = ctx->totals.ptr();
	op.caps = ctx->caps;
	op.caps.vertices = out->cap_vertices; op.caps.indices = out->cap_indices; op.caps.meshes = out->meshes ? out->cap_meshes : ~0ull;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, nfills);
	mark(ctx, s, "scan_concave_fills");
	VgxConcaveArgs a;
	memset(&a, 0, sizeof(a));
	a.contour_verts = contour_verts; a.contours = contours; a.ncontours = ncontours; a.num_contour_vertices = num_contour_vertices;
	a.fills = fills; a.nfills = nfills; a.tess_pos = tess_pos; a.tess_idx = tess_idx;
	a.mtab = ctx->mtab.ptr(); a.pos = out->pos; a.color = out->color; a.idx = out->idx;
	a.totals = ctx->totals.ptr();
	vgx_launch_concave_emit(a, s);
	mark(ctx, s, "concave_emit");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

int vgx_concave_contours(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                         const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out) || (ndraws && (!poly || !subpaths || !draw_info || !draws))) {
		return VGX_E_INVALID_ARG;
	}
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->contourPrefix, 2 * (ndraws + 1))) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	OpContourDraws op;
	op.subs = subpaths; op.dinfo = draw_info; op.draws = draws; op.ndraws = ndraws;
	op.contourPrefix = ctx->contourPrefix.ptr(); op.vertexPrefix = ctx->contourPrefix.ptr() + ndraws + 1;
	op.meshesOut = out->meshes; op.totals = ctx->totals.ptr();
	op.caps = ctx->caps;
	op.caps.vertices = out->cap_vertices; op.caps.indices = out->cap_indices; op.caps.meshes = out->meshes ? out->cap_meshes : ~0ull;
	vgx_device_scan(op, (Sum3*)ctx->partial.p, s, ndraws);
	mark(ctx, s, "scan_contour_draws");
	if (ndraws) {
		VgxContoursArgs a;
		memset(&a, 0, sizeof(a));
		a.poly = poly; a.subpaths = subpaths; a.draw_info = draw_info; a.draws = draws; a.ndraws = ndraws;
		a.contour_prefix = op.contourPrefix; a.vertex_prefix = op.vertexPrefix;
		a.pos = out->pos; a.color = out->color; a.idx = out->idx; a.totals = ctx->totals.ptr();
		vgx_launch_concave_contours(a, s);
		mark(ctx, s, "concave_contours");
	}
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

// vgx_concave_triangulate, vgx_concave_triangulate_rings and vgx_concave_triangulate_nested are one body: `entry` chooses the kernels, the
// bound of the triangle scratch and (nested alone) a word per draw for its group count
enum TriEntry { TRI_ENTRY_RING, TRI_ENTRY_RINGS, TRI_ENTRY_NESTED };
static int concaveTriangulate(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                              const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream, TriEntry entry)
{
	const bool rings = entry != TRI_ENTRY_RING;
	DeviceGuard guard(ctx);
	if (!ctx || !out || !out->pos || !out->color || !out->idx || meshOutMisaligned(out) || (ndraws && (!poly || !subpaths || !draw_info || !draws))) {
		return VGX_E_INVALID_ARG;
	}
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u) || ((uintptr_t)draw_route & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	// a ring's triangles wait in scratch for their place: three indices per ring vertex, and rings that cannot all fit into the caller's
	// vertices (the call then ends with VGX_E_NOSPACE) keep none. A ring that is clipped has at most VGX_TRIANGULATE_MAX_VERTICES: a large
	// output buffer behind a few draws costs no more scratch than those draws can fill
	const uint64_t ringBound = ndraws * (uint64_t)VGX_TRIANGULATE_MAX_VERTICES;
	// With holes a draw of V vertices waits in V + 2 H slots, and H < V / 3 (a ring has three vertices at least): below 5 V / 3
	const uint64_t slotBound = rings ? out->cap_vertices + 2 * (out->cap_vertices / 3) : out->cap_vertices;
	const uint64_t capTri = 3 * (slotBound < ringBound ? slotBound : ringBound);
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->partial, VGX_SCAN_BLOCKS * sizeof(Sum3))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->triRoute, ndraws + 1)) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->triPrefix, 4 * (ndraws + 1))) != VGX_OK) { return st; }
	if ((st = ensure(ctx, ctx->triIdx, capTri + 1)) != VGX_OK) { return st; }
	if (entry == TRI_ENTRY_NESTED && (st = ensure(ctx, ctx->triGroups, ndraws + 1)) != VGX_OK) { return st; }
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	VgxTriArgs a;
	memset(&a, 0, sizeof(a));
	a.poly = poly; a.subpaths = subpaths; a.draw_info = draw_info; a.draws = draws; a.ndraws = ndraws;
	a.route = ctx->triRoute.ptr(); a.draw_route = draw_route;
	a.ring_vertices = ctx->triPrefix.ptr(); a.cand_prefix = a.ring_vertices + (ndraws + 1);
	a.vertex_prefix = a.cand_prefix + (ndraws + 1); a.index_prefix = a.vertex_prefix + (ndraws + 1);
	a.tri = ctx->triIdx.ptr(); a.cap_tri = capTri;
	a.pos = out->pos; a.color = out->color; a.idx = out->idx; a.meshes = out->meshes;
	a.cap_vertices = out->cap_vertices; a.cap_indices = out->cap_indices; a.cap_meshes = out->meshes ? out->cap_meshes : ~0ull;
	a.totals = ctx->totals.ptr();
	if (entry == TRI_ENTRY_NESTED) { vgx_launch_concave_triangulate_nested(a, ctx->triGroups.ptr(), ctx->partial.p, s); }
	else if (rings) { vgx_launch_concave_triangulate_rings(a, ctx->partial.p, s); } else { vgx_launch_concave_triangulate(a, ctx->partial.p, s); }
	mark(ctx, s, entry == TRI_ENTRY_NESTED ? "concave_triangulate_nested" : rings ? "concave_triangulate_rings" : "concave_triangulate");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

int vgx_concave_triangulate(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                            const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	return concaveTriangulate(ctx, poly, subpaths, draw_info, draws, ndraws, out, draw_route, dev_sizes, dev_status, stream, TRI_ENTRY_RING);
}

int vgx_concave_triangulate_rings(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                  const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	return concaveTriangulate(ctx, poly, subpaths, draw_info, draws, ndraws, out, draw_route, dev_sizes, dev_status, stream, TRI_ENTRY_RINGS);
}

int vgx_concave_triangulate_nested(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                   const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	return concaveTriangulate(ctx, poly, subpaths, draw_info, draws, ndraws, out, draw_route, dev_sizes, dev_status, stream, TRI_ENTRY_NESTED);
}

// ---- text runs ----------------------------------------------------------------------------------------
int vgx_text_quads(vgx_ctx* ctx, const float* quads, uint64_t nquads, const vgx_text_run* runs, uint64_t nruns, uint64_t first_mesh,
                   const vgx_mesh_out* out, void* out_uv, uint32_t uv_bytes, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out || !out->pos || !out->color || !out->idx || (nquads && !quads) || (nruns && !runs)
		|| (out_uv && uv_bytes != 4 && uv_bytes != 8) || (!out_uv && uv_bytes != 0 && uv_bytes != 4 && uv_bytes != 8)) {
		return VGX_E_INVALID_ARG;
	}
	// the streams are written in units of their elements, the quads are read as 16-byte pairs
	if (((uintptr_t)quads & 15u) || meshOutMisaligned(out)
		|| (out_uv && ((uintptr_t)out_uv & (uintptr_t)(uv_bytes - 1u))) || ((uintptr_t)runs & 7u)) {
		return VGX_E_INVALID_ARG;
	}
	if (nquads > 0x7FFFFFFFull || nruns > 0x7FFFFFFFull) { return VGX_E_RANGE; }
	hipStream_t s = (hipStream_t)stream;
	markBegin(ctx, s);
	ctx->counted.stage = VGX_COUNTED_NONE;
	int st;
	if ((st = ensure(ctx, ctx->totals, 1)) != VGX_OK) { return st; }
	VgxTextArgs a;
	memset(&a, 0, sizeof(a));
	a.quads = quads; a.nquads = nquads; a.runs = runs; a.nruns = nruns; a.first_mesh = first_mesh;
	a.pos = out->pos; a.color = out->color; a.idx = out->idx; a.meshes = out->meshes;
	a.uv = uv_bytes ? out_uv : nullptr; a.uv_bytes = uv_bytes;
	a.cap_vertices = out->cap_vertices; a.cap_indices = out->cap_indices; a.cap_meshes = out->cap_meshes;
	a.totals = ctx->totals.ptr();
	if (nruns > 4096 || nquads > 65536) { // beyond a frame's size: the run kernel writes the first run of every tile of 256 quads
		if ((st = ensure(ctx, ctx->textTiles, nquads / 256 + 1)) != VGX_OK) { return st; }
		a.tile_run = ctx->textTiles.ptr();
	}
	noteHip(ctx, hipMemsetAsync(ctx->totals.p, 0, sizeof(VgxTotals), s));
	vgx_launch_text_quads(a, s);
	mark(ctx, s, "text_quads");
	publish(ctx, dev_sizes, dev_status, s);
	return launchStatus(ctx);
}

int vgx_get_failure_info(vgx_ctx* ctx, vgx_failure_info* out, void* stream)
{
	if (!ctx || !out) {
		return VGX_E_INVALID_ARG;
	}
	DeviceGuard guard(ctx);
	memset(out, 0, sizeof(*out));
	if (!ctx->totals.p) {
		return VGX_OK;
	}
	const int st = readTotals(ctx, (hipStream_t)stream);
	if (st != VGX_OK) { return st; }
	out->status = ctx->hostTotals->status;
	out->reason = ctx->hostTotals->fail_reason;
	out->aux = ctx->hostTotals->fail_aux;
	out->segment = ctx->hostTotals->fail_segment;
	const VgxRoute& r = ctx->route.chosen;
	out->segment_items = ctx->tmpl.on ? 5u : ctx->opt.inst ? (r.period ? (r.permute ? 4u : 1u) : (r.kind == VGX_ROUTE_GROUPED ? (r.classes > 1 ? 3u : 2u) : 0u)) : 0u; // flatten mode chosen by the last count call
	if (out->segment_items == 0u && ctx->counted.ps && ctx->counted.ps->thinStatic && ctx->opt.thinStatic) { out->segment_items = 6u; } // k_flatten_thin in k_flatten_build's place
	for (int i = 0; i < 16; ++i) { out->prof[i] = ctx->hostTotals->prof[i]; }
	return VGX_OK;
}

int vgx_set_static_batches(vgx_ctx* ctx, int enable)
{
	if (!ctx) {
		return VGX_E_INVALID_ARG;
	}
	ctx->opt.tmplBatch = enable ? 1 : 0;
	if (!enable && ctx->tmpl.isBatch) { tmplDrop(ctx); } // the next vgx_tessellate wants a count again
	return VGX_OK;
}

int vgx_set_profiling(vgx_ctx* ctx, int enable)
{
	if (!ctx) {
		return VGX_E_INVALID_ARG;
	}
	ctx->profiling = enable ? 1 : 0;
	ctx->profCalls = 0;
	return VGX_OK;
}

int vgx_get_stage_times(vgx_ctx* ctx, vgx_stage_times* out)
{
	return vgx_get_stage_times_avg(ctx, out, 1);
}

int vgx_get_stage_times_avg(vgx_ctx* ctx, vgx_stage_times* out, uint32_t ncalls)
{
	DeviceGuard guard(ctx);
	if (!ctx || !out) {
		return VGX_E_INVALID_ARG;
	}
	memset(out, 0, sizeof(*out));
	if (!ctx->profiling || !ctx->evCreated || ctx->profCalls == 0) {
		return VGX_OK;
	}
	uint64_t n = ncalls < 1 ? 1 : ncalls;
	if (n > VGX_PROF_RING) { n = VGX_PROF_RING; }
	if (n > ctx->profCalls) { n = ctx->profCalls; }
	const uint32_t last = (uint32_t)((ctx->profCalls - 1) % VGX_PROF_RING);
	out->num_stages = ctx->numEv[last];
	uint32_t used = 0;
	for (uint64_t c = 0; c < n; ++c) {
		const uint32_t k = (uint32_t)((ctx->profCalls - 1 - c) % VGX_PROF_RING);
		if (ctx->numEv[k] != ctx->numEv[last]) { continue; } // a call of another kind in between: not averaged in
		bool same = true;
		for (uint32_t i = 0; i < ctx->numEv[k]; ++i) { same = same && ctx->evName[k][i] == ctx->evName[last][i]; }
		if (!same) { continue; }
		for (uint32_t i = 0; i < ctx->numEv[k]; ++i) {
			float ms = 0.0f;
			if (hipEventElapsedTime(&ms, ctx->ev[k][i], ctx->ev[k][i + 1]) != hipSuccess) { ms = -1.0f; }
			out->ms[i] += ms;
		}
		++used;
	}
	for (uint32_t i = 0; i < out->num_stages; ++i) {
		out->ms[i] = used ? out->ms[i] / (float)used : -1.0f;
		out->name[i] = ctx->evName[last][i];
	}
	return VGX_OK;
}

} // extern "C"

// ---- multi-GPU gather over RCCL (the layout of vg-renderer_amd/dist.py behind the C-ABI) ------------------
// librccl is bound with dlopen / dlsym from the copy the process already has (a C++ host links it; a torch process
// carries its own), never linked: libvgx.so loads on boxes without it and cannot pull a second copy into a process.
#include <dlfcn.h>

struct VgxRccl
{
	void* lib;
	int (*GroupStart)();
	int (*GroupEnd)();
	int (*Send)(const void*, size_t, int, int, void*, hipStream_t);
	int (*Recv)(void*, size_t, int, int, void*, hipStream_t);
	int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t);
	int (*CommCount)(void*, int*);
	int (*CommUserRank)(void*, int*);
};
enum { kNcclUint8 = 1, kNcclUint64 = 5 }; // ncclDataType_t values (rccl.h)

static void vgx_rccl_release(vgx_ctx* ctx)
{
	if (ctx->rccl) {
		if (ctx->rccl->lib) { (void)dlclose(ctx->rccl->lib); }
		delete ctx->rccl;
		ctx->rccl = nullptr;
	}
}

namespace {

int bindRccl(vgx_ctx* ctx)
{
	if (ctx->rccl) {
		return VGX_OK;
	}
	void* h = nullptr;
	if (const char* over = getenv("VGX_RCCL_LIB")) { h = dlopen(over, RTLD_NOW | RTLD_LOCAL); } // testing knob: tests/native/fake_rccl.cpp
	const char* names[] = { "librccl.so.1", "librccl.so" };
	for (const char* n : names) { if (!h) { h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); } } // the copy the process already uses
	for (const char* n : names) { if (!h) { h = dlopen(n, RTLD_NOW | RTLD_LOCAL); } }
	if (!h) { h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL); }
	if (!h) {
		return VGX_E_NO_DEVICE;
	}
	VgxRccl* r = new VgxRccl;
	r->lib = h;
	r->GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
	r->GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
	r->Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
	r->Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
	r->AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
	r->CommCount = (int (*)(void*, int*))dlsym(h, "ncclCommCount");
	r->CommUserRank = (int (*)(void*, int*))dlsym(h, "ncclCommUserRank");
	if (!r->GroupStart || !r->GroupEnd || !r->Send || !r->Recv || !r->AllGather || !r->CommCount || !r->CommUserRank) {
		(void)dlclose(h);
		delete r;
		return VGX_E_NO_DEVICE;
	}
	ctx->rccl = r;
	return VGX_OK;
}

#define RCCLCHK(ctx, call)                                    \
	do {                                                      \
		const int r_ = (call);                                \
		if (r_ != 0) {                                        \
			(ctx)->lastHipError = 10000 + r_;                 \
			return VGX_E_HIP;                                 \
		}                                                     \
	} while (0)

// mesh records of rank r sit at [mesh0, mesh1): add the rank's vertex / index / draw bases
struct GatherRebase { uint64_t mesh0, mesh1, vbase, ibase; uint32_t dbase; };
#define VGX_GATHER_MAX_RANKS 64
struct GatherRebaseArgs { vgx_mesh* meshes; int n; GatherRebase r[VGX_GATHER_MAX_RANKS]; };

__global__ __launch_bounds__(256) void k_gather_rebase(GatherRebaseArgs A)
{
	const GatherRebase R = A.r[blockIdx.y];
	for (uint64_t m = R.mesh0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < R.mesh1; m += (uint64_t)gridDim.x * blockDim.x) {
		vgx_mesh rec = A.meshes[m];
		rec.first_vertex += R.vbase;
		rec.first_index += R.ibase;
		rec.draw += R.dbase;
		A.meshes[m] = rec;
	}
}

} // namespace

// Transfers larger than this leave in several pieces: piece c of every (rank, stream) pair goes out in group c, so that no
// single RCCL operation is gigabytes long and the proxy threads can pipeline (VGX_GATHER_CHUNK_MB, default 256 MiB).
static size_t gatherChunkBytes()
{
	static size_t v = 0;
	if (!v) {
		const char* e = getenv("VGX_GATHER_CHUNK_MB");
		const long mb = e ? atol(e) : 256;
		v = (size_t)(mb >= 1 ? mb : 256) << 20;
	}
	return v;
}

extern "C" int vgx_gather_sizes(vgx_ctx* ctx, void* rccl_comm, const vgx_rank_sizes* mine, vgx_rank_sizes* all, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !rccl_comm || !mine || !all) {
		return VGX_E_INVALID_ARG;
	}
	int st = bindRccl(ctx);
	if (st != VGX_OK) { return st; }
	int nranks = 0, rank = 0;
	RCCLCHK(ctx, ctx->rccl->CommCount(rccl_comm, &nranks));
	RCCLCHK(ctx, ctx->rccl->CommUserRank(rccl_comm, &rank));
	if (nranks < 1 || rank < 0 || rank >= nranks) { return VGX_E_INVALID_ARG; }
	// five words per rank: the four totals + the rank's transfer piece size. The piece size is part of the wire protocol of
	// vgx_gather_at (sender and root must cut a stream into the same pieces) but comes from each process's own environment
	// (VGX_GATHER_CHUNK_MB): ranks that disagree are told here, before a gather could hang on mismatched Send / Recv sizes.
	if ((st = ensure(ctx, ctx->gatherSizes, (size_t)nranks)) != VGX_OK) { return st; }
	hipStream_t s = (hipStream_t)stream;
	VgxGatherWire* dev = ctx->gatherSizes.ptr();
	std::vector<VgxGatherWire> host((size_t)nranks);
	host[(size_t)rank].z = *mine; host[(size_t)rank].chunk = gatherChunkBytes();
	HIPCHK(ctx, hipMemcpyAsync(dev + rank, &host[(size_t)rank], sizeof(VgxGatherWire), hipMemcpyHostToDevice, s));
	RCCLCHK(ctx, ctx->rccl->AllGather(dev + rank, dev, 5, kNcclUint64, rccl_comm, s)); // in place: my slot is my send buffer
	HIPCHK(ctx, hipMemcpyAsync(host.data(), dev, (size_t)nranks * sizeof(VgxGatherWire), hipMemcpyDeviceToHost, s));
	HIPCHK(ctx, hipStreamSynchronize(s));
	for (int r = 0; r < nranks; ++r) {
		all[r] = host[(size_t)r].z;
		if (host[(size_t)r].chunk != gatherChunkBytes()) { return VGX_E_INVALID_ARG; }
	}
	return VGX_OK;
}

extern "C" int vgx_gather_at(vgx_ctx* ctx, void* rccl_comm, int root, const vgx_mesh_out* local, const vgx_rank_sizes* all, const vgx_rank_sizes* place,
	const vgx_mesh_out* global, void* stream)
{
	DeviceGuard guard(ctx);
	if (!ctx || !rccl_comm || !local || !all || !place) {
		return VGX_E_INVALID_ARG;
	}
	int st = bindRccl(ctx);
	if (st != VGX_OK) { return st; }
	int nranks = 0, rank = 0;
	RCCLCHK(ctx, ctx->rccl->CommCount(rccl_comm, &nranks));
	RCCLCHK(ctx, ctx->rccl->CommUserRank(rccl_comm, &rank));
	if (nranks < 1 || nranks > VGX_GATHER_MAX_RANKS || root < 0 || root >= nranks) { return VGX_E_INVALID_ARG; }
	hipStream_t s = (hipStream_t)stream;
	const vgx_rank_sizes& me = all[rank];
	if (me.num_vertices > local->cap_vertices || me.num_indices > local->cap_indices || (local->meshes && me.num_meshes > local->cap_meshes)) {
		return VGX_E_INVALID_ARG; // the sizes do not describe `local`
	}
	if ((me.num_vertices && (!local->pos || !local->color)) || (me.num_indices && !local->idx) || (me.num_meshes && !local->meshes)) {
		return VGX_E_INVALID_ARG;
	}
	if (rank == root) {
		if (!global || !global->pos || !global->color || !global->idx || !global->meshes) { return VGX_E_INVALID_ARG; }
		for (int r = 0; r < nranks; ++r) { // every block inside the destination
			if (place[r].num_vertices + all[r].num_vertices > global->cap_vertices || place[r].num_indices + all[r].num_indices > global->cap_indices
				|| place[r].num_meshes + all[r].num_meshes > global->cap_meshes) {
				return VGX_E_NOSPACE;
			}
		}
	}
	// the four streams of one rank's block as byte ranges: {local source, destination in global, bytes}
	struct Piece { const uint8_t* src; uint8_t* dst; size_t bytes; };
	auto blockOf = [&](int r, Piece out[4]) {
		const vgx_rank_sizes& z = all[r];
		const vgx_rank_sizes& o = place[r];
		const bool isRoot = rank == root;
		out[0] = Piece{ (const uint8_t*)local->pos, isRoot ? (uint8_t*)(global->pos + 2 * o.num_vertices) : nullptr, (size_t)z.num_vertices * 8 };
		out[1] = Piece{ (const uint8_t*)local->color, isRoot ? (uint8_t*)(global->color + o.num_vertices) : nullptr, (size_t)z.num_vertices * 4 };
		out[2] = Piece{ (const uint8_t*)local->idx, isRoot ? (uint8_t*)(global->idx + o.num_indices) : nullptr, (size_t)z.num_indices * 2 };
		out[3] = Piece{ (const uint8_t*)local->meshes, isRoot ? (uint8_t*)(global->meshes + o.num_meshes) : nullptr, (size_t)z.num_meshes * sizeof(vgx_mesh) };
	};
	const size_t chunk = gatherChunkBytes();
	size_t maxBytes = 0;
	for (int r = 0; r < nranks; ++r) {
		if (rank != root && r != rank) { continue; }
		Piece b[4]; blockOf(r, b);
		for (int k = 0; k < 4; ++k) { if (b[k].bytes > maxBytes) { maxBytes = b[k].bytes; } }
	}
	const size_t nchunks = maxBytes ? (maxBytes + chunk - 1) / chunk : 0;
	// Inside a group a failed call must not return at once: the group stays open on this thread and every later collective
	// would be queued and never issued. Remember the first error, skip the rest, always close the group.
	int rcclErr = 0;
#define RCCLGRP(call) do { if (!rcclErr) { rcclErr = (call); } } while (0)
	if (rank == root) { // my own block: plain copies on the same stream (they overlap with the incoming transfers)
		Piece b[4]; blockOf(root, b);
		for (int k = 0; k < 4; ++k) { if (b[k].bytes) { noteHip(ctx, hipMemcpyAsync(b[k].dst, b[k].src, b[k].bytes, hipMemcpyDeviceToDevice, s)); } }
	}
	for (size_t c = 0; c < nchunks && !rcclErr; ++c) {
		RCCLCHK(ctx, ctx->rccl->GroupStart());
		for (int r = 0; r < nranks; ++r) {
			if (r == root || (rank != root && r != rank)) { continue; }
			Piece b[4]; blockOf(r, b);
			for (int k = 0; k < 4; ++k) {
				const size_t off = c * chunk;
				if (off >= b[k].bytes) { continue; }
				const size_t n = b[k].bytes - off < chunk ? b[k].bytes - off : chunk;
				if (rank == root) { RCCLGRP(ctx->rccl->Recv(b[k].dst + off, n, kNcclUint8, r, rccl_comm, s)); }
				else { RCCLGRP(ctx->rccl->Send(b[k].src + off, n, kNcclUint8, root, rccl_comm, s)); }
			}
		}
		const int endErr = ctx->rccl->GroupEnd();
		if (!rcclErr) { rcclErr = endErr; }
	}
#undef RCCLGRP
	if (rcclErr) { ctx->lastHipError = 10000 + rcclErr; return VGX_E_HIP; }
	if (rank == root) { // mesh records of rank r sit at [place, place + n): add the block's vertex / index / draw bases
		GatherRebaseArgs ra;
		ra.meshes = global->meshes;
		ra.n = 0;
		uint64_t maxMeshes = 0;
		for (int r = 0; r < nranks; ++r) {
			const vgx_rank_sizes& z = all[r];
			const vgx_rank_sizes& o = place[r];
			if (z.num_meshes && (o.num_vertices || o.num_indices || o.num_draws)) {
				GatherRebase& g = ra.r[ra.n++];
				g.mesh0 = o.num_meshes; g.mesh1 = o.num_meshes + z.num_meshes; g.vbase = o.num_vertices; g.ibase = o.num_indices; g.dbase = (uint32_t)o.num_draws;
				if (z.num_meshes > maxMeshes) { maxMeshes = z.num_meshes; }
			}
		}
		if (ra.n) {
			const uint64_t blocks = (maxMeshes + 255) / 256;
			hipLaunchKernelGGL(k_gather_rebase, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)ra.n), dim3(256), 0, s, ra);
		}
	}
	if (ctx->pendingHipError) { ctx->lastHipError = ctx->pendingHipError; ctx->pendingHipError = 0; return VGX_E_HIP; }
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) { ctx->lastHipError = (int)e; return VGX_E_HIP; }
	return VGX_OK;
}

extern "C" int vgx_gather(vgx_ctx* ctx, void* rccl_comm, int root, const vgx_mesh_out* local, const vgx_rank_sizes* all, const vgx_mesh_out* global, void* stream)
{
	if (!ctx || !rccl_comm || !local || !all) {
		return VGX_E_INVALID_ARG;
	}
	int st;
	{
		DeviceGuard guard(ctx);
		st = bindRccl(ctx);
	}
	if (st != VGX_OK) { return st; }
	int nranks = 0;
	RCCLCHK(ctx, ctx->rccl->CommCount(rccl_comm, &nranks));
	if (nranks < 1 || nranks > VGX_GATHER_MAX_RANKS) { return VGX_E_INVALID_ARG; }
	vgx_rank_sizes place[VGX_GATHER_MAX_RANKS];
	uint64_t vo = 0, io = 0, mo = 0, dofs = 0;
	for (int r = 0; r < nranks; ++r) { // rank order = draw order: exclusive prefix of the sizes
		place[r].num_vertices = vo; place[r].num_indices = io; place[r].num_meshes = mo; place[r].num_draws = dofs;
		vo += all[r].num_vertices; io += all[r].num_indices; mo += all[r].num_meshes; dofs += all[r].num_draws;
	}
	return vgx_gather_at(ctx, rccl_comm, root, local, all, place, global, stream);
}
