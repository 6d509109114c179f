// vgx_route_plan.h -- the ordinary pipeline, the host's decisions (compiles without HIP: tests/native/route_plan_test.cpp).
//
// Which flatten route a batch that is not a template takes and how its scratch is sized, from what the host knows about it:
// vgx_tessellate_count from the totals it read back, vgx_tessellate_immediate from the mirror of the last call on the same (path set,
// number of draws). ONE rule set for both (vgx_route_choose); what a caller does not know it says so in the facts. Also the context's
// options. The constants stay with their kernels: the includer defines VGX_SMALL_DRAWS, VGX_BUILD_WAVES, VGX_BUILD_BLOCK
// (vgx_internal.h), VGX_INST_MIN_INSTANCES, VGX_INST_BLOCK, VGX_INST_WAVES (vgx_inst.h) and VGX_TMPL_MAX_TILE first.
#ifndef VGX_ROUTE_PLAN_H
#define VGX_ROUTE_PLAN_H

#include <stdint.h>
#include <stdlib.h>

// ---- options: read from the environment ONCE at vgx_create (tuning / testing knobs), never on the call path -------------------
struct VgxOptions
{
	uint64_t bigEmitMin; uint32_t pickGrid, instClasses, instBlock, tmplTile;
	int tileEmit, psNoSmall, noSmall, buildWaves, inst, instPerm, instWaves, tmpl, tmplClasses, tmplRound, tmplBatch, tessFlat1, f1Seg, f1Waves, f1Cap, thinStatic;
};
// a knob's number when it is set and lies within lo .. hi, else its default; a switch: any number but 0
inline int vgx_opt_int(const char* e, int def, int lo, int hi) { const int v = e ? atoi(e) : def; return v >= lo && v <= hi ? v : def; }
inline int vgx_opt_flag(const char* e, int def) { return e ? atoi(e) != 0 : def; }

// One line per knob: name, default, range / rounding rule. `getenv`: the C library's, or the test's table
inline VgxOptions vgx_options_read(char* (*getenv)(const char*))
{
	VgxOptions o; const char* e;
	o.bigEmitMin = (e = getenv("VGX_BIG_EMIT_MIN")) ? strtoull(e, nullptr, 10) : 1ull << 18; // vertex capacity from which a call launches the tile kernel / k_stroke_long
	o.pickGrid = vgx_opt_int(getenv("VGX_PICK_GRID"), 1024, 1, 0x7FFFFFFF); // workgroups of k_pick_tris: four per CU of a 256-CU part, those without a tile exit at once ...
	if (o.pickGrid > 65536) { o.pickGrid = 65536; } // ... any N > 0, at most 65536 (the tests force many tiles per workgroup)
	o.tileEmit = vgx_opt_flag(getenv("VGX_TILE_EMIT"), 1); // 0: ordinary batches through k_fill + k_stroke_simple, no tile kernel
	o.psNoSmall = getenv("VGX_PS_NO_SMALL") ? 1 : 0; // set (whatever it says): frame-sized path sets through the large-set launch sequence
	o.noSmall = getenv("VGX_NO_SMALL") ? 1 : 0; // set: frame-sized batches through the large-batch launch sequence
	o.buildWaves = vgx_opt_int(getenv("VGX_BUILD_WAVES"), VGX_BUILD_WAVES, 1, VGX_BUILD_WAVES - 1); // grid of k_flatten_build
	o.inst = vgx_opt_flag(getenv("VGX_INST"), 1); // 0: instanced batches through k_flatten_build as well
	o.instPerm = (e = getenv("VGX_INST_PERM")) ? (atoi(e) == 2 ? 2 : atoi(e) != 0) : 1; // scales differ: permute instances (1) or sort draws by (path, class) (0); 2: the several-kernel sort
	o.instClasses = vgx_opt_int(getenv("VGX_INST_CLASSES"), 256, 1, 65536); // tolerance classes per path when the instances differ in scale ...
	while (o.instClasses & (o.instClasses - 1)) { o.instClasses &= o.instClasses - 1; } // ... rounded down to a power of two
	o.instWaves = vgx_opt_int(getenv("VGX_INST_WAVES"), VGX_INST_WAVES, 1, 65536); // k_flatten_inst (vgx_inst.hip): grid ...
	o.instBlock = vgx_opt_int(getenv("VGX_INST_BLOCK"), VGX_INST_BLOCK, 1, 65536); // ... and lane block
	o.tmpl = vgx_opt_flag(getenv("VGX_TMPL"), 1); // 0: no template mode
	o.tmplClasses = vgx_opt_flag(getenv("VGX_TMPL_CLASSES"), 1); // 0: only for batches whose instances all repeat the first period
	o.tmplRound = vgx_opt_flag(getenv("VGX_TMPL_ROUND"), 1); // 0: batches with Round joins keep the ordinary pipeline
	o.tmplBatch = vgx_opt_flag(getenv("VGX_TMPL_BATCH"), 0); // vgx_set_static_batches: a batch without a period becomes ONE template
	o.tmplTile = vgx_opt_int(getenv("VGX_TMPL_TILE"), VGX_TMPL_MAX_TILE, 64, VGX_TMPL_MAX_TILE) / 64 * 64; // elements per tile, a multiple of 64
	o.tessFlat1 = vgx_opt_int(getenv("VGX_TESS_FLAT1"), 1, 0, 2); // vgx_tessellate's one-walk route: 1 = batches of long curves, 0 = never, 2 = every eligible batch
	o.f1Seg = vgx_opt_int(getenv("VGX_F1_SEG"), 0, 2, 64); // vgx_flatten (vgx_flat1.hip): the segment bucket, ...
	o.f1Waves = vgx_opt_int(getenv("VGX_F1_WAVES"), 0, 1, 65536); // ... its grid (persistent one-wave workgroups), ...
	o.f1Cap = (e = getenv("VGX_F1_CAP")) ? atoi(e) : 0; // ... the leaf-list capacity of the kernel instance (0 = chosen per batch)
	o.thinStatic = vgx_opt_flag(getenv("VGX_THIN_STATIC"), 1); // 0: lineTo-only path sets through k_flatten_build, not k_flatten_thin (vgx_thin.h)
	return o;
}

// ---- the pure rules ------------------------------------------------------------------------------------------------------------
// What identifies a batch where only its size and its path set are compared: path set generation, number of draws
inline uint64_t vgx_batch_tag(uint64_t psGen, uint64_t ndraws) { return psGen * 0x9E3779B97F4A7C15ull + ndraws; }

// The period k_inst_detect found (VgxTotals::inst_detect_inv / inst_detect_bad): the draws repeat one sequence of that many paths (a
// drawing submitted for many instances). 0: none, or more than the instanced kernel's 32 bits hold
inline uint32_t vgx_period_decode(unsigned long long detectInv, uint32_t detectBad)
{
	const unsigned long long P = (detectInv != 0 && !detectBad) ? ~0ull - detectInv : 0ull;
	return P <= 0xFFFFFFFFull ? (uint32_t)P : 0u;
}
// Can the instanced kernel assume that `ndraws` draws repeat a sequence of P paths (enough whole instances of it)?
inline bool vgx_period_usable(const VgxOptions& o, uint64_t P, uint64_t ndraws) { return P && o.inst && ndraws % P == 0 && ndraws / P >= VGX_INST_MIN_INSTANCES; }
// Do `ndraws` draws over `distinct` paths reuse them (>= VGX_INST_MIN_INSTANCES draws per used path on average)? Then grouped mode sorts them by path
inline bool vgx_paths_reused(const VgxOptions& o, uint64_t ndraws, uint64_t distinct) { return o.inst && distinct != 0 && ndraws < 0xFFFFFFFFull && ndraws / distinct >= VGX_INST_MIN_INSTANCES; }

// Polyline scratch doubles as the heap of k_flatten_build, for a batch of V polyline vertices, `longV` of them in sub-paths longer than
// VGX_LONG_SUBPATH, `ncmd` command instances. Its waves switch to a fresh block when a chunk does not fit: the unused tail of the old block
// is smaller than that chunk (<= 1x the vertices), the moved prefix of a spanning sub-path is < VGX_LONG_SUBPATH per >= VGX_BUILD_BLOCK
// block (<= 1/4), longer sub-paths grow geometrically (<= 4x their size). Plus every wave's last open block. k_flatten_thin (`thin`: a
// lineTo-only set, or any set) places draw d at its command prefix -- one slot per command instance --, the exact builder's draws behind
inline uint64_t vgx_heap_build_verts(bool thin, uint64_t V, uint64_t ncmd, uint64_t longV)
{
	uint64_t h = V * 9 / 4 + 4 * longV + 2 * (uint64_t)VGX_BUILD_WAVES * VGX_BUILD_BLOCK;
	if (thin && h < 2 * ncmd + 4096) { h = 2 * ncmd + 4096; }
	return h;
}
// ... of k_flatten_inst's lane-private blocks (instLong = vertices in sub-paths longer than VGX_INST_LONG_SUBPATH): a block left behind wastes
// less than the one sub-path that did not fit, longer sub-paths grow geometrically (<= 4x + a block, with head room), plus every lane's open block
inline uint64_t vgx_heap_inst_verts(const VgxOptions& o, uint64_t V, uint64_t instLong)
{
	const uint64_t grown = (o.instBlock >= VGX_INST_BLOCK) ? V * 9 / 4 + 8 * instLong : V * 10;
	return grown + (uint64_t)o.instWaves * 64 * o.instBlock + 4096;
}

// Leaf-list capacity of the one-walk kernel instance and commands per segment bucket, for V polyline vertices over `ncmd` command instances
// (0: not known). A 64-command chunk of ~45-segment cubics stages ~1450 leaves (the 1664-entry instance: six waves per CU); lighter batches
// take the 1024-entry instance (eight waves per CU), heavier ones the 3072-entry instance with smaller buckets, so that a chunk's leaves
// still fit (a chunk that overflows the list walks its cubics a second time). VGX_F1_CAP / VGX_F1_SEG override both.
inline void vgx_f1_shape(const VgxOptions& o, uint64_t V, uint64_t ncmd, int* cap, uint32_t* segMax)
{
	*cap = 1664; *segMax = 64;
	if (ncmd) {
		const double perCmd = (double)V / (double)ncmd;
		if (perCmd * 64.0 <= 800.0) { *cap = 1024; }
		else if (perCmd * 64.0 > 1500.0) {
			// long curves (145 segments per cubic at box 10 000): buckets of a power of two -- 2^k cubics become 64 tasks after whole rounds of
			// cutting. Measured on 1 M such cubics: 3072 entries x 32 commands 3.4 ms, 1664 x 16 4.1 ms, 1664 x 8 6.2 ms (two-phase entry: 6.0 ms)
			*cap = 3072;
			const double m = 0.8 * 3072.0 / perCmd;
			*segMax = m >= 64.0 ? 64u : (m >= 32.0 ? 32u : (m >= 16.0 ? 16u : 8u));
		}
	}
	if (o.f1Cap) { *cap = o.f1Cap; }
	if (o.f1Seg) { *segMax = (uint32_t)o.f1Seg; }
}
// segments the one-walk route's look-back tables must hold for ANY `ndraws` draws on a path set whose longest path has `maxCmdsPerPath` commands
inline uint64_t vgx_f1_route_segments(uint32_t maxCmdsPerPath, uint64_t ndraws, uint32_t segMax)
{
	const uint64_t minItems = segMax < 32 ? segMax : 32;
	return ndraws * (uint64_t)(maxCmdsPerPath ? maxCmdsPerPath : 1) / minItems + 2;
}

// ---- the decision --------------------------------------------------------------------------------------------------------------
// What a decision reads about the batch. A caller that does not know a group of facts leaves it zero and its flag false.
struct VgxRouteFacts
{
	uint64_t ndraws;
	uint32_t npaths, maxCmdsPerPath; bool thinStatic; // of the path set; ... a lineTo-only set with its static layout tables (vgx_thin.h)
	bool sizesKnown; uint64_t V, ncmd; // polyline vertices, command instances
	uint32_t period; uint64_t distinct; // the period of its paths, decoded (0: none, or the detection pass did not run); different paths used (0: not known)
	bool tolKnown, tolVariesPeriodic, tolVariesAny; // do the tolerances vary between the instances at some place of the period / anywhere in the batch
	bool longKnown; uint64_t longV, instLongV; // vertices in sub-paths longer than VGX_LONG_SUBPATH / VGX_INST_LONG_SUBPATH (not known: every vertex counts)
	uint64_t f1Draws;                // draws the one-walk tables would be sized for (0: the one-walk route is not offered)
	bool oneBatch;                   // the facts are those of THIS (path set, number of draws) only: nothing is kept for other draw counts
};
// BUILD: k_flatten_build (k_flatten_thin for a lineTo-only set); FRAME: frame-sized, the five-launch sequence; PERIODIC: k_flatten_inst, lane =
// instance; GROUPED: k_flatten_inst over the draws sorted by path (k_inst_hist / k_inst_plan / k_inst_scatter, every call); ONE_WALK: k_flat1
enum VgxRouteKind : uint32_t { VGX_ROUTE_BUILD = 0, VGX_ROUTE_FRAME, VGX_ROUTE_PERIODIC, VGX_ROUTE_GROUPED, VGX_ROUTE_ONE_WALK };
struct VgxRoute
{
	VgxRouteKind kind;   // of the batch the facts describe (one-walk: the shape below is only meant with it)
	uint32_t period;     // of the path sequence (0 = none). A later call re-checks it for ITS draw count (vgx_period_usable), the device for its draws
	uint32_t classes;    // instances of different scales: the sort key is (path, tolerance class), this many per path (1 = by path only): a wave's lanes stay in lock-step
	bool permute;        // ... periodic mode: every call sorts the INSTANCES by tolerance class instead (vgx_launch_inst_perm)
	int f1Cap; uint32_t f1SegMax; uint64_t f1SegBound; // one-walk: the kernel instance / bucket size, the segments the look-back tables hold
	uint64_t heapVerts;  // polyline vertices the heap must hold (sizes known)
};
inline VgxRoute vgx_route_none() { VgxRoute r = VgxRoute(); r.classes = 1; r.f1Cap = 1664; r.f1SegMax = 64; return r; }

// the instanced kernel's heap when the draws repeat a sequence or reuse their paths and it is the larger one, else k_flatten_build's
inline uint64_t vgx_route_heap_verts(const VgxRouteFacts& f, const VgxOptions& o)
{
	const uint64_t build = vgx_heap_build_verts(f.thinStatic, f.V, f.ncmd, f.longKnown ? f.longV : f.V), inst = vgx_heap_inst_verts(o, f.V, f.longKnown ? f.instLongV : f.V);
	return (vgx_period_usable(o, f.period, f.ndraws) || vgx_paths_reused(o, f.ndraws, f.distinct)) && inst > build ? inst : build;
}

#define VGX_NO_HEAP_LIMIT (~0ull)
// heapLimit: the vertices the heap holds when it cannot grow in this call (the instanced kernel only when its lane-private blocks fit)
inline VgxRoute vgx_route_choose(const VgxRouteFacts& f, const VgxOptions& o, uint64_t heapLimit)
{
	VgxRoute r = vgx_route_none();
	if (f.sizesKnown) { r.heapVerts = vgx_route_heap_verts(f, o); }
	if (f.ndraws <= VGX_SMALL_DRAWS && !o.noSmall) { r.kind = VGX_ROUTE_FRAME; return r; }
	const bool instFits = vgx_heap_inst_verts(o, f.V, f.longKnown ? f.instLongV : f.V) <= heapLimit;
	uint32_t period = instFits ? f.period : 0;
	const bool reused = instFits && f.ndraws > VGX_SMALL_DRAWS && vgx_paths_reused(o, f.ndraws, f.distinct);
	const bool periodic = vgx_period_usable(o, period, f.ndraws);
	if (reused && o.instClasses > 1 && f.tolKnown && (periodic ? f.tolVariesPeriodic : f.tolVariesAny)) {
		// The instances of a path differ in scale: with lane = instance the lanes of a wave would disagree about nearly every cubic
		uint32_t nc = o.instClasses;
		if (periodic && o.instPerm) { // the sequence repeats: keep the periodic mapping (closed-form offsets, no per-draw sort), permute the INSTANCES
			if (nc > 1024u) { nc = 1024u; }
			r.permute = true;
		} else { // grouped mode sorted by (path, tolerance class)
			while (nc > 1 && (uint64_t)f.npaths * nc > (1ull << 22)) { nc >>= 1; } // scratch of at most 4 M keys
			if (nc > 1) { period = 0; }
		}
		r.classes = nc;
	}
	r.period = period;
	if (vgx_period_usable(o, period, f.ndraws)) { r.kind = VGX_ROUTE_PERIODIC; return r; }
	if (f.oneBatch) { r.period = 0; }
	if (reused) { r.kind = VGX_ROUTE_GROUPED; return r; } // paths are reused but not as a repeating sequence
	// the one-walk route? Unrelated draws, curves (not a lineTo-only set), and long ones: >= 10 polyline vertices per command instance (VGX_TESS_FLAT1=2:
	// whatever their length; the routes cross between 7.5 and 12.6, profiles/experiments/r06_cubics_tessellate_boxes.txt). Not beyond 2^24 segments
	if (f.f1Draws && o.tessFlat1 && f.sizesKnown && !(f.thinStatic && o.thinStatic) && f.ncmd != 0 && (o.tessFlat1 == 2 || f.V >= 10 * f.ncmd)) {
		vgx_f1_shape(o, f.V, f.ncmd, &r.f1Cap, &r.f1SegMax);
		r.f1SegBound = vgx_f1_route_segments(f.maxCmdsPerPath, f.f1Draws, r.f1SegMax);
		if (r.f1SegBound <= (1ull << 24)) { r.kind = VGX_ROUTE_ONE_WALK; }
	}
	return r;
}

#endif // VGX_ROUTE_PLAN_H
