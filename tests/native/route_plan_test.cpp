// route_plan_test.cpp -- the ordinary pipeline's host decisions (vg-renderer_amd/csrc/vgx_route_plan.h): batch tag, period decoding,
// period / reuse predicates, heap and one-walk sizing, the route choice of the count and of the immediate call, the options table.
// Host only; prints "ok" and returns 0, or names the first check that failed. Built and run by tests/test_route_plan_host.py. The
// expectations are the rules written out a second time (the expressions vgx_api.hip held before the header) or worked out by hand,
// never the header's own results.
#include <stdio.h>
#include <string.h>
#include <map>
#include <string>

// the library's values (vgx_internal.h, vgx_inst.h, vgx_tmpl_plan.h; tests/test_route_plan_host.py compares them with those headers)
#define VGX_SMALL_DRAWS 2048
#define VGX_BUILD_WAVES 4096
#define VGX_BUILD_BLOCK 8192
#define VGX_INST_BLOCK 256u
#define VGX_INST_WAVES 4096
#define VGX_INST_MIN_INSTANCES 32u
#define VGX_TMPL_MAX_TILE 2048
#include "vgx_route_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!failures++) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } } while (0)

static std::map<std::string, std::string> g_env;
static char* envLookup(const char* name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : &it->second[0]; } // (getenv's signature)
static VgxOptions optionsWith(std::initializer_list<std::pair<const char*, const char*>> kv)
{
	g_env.clear();
	for (const auto& p : kv) { g_env[p.first] = p.second; }
	return vgx_options_read(envLookup);
}

// ---- the old expressions ---------------------------------------------------------------------------------------------------------
static uint64_t oldHeapBuild(bool anyOrThin, uint64_t V, uint64_t ncmd, uint64_t longV)
{
	uint64_t h = V * 9 / 4 + 4 * longV + 2 * (uint64_t)4096 * 8192;
	if (anyOrThin && h < 2 * ncmd + 4096) { h = 2 * ncmd + 4096; }
	return h;
}
static uint64_t oldHeapInst(uint32_t optInstBlock, int optInstWaves, uint64_t V, uint64_t instLong)
{
	const uint64_t grown = (optInstBlock >= 256u) ? V * 9 / 4 + 8 * instLong : V * 10;
	return grown + (uint64_t)optInstWaves * 64 * optInstBlock + 4096;
}
static void oldF1Shape(int optF1Cap, int optF1Seg, uint64_t V, uint64_t ncmd, int* cap, uint32_t* segMax)
{
	*cap = 1664; *segMax = 64;
	if (ncmd) {
		const double perCmd = (double)V / (double)ncmd;
		if (perCmd * 64.0 <= 800.0) { *cap = 1024; }
		else if (perCmd * 64.0 > 1500.0) {
			*cap = 3072;
			const double m = 0.8 * 3072.0 / perCmd;
			*segMax = m >= 64.0 ? 64u : (m >= 32.0 ? 32u : (m >= 16.0 ? 16u : 8u));
		}
	}
	if (optF1Cap) { *cap = optF1Cap; }
	if (optF1Seg) { *segMax = (uint32_t)optF1Seg; }
}
static uint64_t oldSegments(uint32_t maxCmdsPerPath, uint64_t ndraws, uint32_t segMax)
{
	const uint64_t minItems = segMax < 32 ? segMax : 32;
	return ndraws * (uint64_t)(maxCmdsPerPath ? maxCmdsPerPath : 1) / minItems + 2;
}

static void testTagAndPeriod()
{
	CHECK(vgx_batch_tag(0, 7) == 7);
	CHECK(vgx_batch_tag(1, 0) == 0x9E3779B97F4A7C15ull);
	CHECK(vgx_batch_tag(3, 3072) == 3 * 0x9E3779B97F4A7C15ull + 3072); // (wraps)
	CHECK(vgx_batch_tag(0xFFFFFFFFFFFFFFFFull, 5) == 5 - 0x9E3779B97F4A7C15ull);
		CHECK(vgx_period_decode(0, 0) == 0);                         // the detection pass did not run / found nothing
	CHECK(vgx_period_decode(~0ull - 64, 0) == 64);
	CHECK(vgx_period_decode(~0ull - 64, 1) == 0);                // inst_detect_bad
	CHECK(vgx_period_decode(~0ull - 0xFFFFFFFFull, 0) == 0xFFFFFFFFu);
	CHECK(vgx_period_decode(~0ull - 0x100000000ull, 0) == 0); // above 2^32 - 1: no period for the instanced kernel
	CHECK(vgx_period_decode(~0ull - 1, 0) == 1);
}

static void testPredicates()
{
	const VgxOptions on = optionsWith({}), off = optionsWith({ { "VGX_INST", "0" } });
	CHECK(!vgx_period_usable(on, 64, 31 * 64) && vgx_period_usable(on, 64, 32 * 64));
	CHECK(!vgx_period_usable(on, 64, 32 * 64 + 1) && !vgx_period_usable(on, 96, 2976) && vgx_period_usable(on, 96, 3072));
	CHECK(!vgx_period_usable(on, 0, 4096) && !vgx_period_usable(off, 64, 32 * 64));
	CHECK(vgx_period_usable(on, 1, 32) && !vgx_period_usable(on, 1, 31));
	CHECK(!vgx_paths_reused(on, 4096, 0));                                             // distinct == 0: not known
	CHECK(vgx_paths_reused(on, 64 * 32, 64) && !vgx_paths_reused(on, 64 * 32 - 1, 64));  // 32 against 31 draws per used path
	CHECK(vgx_paths_reused(on, 0xFFFFFFFEull, 1) && !vgx_paths_reused(on, 0xFFFFFFFFull, 1)); // 2^32 - 1 draws: the sort holds 32-bit draw indices
	CHECK(!vgx_paths_reused(off, 64 * 32, 64));
}

static void testSizing()
{
	const uint64_t Vs[] = { 0, 1, 1000, 123457, 40000000ull }, ncmds[] = { 0, 1, 4098, 1000000, 90000000ull }, longs[] = { 0, 999, 123457 };
	const VgxOptions def = optionsWith({}), small = optionsWith({ { "VGX_INST_BLOCK", "8" }, { "VGX_INST_WAVES", "5" } });
	for (uint64_t V : Vs) { for (uint64_t ncmd : ncmds) { for (uint64_t L : longs) {
		CHECK(vgx_heap_build_verts(false, V, ncmd, L) == oldHeapBuild(false, V, ncmd, L));
		CHECK(vgx_heap_build_verts(true, V, ncmd, L) == oldHeapBuild(true, V, ncmd, L));
		CHECK(vgx_heap_inst_verts(def, V, L) == oldHeapInst(256, 4096, V, L));
		CHECK(vgx_heap_inst_verts(small, V, L) == oldHeapInst(8, 5, V, L));
	} } }
	// by hand: 1000 vertices, none long -> 2250 + 2 x 4096 x 8192; the thin floor 2 x ncmd + 4096 only above that
	CHECK(vgx_heap_build_verts(false, 1000, 90000000ull, 0) == 2250 + 67108864ull);
	CHECK(vgx_heap_build_verts(true, 1000, 90000000ull, 0) == 180004096ull);
	CHECK(vgx_heap_build_verts(true, 1000, 1000, 0) == 2250 + 67108864ull);
	CHECK(vgx_heap_inst_verts(def, 1000, 10) == 2250 + 80 + 4096ull * 64 * 256 + 4096);
	CHECK(vgx_heap_inst_verts(small, 1000, 10) == 10000 + 5 * 64 * 8 + 4096); // a lane block below VGX_INST_BLOCK: ten times the vertices
	// the one-walk shape: leaves per 64-command chunk at the 800 / 1500 thresholds, the bucket steps, the overrides
	struct { uint64_t V, ncmd; int cap; uint32_t seg; } shapes[] = {
		{ 5000, 0, 1664, 64 },        // command instances not known
		{ 12500, 1000, 1024, 64 },    // 12.5 per command: exactly 800 per chunk
		{ 12501, 1000, 1664, 64 },
		{ 23437, 1000, 1664, 64 },    // 23.437 x 64 = 1499.97
		{ 23438, 1000, 3072, 64 },    // just above 1500; 0.8 x 3072 / 23.438 = 104.9 -> 64
		{ 38000, 1000, 3072, 64 },    // 2457.6 / 38.0 = 64.7
		{ 38500, 1000, 3072, 32 },
		{ 76000, 1000, 3072, 32 },    // 32.3
		{ 77000, 1000, 3072, 16 },
		{ 153000, 1000, 3072, 16 },   // 16.06
		{ 154000, 1000, 3072, 8 },
		{ 1000000, 1000, 3072, 8 },
	};
	const VgxOptions over = optionsWith({ { "VGX_F1_CAP", "777" }, { "VGX_F1_SEG", "12" } }), overSeg = optionsWith({ { "VGX_F1_SEG", "2" } });
	for (const auto& c : shapes) {
		int cap, cap2; uint32_t seg, seg2;
		vgx_f1_shape(def, c.V, c.ncmd, &cap, &seg);
		oldF1Shape(0, 0, c.V, c.ncmd, &cap2, &seg2);
		CHECK(cap == c.cap && seg == c.seg && cap == cap2 && seg == seg2);
		vgx_f1_shape(over, c.V, c.ncmd, &cap, &seg);
		CHECK(cap == 777 && seg == 12);
		vgx_f1_shape(overSeg, c.V, c.ncmd, &cap, &seg);
		CHECK(cap == c.cap && seg == 2);
	}
	const uint32_t segs[] = { 2, 8, 16, 31, 32, 33, 64 }, maxCmds[] = { 0, 1, 2, 700 };
	for (uint32_t sm : segs) { for (uint32_t mc : maxCmds) { for (uint64_t n : { 0ull, 2049ull, 1000000ull }) {
		CHECK(vgx_f1_route_segments(mc, n, sm) == oldSegments(mc, n, sm));
	} } }
	CHECK(vgx_f1_route_segments(2, 4096, 64) == 4096 * 2 / 32 + 2 && vgx_f1_route_segments(0, 4096, 8) == 4096 / 8 + 2);
}

// ---- the route choice -------------------------------------------------------------------------------------------------------------
// tests/immediate_kinds.py: PROPS (draws, period, distinct paths, >= 10 polyline vertices per command instance) and LEARNED
struct Kind { const char* name; uint64_t ndraws; uint32_t period; uint64_t distinct; bool longCurves; VgxRouteKind learned; bool thin; };
static const Kind KINDS[] = {
	{ "periodic64", 3072, 64, 64, true, VGX_ROUTE_PERIODIC, false }, { "periodic48", 3072, 48, 48, true, VGX_ROUTE_PERIODIC, false },
	{ "shuffled64", 3072, 0, 64, true, VGX_ROUTE_GROUPED, false }, { "broken_last", 3072, 0, 65, true, VGX_ROUTE_GROUPED, false },
	{ "broken_first", 3072, 0, 65, true, VGX_ROUTE_GROUPED, false }, { "fill_only64", 3072, 64, 64, true, VGX_ROUTE_PERIODIC, false },
	{ "nothing", 3072, 64, 64, true, VGX_ROUTE_PERIODIC, false }, { "p96x32", 3072, 96, 96, true, VGX_ROUTE_PERIODIC, false },
	{ "periodic64_small", 3072, 64, 64, false, VGX_ROUTE_PERIODIC, false }, { "unique", 3072, 0, 3072, true, VGX_ROUTE_ONE_WALK, false },
	{ "p96x31", 2976, 96, 96, true, VGX_ROUTE_ONE_WALK, false }, { "frame2048", 2048, 0, 2048, true, VGX_ROUTE_FRAME, false },
	{ "large2049", 2049, 0, 2049, true, VGX_ROUTE_ONE_WALK, false }, { "periodic64_big", 3072, 64, 64, true, VGX_ROUTE_PERIODIC, false },
	{ "unique_big", 3072, 0, 3072, true, VGX_ROUTE_ONE_WALK, false }, { "cubics_long", 4096, 0, 4096, true, VGX_ROUTE_ONE_WALK, false },
	{ "cubics_short", 4096, 0, 4096, false, VGX_ROUTE_BUILD, false }, { "thin", 3072, 64, 64, false, VGX_ROUTE_PERIODIC, true },
	{ "tiger10", 2400, 240, 240, false, VGX_ROUTE_BUILD, false },
};
static const Kind& kind(const char* name)
{
	for (const Kind& k : KINDS) { if (!strcmp(k.name, name)) { return k; } }
	CHECK(!"kind");
	return KINDS[0];
}

// what the immediate call knows of a kind once its mirror has been read: 20 commands per draw, 12 or 3 vertices per command
static VgxRouteFacts learnedFacts(const Kind& k)
{
	VgxRouteFacts f = VgxRouteFacts();
	f.ndraws = k.ndraws; f.npaths = 3072; f.maxCmdsPerPath = 40; f.thinStatic = k.thin;
	f.sizesKnown = true; f.ncmd = k.ndraws * 20; f.V = f.ncmd * (k.longCurves ? 12 : 3);
	f.period = k.period; f.distinct = k.distinct;
	f.f1Draws = k.ndraws; f.oneBatch = true;
	return f;
}
// ... and what the count knows: the tolerances too, the long sub-paths, tables for whatever the draw buffers hold
static VgxRouteFacts countedFacts(const Kind& k, bool variesPeriodic, bool variesAny)
{
	VgxRouteFacts f = learnedFacts(k);
	f.oneBatch = false;
	f.tolKnown = true; f.tolVariesPeriodic = variesPeriodic; f.tolVariesAny = variesAny;
	f.longKnown = true; f.longV = 100; f.instLongV = 1000;
	f.f1Draws = k.ndraws <= 2048 ? 0 : 5000;
	return f;
}

static void testChoose()
{
	const VgxOptions def = optionsWith({});
	const uint64_t roomy = 1ull << 40;
	for (const Kind& k : KINDS) {
		const VgxRoute r = vgx_route_choose(learnedFacts(k), def, roomy);
		CHECK(r.kind == k.learned);
		CHECK(r.classes == 1 && !r.permute);                                          // never in the immediate call
		CHECK(r.period == (k.learned == VGX_ROUTE_PERIODIC ? k.period : 0u));         // (p96x31, tiger10: a period that is not usable is not kept)
		const VgxRoute c = vgx_route_choose(countedFacts(k, false, false), def, VGX_NO_HEAP_LIMIT);
		CHECK(c.kind == k.learned && c.classes == 1 && !c.permute);
		CHECK(c.period == (k.learned == VGX_ROUTE_FRAME ? 0u : k.period));            // the count keeps it for calls with another number of draws
		// a batch not seen before: only its size is known
		VgxRouteFacts blank = VgxRouteFacts();
		blank.ndraws = k.ndraws; blank.npaths = 3072; blank.maxCmdsPerPath = 40; blank.thinStatic = k.thin; blank.oneBatch = true;
		CHECK(vgx_route_choose(blank, def, 4096).kind == (k.ndraws <= 2048 ? VGX_ROUTE_FRAME : VGX_ROUTE_BUILD));
	}
	// 2048 against 2049 draws; VGX_NO_SMALL
	VgxRouteFacts f = learnedFacts(kind("frame2048"));
	CHECK(vgx_route_choose(f, def, roomy).kind == VGX_ROUTE_FRAME);
	CHECK(vgx_route_choose(f, optionsWith({ { "VGX_NO_SMALL", "" } }), roomy).kind == VGX_ROUTE_ONE_WALK);
	CHECK(vgx_route_choose(countedFacts(kind("frame2048"), false, false), optionsWith({ { "VGX_NO_SMALL", "" } }), VGX_NO_HEAP_LIMIT).kind == VGX_ROUTE_BUILD); // the count offers one-walk beyond frame size only
	f.ndraws = 2049; f.distinct = 2049;
	CHECK(vgx_route_choose(f, def, roomy).kind == VGX_ROUTE_ONE_WALK);
	// the knobs of the sequence tests
	CHECK(vgx_route_choose(learnedFacts(kind("cubics_short")), optionsWith({ { "VGX_TESS_FLAT1", "2" } }), roomy).kind == VGX_ROUTE_ONE_WALK);
	CHECK(vgx_route_choose(learnedFacts(kind("thin")), optionsWith({ { "VGX_TESS_FLAT1", "2" }, { "VGX_INST", "0" } }), roomy).kind == VGX_ROUTE_BUILD); // a lineTo-only set: k_flatten_thin
	CHECK(vgx_route_choose(learnedFacts(kind("thin")), optionsWith({ { "VGX_TESS_FLAT1", "2" }, { "VGX_INST", "0" }, { "VGX_THIN_STATIC", "0" } }), roomy).kind == VGX_ROUTE_ONE_WALK);
	CHECK(vgx_route_choose(learnedFacts(kind("unique")), optionsWith({ { "VGX_TESS_FLAT1", "0" } }), roomy).kind == VGX_ROUTE_BUILD);
	const VgxOptions noInst = optionsWith({ { "VGX_INST", "0" } });
	CHECK(vgx_route_choose(learnedFacts(kind("periodic64")), noInst, roomy).kind == VGX_ROUTE_ONE_WALK);
	CHECK(vgx_route_choose(learnedFacts(kind("shuffled64")), noInst, roomy).kind == VGX_ROUTE_ONE_WALK);
	CHECK(vgx_route_choose(learnedFacts(kind("periodic64_small")), noInst, roomy).kind == VGX_ROUTE_BUILD);
	// the one-walk shape and its tables: 12 vertices per command -> 768 leaves per chunk -> the 1024-entry instance, buckets of 64;
	// 5000 draws x 40 commands / 32 + 2 segments at the count, the batch's own draws in the immediate call
	VgxRoute r = vgx_route_choose(countedFacts(kind("unique"), false, false), def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_ONE_WALK && r.f1Cap == 1024 && r.f1SegMax == 64 && r.f1SegBound == 5000 * 40 / 32 + 2);
	r = vgx_route_choose(learnedFacts(kind("unique")), def, roomy);
	CHECK(r.kind == VGX_ROUTE_ONE_WALK && r.f1SegBound == 3072 * 40 / 32 + 2);
	f = learnedFacts(kind("unique"));
	f.maxCmdsPerPath = 200000; // 3072 x 200000 / 32 > 2^24 segments: not taken
	CHECK(vgx_route_choose(f, def, roomy).kind == VGX_ROUTE_BUILD);
	f = learnedFacts(kind("unique"));
	f.ncmd = 0;
	CHECK(vgx_route_choose(f, def, roomy).kind == VGX_ROUTE_BUILD);
	// the heap the count sizes: k_flatten_build's, or the instanced kernel's where that is larger
	const Kind& p64 = kind("periodic64");
	const uint64_t V = 3072 * 20 * 12, ncmd = 3072 * 20;
	CHECK(vgx_route_choose(countedFacts(kind("unique"), false, false), def, VGX_NO_HEAP_LIMIT).heapVerts == oldHeapBuild(false, V, ncmd, 100));
	CHECK(oldHeapInst(256, 4096, V, 1000) > oldHeapBuild(false, V, ncmd, 100));
	CHECK(vgx_route_choose(countedFacts(p64, false, false), def, VGX_NO_HEAP_LIMIT).heapVerts == oldHeapInst(256, 4096, V, 1000));
	CHECK(vgx_route_choose(countedFacts(kind("shuffled64"), false, false), def, VGX_NO_HEAP_LIMIT).heapVerts == oldHeapInst(256, 4096, V, 1000));
	CHECK(vgx_route_heap_verts(learnedFacts(p64), def) == oldHeapInst(256, 4096, V, V)); // long sub-paths not known: every vertex counts
	// count only -- tolerances vary with a period: the periodic mapping, instances permuted, at most 1024 classes
	r = vgx_route_choose(countedFacts(p64, true, true), def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_PERIODIC && r.period == 64 && r.permute && r.classes == 256);
	r = vgx_route_choose(countedFacts(p64, true, true), optionsWith({ { "VGX_INST_CLASSES", "4096" } }), VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_PERIODIC && r.permute && r.classes == 1024);
	r = vgx_route_choose(countedFacts(p64, false, true), def, VGX_NO_HEAP_LIMIT); // (they vary in the batch, not between the instances of a place)
	CHECK(r.kind == VGX_ROUTE_PERIODIC && !r.permute && r.classes == 1);
	r = vgx_route_choose(countedFacts(p64, true, true), optionsWith({ { "VGX_INST_CLASSES", "1" } }), VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_PERIODIC && !r.permute && r.classes == 1);
	// ... VGX_INST_PERM=0: grouped by (path, class), the period given up
	r = vgx_route_choose(countedFacts(p64, true, true), optionsWith({ { "VGX_INST_PERM", "0" } }), VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_GROUPED && r.period == 0 && !r.permute && r.classes == 256);
	// ... without a period: grouped with classes, halved until npaths x classes <= 2^22
	VgxRouteFacts g = countedFacts(kind("shuffled64"), false, true);
	r = vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_GROUPED && r.classes == 256 && !r.permute); // 3072 x 256 < 2^22
	g.npaths = 1u << 15;
	CHECK(vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT).classes == 128);
	g.npaths = 1u << 22;
	CHECK(vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT).classes == 1 && vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT).kind == VGX_ROUTE_GROUPED);
	g.npaths = (1u << 22) + 1; g.period = 96; // an unusable period survives when no classes are left
	g.ndraws = 2976 * 4; g.distinct = 96;
	r = vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_PERIODIC && r.period == 96); // 124 instances of 96
	g.ndraws = 96 * 124 + 48; // not whole instances
	r = vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_GROUPED && r.classes == 1 && r.period == 96);
	g.npaths = 3072;
	r = vgx_route_choose(g, def, VGX_NO_HEAP_LIMIT);
	CHECK(r.kind == VGX_ROUTE_GROUPED && r.classes == 256 && r.period == 0);
	// immediate only -- a usable period whose lane-private blocks do not fit the heap the context has: no instanced kernel, on to the
	// next rule (long curves: one-walk; short ones: k_flatten_build), and no period
	const uint64_t need = oldHeapInst(256, 4096, V, V);
	CHECK(vgx_route_choose(learnedFacts(p64), def, need).kind == VGX_ROUTE_PERIODIC);
	r = vgx_route_choose(learnedFacts(p64), def, need - 1);
	CHECK(r.kind == VGX_ROUTE_ONE_WALK && r.period == 0);
	CHECK(vgx_route_choose(learnedFacts(kind("shuffled64")), def, need - 1).kind == VGX_ROUTE_ONE_WALK);
	r = vgx_route_choose(learnedFacts(kind("periodic64_small")), def, 4096);
	CHECK(r.kind == VGX_ROUTE_BUILD && r.period == 0);
	VgxRouteFacts lk = learnedFacts(p64); // the long sub-paths known after VGX_E_GROWN: their count decides
	lk.longKnown = true; lk.instLongV = 10;
	CHECK(vgx_route_choose(lk, def, oldHeapInst(256, 4096, V, 10)).kind == VGX_ROUTE_PERIODIC);
	CHECK(vgx_route_choose(lk, def, oldHeapInst(256, 4096, V, 10) - 1).kind == VGX_ROUTE_ONE_WALK);
	// nothing chosen
	const VgxRoute none = vgx_route_none();
	CHECK(none.kind == VGX_ROUTE_BUILD && none.period == 0 && none.classes == 1 && !none.permute && none.f1Cap == 1664 && none.f1SegMax == 64 && none.f1SegBound == 0);
}

static void testOptions()
{
	const VgxOptions d = optionsWith({});
	CHECK(d.bigEmitMin == (1ull << 18) && d.pickGrid == 1024 && d.tileEmit == 1 && d.psNoSmall == 0 && d.noSmall == 0 && d.buildWaves == 4096);
	CHECK(d.inst == 1 && d.instPerm == 1 && d.instClasses == 256 && d.instWaves == 4096 && d.instBlock == 256);
	CHECK(d.tmpl == 1 && d.tmplClasses == 1 && d.tmplRound == 1 && d.tmplBatch == 0 && d.tmplTile == 2048);
	CHECK(d.tessFlat1 == 1 && d.f1Seg == 0 && d.f1Waves == 0 && d.f1Cap == 0 && d.thinStatic == 1);
	auto one = [](const char* name, const char* value) { return optionsWith({ { name, value } }); };
	// rounds down to a power of two, within 1 .. 65536
	CHECK(one("VGX_INST_CLASSES", "1000").instClasses == 512 && one("VGX_INST_CLASSES", "1").instClasses == 1 && one("VGX_INST_CLASSES", "65536").instClasses == 65536);
	CHECK(one("VGX_INST_CLASSES", "65537").instClasses == 256 && one("VGX_INST_CLASSES", "0").instClasses == 256 && one("VGX_INST_CLASSES", "3").instClasses == 2);
	// a multiple of 64 within 64 .. VGX_TMPL_MAX_TILE
	CHECK(one("VGX_TMPL_TILE", "200").tmplTile == 192 && one("VGX_TMPL_TILE", "64").tmplTile == 64 && one("VGX_TMPL_TILE", "63").tmplTile == 2048);
	CHECK(one("VGX_TMPL_TILE", "2048").tmplTile == 2048 && one("VGX_TMPL_TILE", "2049").tmplTile == 2048 && one("VGX_TMPL_TILE", "2047").tmplTile == 1984);
	CHECK(one("VGX_INST_PERM", "2").instPerm == 2 && one("VGX_INST_PERM", "0").instPerm == 0 && one("VGX_INST_PERM", "3").instPerm == 1 && one("VGX_INST_PERM", "-1").instPerm == 1);
	CHECK(one("VGX_PICK_GRID", "70000").pickGrid == 65536 && one("VGX_PICK_GRID", "3").pickGrid == 3 && one("VGX_PICK_GRID", "0").pickGrid == 1024 && one("VGX_PICK_GRID", "-5").pickGrid == 1024);
	// only values below the default
	CHECK(one("VGX_BUILD_WAVES", "4095").buildWaves == 4095 && one("VGX_BUILD_WAVES", "4096").buildWaves == 4096 && one("VGX_BUILD_WAVES", "5000").buildWaves == 4096);
	CHECK(one("VGX_BUILD_WAVES", "1").buildWaves == 1 && one("VGX_BUILD_WAVES", "0").buildWaves == 4096);
	// presence only
	CHECK(one("VGX_NO_SMALL", "0").noSmall == 1 && one("VGX_NO_SMALL", "").noSmall == 1 && one("VGX_PS_NO_SMALL", "0").psNoSmall == 1);
	// switches: any number but 0
	CHECK(one("VGX_INST", "0").inst == 0 && one("VGX_INST", "7").inst == 1 && one("VGX_INST", "x").inst == 0);
	CHECK(one("VGX_TMPL", "0").tmpl == 0 && one("VGX_TMPL_CLASSES", "0").tmplClasses == 0 && one("VGX_TMPL_ROUND", "0").tmplRound == 0 && one("VGX_TMPL_BATCH", "1").tmplBatch == 1);
	CHECK(one("VGX_TILE_EMIT", "0").tileEmit == 0 && one("VGX_THIN_STATIC", "0").thinStatic == 0);
	// ranges: outside them the default stays
	CHECK(one("VGX_TESS_FLAT1", "2").tessFlat1 == 2 && one("VGX_TESS_FLAT1", "0").tessFlat1 == 0 && one("VGX_TESS_FLAT1", "3").tessFlat1 == 1 && one("VGX_TESS_FLAT1", "-1").tessFlat1 == 1);
	CHECK(one("VGX_F1_SEG", "2").f1Seg == 2 && one("VGX_F1_SEG", "64").f1Seg == 64 && one("VGX_F1_SEG", "1").f1Seg == 0 && one("VGX_F1_SEG", "65").f1Seg == 0);
	CHECK(one("VGX_F1_WAVES", "65536").f1Waves == 65536 && one("VGX_F1_WAVES", "65537").f1Waves == 0 && one("VGX_F1_WAVES", "0").f1Waves == 0);
	CHECK(one("VGX_INST_WAVES", "3").instWaves == 3 && one("VGX_INST_WAVES", "0").instWaves == 4096 && one("VGX_INST_BLOCK", "1").instBlock == 1 && one("VGX_INST_BLOCK", "65537").instBlock == 256);
	CHECK(one("VGX_F1_CAP", "3072").f1Cap == 3072 && one("VGX_F1_CAP", "-4").f1Cap == -4); // taken as it is
	CHECK(one("VGX_BIG_EMIT_MIN", "0").bigEmitMin == 0 && one("VGX_BIG_EMIT_MIN", "18446744073709551615").bigEmitMin == ~0ull); // (all of uint64_t)
	// one knob leaves the others alone
	const VgxOptions o = optionsWith({ { "VGX_INST_BLOCK", "8" }, { "VGX_INST_WAVES", "5" } });
	CHECK(o.instBlock == 8 && o.instWaves == 5 && o.inst == 1 && o.instClasses == 256 && o.buildWaves == 4096);
}

int main()
{
	testTagAndPeriod();
	testPredicates();
	testSizing();
	testChoose();
	testOptions();
	if (failures) { printf("%d check(s) failed\n", failures); return 1; }
	printf("ok\n");
	return 0;
}
