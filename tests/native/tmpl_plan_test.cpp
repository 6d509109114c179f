// tmpl_plan_test.cpp -- template mode's host decisions (vg-renderer_amd/csrc/vgx_tmpl_plan.h): kernel kind and tile size from the
// style word, class grouping, per-class sizes, Round-join layout, the batch plan and its two tables. Host only; prints "ok" and
// returns 0, or names the first check that failed. Built and run by tests/test_tmpl_plan_host.py. The expectations are the rules
// written out a second time (the nested conditional vgx_api.hip used to hold) or worked out by hand, never the header's own results.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

// tile sizes that differ from each other, so that each rule shows (the library builds with 2048 for all three)
#define VGX_TMPL_MAX_TILE 2048
#define VGX_TMPL_GENERAL_TILE 1024
#define VGX_TMPL_RC_TILE 1536
#include "vgx_tmpl_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!failures++) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } } while (0)

// the rule as the host code spelled it before the enums
static uint32_t oracleKernel(uint32_t styles)
{
	return (styles & 4u) ? ((styles & 3u) ? 3u : ((styles & 32u) ? 6u : 5u)) : ((styles & 2u) ? 2u : ((styles & 8u) ? ((styles & 1u) ? 2u : 4u) : ((styles & 1u) ? 1u : 0u)));
}
static uint32_t oracleTile(uint32_t kernelKind, uint32_t optTmplTile)
{
	uint32_t tileSize = ((kernelKind == 2u || kernelKind == 3u) && optTmplTile > VGX_TMPL_GENERAL_TILE) ? (uint32_t)VGX_TMPL_GENERAL_TILE : optTmplTile;
	if ((kernelKind == 5u || kernelKind == 6u) && optTmplTile == VGX_TMPL_MAX_TILE) { tileSize = VGX_TMPL_RC_TILE; }
	return tileSize;
}

static void testKernelAndTile()
{
	CHECK(VGX_TK_EMIT == 0 && VGX_TK_OPEN == 1 && VGX_TK_GENERAL == 2 && VGX_TK_ROUND == 3 && VGX_TK_BEVEL == 4 && VGX_TK_ROUND_AA == 5 && VGX_TK_ROUND_AA_OPEN == 6);
	CHECK(VGX_TS_OPEN_MITER == 1 && VGX_TS_OTHER == 2 && VGX_TS_ROUND == 4 && VGX_TS_CLOSED_BEVEL == 8 && VGX_TS_ROUND_AA_CLOSED == 16 && VGX_TS_ROUND_AA_OPEN == 32);
	for (uint32_t s = 0; s < 64; ++s) {
		const uint32_t k = oracleKernel(s);
		CHECK((uint32_t)vgx_tmpl_kernel_for(s) == k);
		CHECK(vgx_tmpl_kernel_is_round((VgxTmplKernel)k) == (k == 3 || k == 5 || k == 6));
	}
	CHECK(vgx_tmpl_kernel_for(0) == VGX_TK_EMIT);
	CHECK(vgx_tmpl_kernel_for(1) == VGX_TK_OPEN);
	CHECK(vgx_tmpl_kernel_for(8) == VGX_TK_BEVEL);
	CHECK(vgx_tmpl_kernel_for(8 | 1) == VGX_TK_GENERAL);
	CHECK(vgx_tmpl_kernel_for(4 | 16) == VGX_TK_ROUND_AA);
	CHECK(vgx_tmpl_kernel_for(4 | 32) == VGX_TK_ROUND_AA_OPEN);
	CHECK(vgx_tmpl_kernel_for(4 | 1) == VGX_TK_ROUND);
	const uint32_t opts[] = { 64, 1024, 1088, 1536, 2048, 4096 };
	for (uint32_t k = 0; k <= 6; ++k) {
		for (uint32_t o : opts) { CHECK(vgx_tmpl_tile_for((VgxTmplKernel)k, o) == oracleTile(k, o)); }
		CHECK(vgx_tmpl_tile_for((VgxTmplKernel)k, 64) == 64); // an override stands for every kind
	}
	CHECK(vgx_tmpl_tile_for(VGX_TK_GENERAL, 2048) == 1024 && vgx_tmpl_tile_for(VGX_TK_ROUND, 1088) == 1024); // capped above the general tile ...
	CHECK(vgx_tmpl_tile_for(VGX_TK_GENERAL, 1024) == 1024 && vgx_tmpl_tile_for(VGX_TK_ROUND, 960) == 960);   // ... and only there
	CHECK(vgx_tmpl_tile_for(VGX_TK_ROUND_AA, 2048) == 1536 && vgx_tmpl_tile_for(VGX_TK_ROUND_AA_OPEN, 2048) == 1536); // their own tile at the default ...
	CHECK(vgx_tmpl_tile_for(VGX_TK_ROUND_AA, 1984) == 1984 && vgx_tmpl_tile_for(VGX_TK_ROUND_AA_OPEN, 4096) == 4096); // ... and only there
	CHECK(vgx_tmpl_tile_for(VGX_TK_EMIT, 2048) == 2048 && vgx_tmpl_tile_for(VGX_TK_OPEN, 2048) == 2048 && vgx_tmpl_tile_for(VGX_TK_BEVEL, 2048) == 2048);
}

static VgxTotals totalsOf(uint64_t elems, uint64_t verts, uint64_t idx, uint64_t poly, uint64_t meshes, uint32_t round)
{
	VgxTotals t;
	memset(&t, 0, sizeof(t));
	t.sizes.num_elements = elems; t.sizes.num_vertices = verts; t.sizes.num_indices = idx; t.sizes.num_poly_vertices = poly; t.sizes.num_meshes = meshes;
	t.num_round_meshes = round;
	return t;
}
static void testEligible()
{
	CHECK(vgx_tmpl_eligible(totalsOf(1, 0, 0, 0, 0, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(0, 0, 0, 0, 0, 0), false)); // nothing to emit
	CHECK(vgx_tmpl_eligible(totalsOf((1ull << 31) - 1, (1ull << 29) - 1, (1ull << 31) - 1, (1ull << 32) - 1, (1ull << 32) - 1, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1ull << 31, 1, 1, 1, 1, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1, 1ull << 29, 1, 1, 1, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1, 1, 1ull << 31, 1, 1, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1, 1, 1, 1ull << 32, 1, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1, 1, 1, 1, 1ull << 32, 0), false));
	CHECK(!vgx_tmpl_eligible(totalsOf(1, 1, 1, 1, 1, 3), false) && vgx_tmpl_eligible(totalsOf(1, 1, 1, 1, 1, 3), true));
}

static void testGrouping()
{
	std::vector<uint32_t> cls, reps;
	const unsigned long long a = 0xA5A5ull, b = 7ull, c = ~0ull;
	const unsigned long long h[] = { a, b, a, c, b };
	CHECK(vgx_tmpl_group_classes(h, 5, cls, reps));
	CHECK((cls == std::vector<uint32_t>{ 0, 1, 0, 2, 1 }) && (reps == std::vector<uint32_t>{ 0, 1, 3 }));
	CHECK(vgx_tmpl_group_classes(h, 0, cls, reps) && cls.empty() && reps.empty());
	// 64 flavours, each seen again, are accepted; the 65th is refused where it appears and not before
	std::vector<unsigned long long> many;
	for (uint32_t k = 0; k < 64; ++k) { many.push_back(1000 + 3 * k); }
	for (uint32_t k = 0; k < 64; ++k) { many.push_back(1000 + 3 * (63 - k)); }
	CHECK(VGX_TMPL_MAX_CLASSES == 64);
	CHECK(vgx_tmpl_group_classes(many.data(), many.size(), cls, reps) && reps.size() == 64);
	for (uint32_t k = 0; k < 64; ++k) { CHECK(reps[k] == k && cls[k] == k && cls[64 + k] == 63 - k); }
	many.push_back(5);        // instance 128: the 65th flavour
	many.push_back(1000);
	CHECK(vgx_tmpl_group_classes(many.data(), 128, cls, reps) && reps.size() == 64); // up to the instance in front of it: fine
	CHECK(!vgx_tmpl_group_classes(many.data(), 129, cls, reps));
	CHECK(!vgx_tmpl_group_classes(many.data(), 130, cls, reps));
}

static VgxTmplClass classAt(uint64_t elem0, uint64_t v0, uint64_t i0, uint32_t mesh0, uint32_t tile0, uint32_t relem0 = 0, uint32_t rmesh0 = 0)
{
	VgxTmplClass r;
	memset(&r, 0, sizeof(r));
	r.elem0 = elem0; r.v0 = v0; r.i0 = i0; r.mesh0 = mesh0; r.tile0 = tile0; r.round[VGX_TC_ELEM0] = relem0; r.round[VGX_TC_MESH0] = rmesh0;
	return r;
}
static bool sizesAre(const vgx_sizes& z, uint64_t poly, uint64_t sub, uint64_t meshes, uint64_t v, uint64_t i, uint64_t serial, uint64_t cmd, uint64_t elems, uint64_t fill)
{
	return z.num_poly_vertices == poly && z.num_subpaths == sub && z.num_meshes == meshes && z.num_vertices == v && z.num_indices == i
		&& z.num_serial_draws == serial && z.num_cmd_instances == cmd && z.num_elements == elems && z.num_fill_elements == fill && z.num_drawcmds == 0;
}
static vgx_sizes sizesOf(uint64_t poly, uint64_t sub, uint64_t meshes, uint64_t v, uint64_t i, uint64_t serial, uint64_t cmd, uint64_t elems, uint64_t fill)
{
	vgx_sizes z;
	memset(&z, 0, sizeof(z));
	z.num_poly_vertices = poly; z.num_subpaths = sub; z.num_meshes = meshes; z.num_vertices = v; z.num_indices = i;
	z.num_serial_draws = serial; z.num_cmd_instances = cmd; z.num_elements = elems; z.num_fill_elements = fill;
	return z;
}

static void testClassSizes()
{
	// three classes; every column differs. Columns of the sums: polyline vertices, sub-paths, command instances, fill elements in FRONT of
	// the class -- and serial draws, where row c + 1 holds class c's own count (1 -> row 1 = 2, not a difference: class 1 has 0, class 2 has 5)
	const VgxTmplClass cls[4] = { classAt(0, 0, 0, 0, 0), classAt(100, 1000, 3000, 4, 1), classAt(250, 2100, 6500, 9, 3), classAt(310, 2500, 7700, 11, 4) };
	const unsigned long long csum[4 * 5] = { 0, 0, 0, 0, 0,  40, 3, 12, 60, 2,  95, 8, 30, 130, 0,  120, 10, 41, 150, 5 };
	std::vector<vgx_sizes> csz;
	CHECK(vgx_tmpl_class_sizes(cls, csum, 3, csz) && csz.size() == 3);
	CHECK(sizesAre(csz[0], 40, 3, 4, 1000, 3000, 2, 12, 100, 60));
	CHECK(sizesAre(csz[1], 55, 5, 5, 1100, 3500, 0, 18, 150, 70));
	CHECK(sizesAre(csz[2], 25, 2, 2, 400, 1200, 5, 11, 60, 20));
	// a class beyond the limits of one instance: no elements; 2^29 vertices
	const VgxTmplClass empty[3] = { classAt(0, 0, 0, 0, 0), classAt(100, 10, 10, 1, 1), classAt(100, 20, 20, 2, 1) };
	const unsigned long long zeros[3 * 5] = { 0 };
	CHECK(!vgx_tmpl_class_sizes(empty, zeros, 2, csz));
	const VgxTmplClass big[3] = { classAt(0, 0, 0, 0, 0), classAt(100, (1ull << 29) - 1, 10, 1, 1), classAt(200, (1ull << 30) - 1, 20, 2, 2) };
	CHECK(!vgx_tmpl_class_sizes(big, zeros, 2, csz));
	CHECK(vgx_tmpl_class_sizes(big, zeros, 1, csz) && csz[0].num_vertices == (1ull << 29) - 1);
}

static void testRoundLayout()
{
	std::vector<uint64_t> relems;
	uint32_t lds = 77;
	// classes begin at Round-join meshes 0, 2, 2 of 5 and elements 0, 9, 9 of 20: the middle class holds none
	const VgxTmplClass cls[4] = { classAt(0, 0, 0, 0, 0, 0, 0), classAt(0, 0, 0, 0, 0, 9, 2), classAt(0, 0, 0, 0, 0, 9, 2), classAt(0, 0, 0, 0, 0, 0x3F /* styles */, 5) };
	vgx_tmpl_round_layout(cls, 3, 5, 20, relems, lds);
	CHECK((relems == std::vector<uint64_t>{ 9, 0, 11 }) && lds == 3);
	vgx_tmpl_round_layout(cls, 1, 5, 20, relems, lds);
	CHECK((relems == std::vector<uint64_t>{ 20 }) && lds == 5);
}

static bool instIs(const VgxTmplInst& r, uint64_t v, uint64_t i, uint32_t m, uint32_t cls, uint32_t cmesh0, uint64_t rel)
{
	return r.v == v && r.i == i && r.m == m && r.cls == cls && r.cmesh0 == cmesh0 && r.pad == 0 && r.rel == rel;
}

static void testBatchPlan()
{
	// two classes: class 0 = meshes [0, 5), tiles [0, 2), Round-join elements [0, 7); class 1 = meshes [5, 8), tiles [2, 5), elements [7, 11)
	const VgxTmplClass cls[3] = { classAt(0, 0, 0, 0, 0, 0, 0), classAt(50, 100, 300, 5, 2, 7, 2), classAt(90, 170, 500, 8, 5, 0, 3) };
	const vgx_sizes csz[2] = { sizesOf(10, 2, 5, 100, 300, 1, 20, 50, 30), sizesOf(11, 3, 3, 70, 200, 0, 22, 40, 15) };
	const uint32_t instCls[3] = { 1, 0, 1 };
	const uint64_t relems[2] = { 7, 4 };
	VgxTmplPlan p;
	CHECK(vgx_tmpl_plan_batch(csz, cls, 2, 3, instCls, relems, p));
	CHECK((p.cnt == std::vector<uint64_t>{ 1, 2 }));
	CHECK(sizesAre(p.total, 32, 8, 11, 240, 700, 1, 64, 130, 60));
	CHECK(p.numWg == 8 && p.relemWords == 15);
	CHECK(p.inst.size() == 4);
	CHECK(instIs(p.inst[0], 0, 0, 0, 1, 5, (uint64_t)0 - 7)); // (wraps: the kernel adds an element number >= 7)
	CHECK(instIs(p.inst[1], 70, 200, 3, 0, 0, 4));
	CHECK(instIs(p.inst[2], 170, 500, 8, 1, 5, 11 - 7));
	CHECK(instIs(p.inst[3], 240, 700, 11, 0, 0, 0));           // the terminal entry = the totals
	const uint32_t wg[8][2] = { { 1, 0 }, { 1, 1 }, { 0, 2 }, { 0, 3 }, { 0, 4 }, { 2, 2 }, { 2, 3 }, { 2, 4 } }; // class after class
	CHECK(p.wg.size() == 8);
	for (size_t k = 0; k < 8 && k < p.wg.size(); ++k) { CHECK(p.wg[k].inst == wg[k][0] && p.wg[k].tile == wg[k][1]); }
	// no Round joins: no table words, rel = 0
	CHECK(vgx_tmpl_plan_batch(csz, cls, 2, 3, instCls, nullptr, p));
	CHECK(p.relemWords == 0 && p.numWg == 8 && p.inst.size() == 4 && instIs(p.inst[0], 0, 0, 0, 1, 5, 0) && instIs(p.inst[2], 170, 500, 8, 1, 5, 0));
	// one class: instances x sizes, no tables
	const VgxTmplClass one[2] = { classAt(0, 0, 0, 0, 0), classAt(50, 100, 300, 5, 3) };
	const uint64_t oneRelems[1] = { 5 };
	CHECK(vgx_tmpl_plan_batch(csz, one, 1, 7, nullptr, oneRelems, p));
	CHECK((p.cnt == std::vector<uint64_t>{ 7 }) && sizesAre(p.total, 70, 14, 35, 700, 2100, 7, 140, 350, 210) && p.numWg == 21 && p.relemWords == 35);
	CHECK(p.inst.empty() && p.wg.empty());
	vgx_sizes z = sizesOf(1, 1, 1, 1, 1, 1, 1, 1, 1);
	vgx_tmpl_add_instances(z, 3, csz[1]);
	CHECK(sizesAre(z, 34, 10, 10, 211, 601, 1, 67, 121, 46));
	// refused from 2^32 meshes on, not one below
	const VgxTmplClass two[3] = { classAt(0, 0, 0, 0, 0), classAt(0, 0, 0, 0, 1), classAt(0, 0, 0, 0, 2) };
	const uint32_t each[2] = { 0, 1 };
	vgx_sizes m[2] = { sizesOf(0, 0, 1ull << 31, 0, 0, 0, 0, 0, 0), sizesOf(0, 0, (1ull << 31) - 1, 0, 0, 0, 0, 0, 0) };
	CHECK(vgx_tmpl_plan_batch(m, two, 2, 2, each, nullptr, p) && p.total.num_meshes == (1ull << 32) - 1 && p.wg.size() == 2);
	m[1].num_meshes = 1ull << 31;
	CHECK(!vgx_tmpl_plan_batch(m, two, 2, 2, each, nullptr, p) && p.inst.empty() && p.wg.empty());
	// refused beyond 2^31 - 1 workgroups, not at it (the totals alone: the table of the accepted case would be 16 GB)
	VgxTmplClass wide[3] = { classAt(0, 0, 0, 0, 0), classAt(0, 0, 0, 0, 0x40000000u), classAt(0, 0, 0, 0, 0x7FFFFFFFu) };
	CHECK(vgx_tmpl_plan_totals(csz, wide, 2, 2, each, nullptr, p) && p.numWg == 0x7FFFFFFFull);
	wide[2].tile0 = 0x80000000u;
	CHECK(!vgx_tmpl_plan_totals(csz, wide, 2, 2, each, nullptr, p) && p.numWg == 0x80000000ull);
	CHECK(!vgx_tmpl_plan_batch(csz, wide, 2, 2, each, nullptr, p) && p.wg.empty());
	CHECK(vgx_tmpl_plan_totals(csz, wide, 1, 4, nullptr, nullptr, p) && p.numWg == 0x100000000ull); // one class: the step checks its own grid
}

int main()
{
	testKernelAndTile();
	testEligible();
	testGrouping();
	testClassSizes();
	testRoundLayout();
	testBatchPlan();
	if (failures) { printf("%d checks failed\n", failures); return 1; }
	printf("ok\n");
	return 0;
}
