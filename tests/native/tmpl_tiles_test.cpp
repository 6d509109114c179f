// tmpl_tiles_test.cpp -- template mode's tile boundaries (vg-renderer_amd/csrc/vgx_tmpl_plan.h: snap limit, stride, nominal boundary,
// snap decision): the functions k_tmpl_mesh_lmax / k_tmpl_classes / k_tmpl_elems run on the device, here on random lists of mesh lengths.
// Host only; prints "ok" and returns 0, or names the first check that failed. Built and run by tests/test_tmpl_tiles_host.py. Every
// boundary is found the way the device finds it: on its own, from the mesh that owns the nominal place; small classes also walk the
// greedy packing of k_tmpl_classes.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include <algorithm>

#include "vgx_tmpl_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!failures++) { printf("FAILED %s:%d: %s (T=%u case=%d)\n", __FILE__, __LINE__, #c, curT, curCase); } } } while (0)
static uint32_t curT = 0;
static int curCase = 0;

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17;
	return (uint32_t)(rngState >> 32);
}
static uint32_t rndIn(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); } // inclusive

// one class: meshes of the given lengths, the first one beginning at element elem0
static void checkClass(uint32_t T, const std::vector<uint32_t>& lens, uint64_t elem0)
{
	const uint32_t L = vgx_tmpl_snap_limit(T);
	CHECK(L == T / 8);
	std::vector<uint64_t> first(lens.size() + 1);
	first[0] = elem0;
	uint32_t lmax = 0; // what k_tmpl_mesh_lmax leaves: the maximum of the meshes' contributions
	for (size_t m = 0; m < lens.size(); ++m) {
		first[m + 1] = first[m] + lens[m];
		lmax = std::max(lmax, vgx_tmpl_snap_len(lens[m], T));
		CHECK(vgx_tmpl_snap_len(lens[m], T) == (lens[m] <= L ? lens[m] : 0u));
	}
	const uint64_t end = first[lens.size()], E = end - elem0;
	const uint32_t S = vgx_tmpl_stride(T, lmax);
	// the stride as the rule states it: T - (Lmax - 1), Lmax = the longest mesh of at most L elements, or 1
	uint32_t longestShort = 1;
	for (uint32_t n : lens) { if (n <= L && n > longestShort) { longestShort = n; } }
	CHECK(S == T - (longestShort - 1));
	CHECK(S >= 1 && S <= T);
	const uint64_t nt = vgx_tmpl_tile_count(E, S);
	CHECK(nt == (E + S - 1) / S);                              // the closed form
	CHECK(nt <= vgx_tmpl_max_tiles(E, T, 1));                  // what the tables are sized for
	std::vector<uint64_t> b((size_t)nt + 1);
	for (uint64_t k = 0; k <= nt; ++k) {
		const uint64_t nom = vgx_tmpl_nominal_boundary(elem0, end, k, S);
		CHECK(nom == std::min(elem0 + k * S, end));
		if (nom >= end) { b[(size_t)k] = end; continue; }      // (the class's end: no mesh of the class owns it)
		const size_t m = (size_t)(std::upper_bound(first.begin(), first.end(), nom) - first.begin()) - 1; // the mesh that owns element nom
		b[(size_t)k] = vgx_tmpl_snap_boundary(nom, first[m], lens[m], T);
		CHECK(b[(size_t)k] == nom || (b[(size_t)k] == first[m] && lens[m] <= L));
		if (lens[m] > L) { CHECK(b[(size_t)k] == nom); }       // a long mesh is cut where the boundary falls
	}
	CHECK(nt == 0 || (b[0] == elem0 && b[(size_t)nt] == end)); // the tiles partition the class's elements ...
	if (nt == 0) { CHECK(E == 0); }
	for (uint64_t k = 0; k < nt; ++k) {
		CHECK(b[(size_t)k] < b[(size_t)k + 1]);                // ... boundaries strictly increasing
		CHECK(b[(size_t)k + 1] - b[(size_t)k] <= T);           // no tile beyond its slots
	}
	// no boundary strictly inside a mesh of at most L elements
	for (uint64_t k = 0; k <= nt; ++k) {
		if (b[(size_t)k] >= end) { continue; }
		const size_t m = (size_t)(std::upper_bound(first.begin(), first.end(), b[(size_t)k]) - first.begin()) - 1;
		CHECK(!(first[m] < b[(size_t)k] && lens[m] <= L));
	}
	// small classes: the greedy walk (k_tmpl_classes' loop) -- the same invariants, never more tiles than the stride rule
	CHECK(vgx_tmpl_greedy_class(lens.size(), E, T) == (lens.size() <= 4096 && E <= 64ull * (T - L)));
	if (!vgx_tmpl_greedy_class(lens.size(), E, T)) { return; }
	std::vector<uint64_t> g;
	for (uint64_t at = elem0; at < end;) {
		g.push_back(at);
		const uint64_t nom = vgx_tmpl_greedy_nominal(at, end, T);
		CHECK(nom == std::min(at + T, end));
		if (nom >= end) { break; }
		const size_t m = (size_t)(std::upper_bound(first.begin(), first.end(), nom) - first.begin()) - 1;
		const uint64_t nx = vgx_tmpl_snap_boundary(nom, first[m], lens[m], T);
		CHECK(nx > at && nx - at <= T);
		CHECK(!(first[m] < nx && lens[m] <= L));
		if (nx <= at) { break; }
		at = nx;
	}
	CHECK(g.size() <= nt && g.size() <= 65);
	if (E) { CHECK(g[0] == elem0 && end - g.back() <= T && end > g.back()); }
}

int main()
{
	const uint32_t tiles[] = { 64, 128, 2048 };
	for (uint32_t T : tiles) {
		curT = T;
		const uint32_t L = T / 8;
		const uint32_t edge[] = { L - 1, L, L + 1, T - 1, T, T + 1, 2, 3 * T };
		for (curCase = 0; curCase < 600; ++curCase) {
			const int mix = curCase % 3; // 0: short meshes only, 1: long meshes only, 2: both
			const uint32_t count = curCase < 6 ? (uint32_t)curCase / 3 : rndIn(1, curCase % 7 == 0 ? 3000 : 200);
			std::vector<uint32_t> lens;
			for (uint32_t i = 0; i < count; ++i) {
				uint32_t n;
				const bool isShort = mix == 0 || (mix == 2 && (rnd() & 1u));
				if (isShort) { n = rndIn(2, L); } else { n = rndIn(L + 1, 3 * T); }
				if (rnd() % 5 == 0) { // the lengths around the limit and the tile, where the mix allows them
					const uint32_t e = edge[rnd() % 8];
					if (e >= 2 && (mix == 2 || (mix == 0) == (e <= L))) { n = e; }
				}
				lens.push_back(n);
			}
			checkClass(T, lens, curCase % 2 ? 0 : rndIn(0, 100000)); // (a later class of a template begins anywhere)
		}
		// every edge length on its own and repeated
		for (uint32_t e : edge) {
			if (e < 2) { continue; }
			curCase = 1000 + (int)e;
			checkClass(T, std::vector<uint32_t>(1, e), 0);
			checkClass(T, std::vector<uint32_t>(37, e), 5);
		}
	}
	if (failures) { printf("%d checks failed\n", failures); return 1; }
	printf("ok\n");
	return 0;
}
