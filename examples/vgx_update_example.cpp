// vgx_update_example.cpp -- drag and recolour the drawing under the cursor without submitting the frame again, through the C-ABI (no
// Python, no torch). The overlapping cached grid of vgx_pick_example.cpp (every other fill non-AA here, so that the instance's colour
// shows): one drawing tessellated ONCE, ONE frame of 12 x 12 instances (vgx_cache_submit). Then
//   vgx_cache_layout   where every instance lives in the frame; vgx_mesh_bounds: the frame's box table, computed once
//   vgx_pick           the instance under a cursor, and the one beneath it
//   vgx_cache_update   the hit instance translated and recoloured: its slice of pos / color rewritten, its boxes refreshed
//   vgx_pick           at the old position the drawing beneath answers, at the new one the moved drawing
// Every pick is checked against a plain host loop over the downloaded frame, the updated frame and box table against a fresh
// vgx_cache_submit / vgx_mesh_bounds of the edited array.
//   hipcc -O2 -I include examples/vgx_update_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_update_example
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vgx.h"

#define CHECK(call)                                                                        \
	do {                                                                                   \
		const int st_ = (call);                                                            \
		if (st_ != VGX_OK) {                                                               \
			fprintf(stderr, "%s failed: %s (%d)\n", #call, vgx_status_string(st_), st_); \
			return 1;                                                                      \
		}                                                                                  \
	} while (0)

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// The rule of include/vgx.h for one triangle: the closed box in binary32, the edge expressions in binary64 without FMA.
static bool hitTriangle(const float* a, const float* b, const float* c, float px, float py)
{
#pragma clang fp contract(off)
	const float lox = fminf(fminf(a[0], b[0]), c[0]), hix = fmaxf(fmaxf(a[0], b[0]), c[0]);
	const float loy = fminf(fminf(a[1], b[1]), c[1]), hiy = fmaxf(fmaxf(a[1], b[1]), c[1]);
	if (!(px >= lox && px <= hix && py >= loy && py <= hiy)) { return false; }
	const double ax = a[0], ay = a[1], bx = b[0], by = b[1], cx = c[0], cy = c[1], x = px, y = py;
	const double A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
	const double e0 = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
	const double e1 = (cx - bx) * (y - by) - (cy - by) * (x - bx);
	const double e2 = (ax - cx) * (y - cy) - (ay - cy) * (x - cx);
	if (A > 0.0) { return e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0; }
	if (A < 0.0) { return e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0; }
	return false;
}

// The whole frame on the host, mesh after mesh: the last hit triangle of the last hit mesh below meshEnd.
static vgx_pick_hit hostPick(const std::vector<float>& pos, const std::vector<uint16_t>& idx, const std::vector<vgx_mesh>& meshes, vgx_pick_query q)
{
	vgx_pick_hit h = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
	for (size_t m = 0; m < meshes.size() && m < (size_t)q.mesh_end; ++m) {
		const vgx_mesh& me = meshes[m];
		const float* p = pos.data() + 2 * me.first_vertex;
		const uint16_t* ip = idx.data() + me.first_index;
		for (uint32_t t = 0; t < me.num_indices / 3; ++t) {
			const uint32_t i0 = ip[3 * t], i1 = ip[3 * t + 1], i2 = ip[3 * t + 2];
			if (i0 >= me.num_vertices || i1 >= me.num_vertices || i2 >= me.num_vertices) { continue; }
			if (hitTriangle(p + 2 * i0, p + 2 * i1, p + 2 * i2, q.x, q.y)) { h.mesh = (uint32_t)m; h.triangle = t; h.draw = me.draw; h.subpath_kind = me.subpath_kind; }
		}
	}
	return h;
}

int main()
{
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));

	// the drawing: 120 closed rings of 8-40 points inside a 400 x 400 box
	const uint32_t npaths = 120;
	const float drawingSize = 400.0f;
	std::vector<uint8_t> cmdType;
	std::vector<uint32_t> cmdArgOff(1, 0u), pathCmdBegin(1, 0u);
	std::vector<float> args;
	uint32_t seed = 2024u;
	for (uint32_t p = 0; p < npaths; ++p) {
		const uint32_t n = 8 + rnd(seed) % 33;
		const float r = 8.0f + (float)(rnd(seed) % 40);
		const float cx = r + (float)(rnd(seed) % (uint32_t)(drawingSize - 2.0f * r)), cy = r + (float)(rnd(seed) % (uint32_t)(drawingSize - 2.0f * r));
		for (uint32_t k = 0; k < n; ++k) {
			const float a = 6.2831853f * (float)k / (float)n, rr = r * (0.6f + 0.4f * (float)(rnd(seed) % 100) / 100.0f);
			cmdType.push_back(k == 0 ? VGX_CMD_MOVE_TO : VGX_CMD_LINE_TO);
			args.push_back(cx + rr * cosf(a)); args.push_back(cy + rr * sinf(a));
			cmdArgOff.push_back((uint32_t)args.size());
		}
		cmdType.push_back(VGX_CMD_CLOSE); cmdArgOff.push_back((uint32_t)args.size());
		pathCmdBegin.push_back((uint32_t)cmdType.size());
	}
	vgx_pathset_desc desc = { cmdType.data(), cmdArgOff.data(), args.data(), pathCmdBegin.data(), npaths, (uint32_t)cmdType.size() };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	std::vector<vgx_draw> draws(npaths);
	for (uint32_t p = 0; p < npaths; ++p) {
		vgx_draw d;
		memset(&d, 0, sizeof(d));
		d.path = p;
		d.fill_flags = VGX_FILL_ENABLE | (p % 2 ? VGX_FILL_AA : 0u); d.fill_color = 0xFF000000u | rnd(seed);
		if (p % 3 == 0) { d.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0); d.stroke_color = 0xFF000000u | rnd(seed); d.stroke_width = 2.0f; }
		d.scale = 1.0f; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = 1.0f; d.mtx[3] = 1.0f;
		draws[p] = d;
	}
	vgx_draw* devDraws = nullptr;
	if (hipMalloc(&devDraws, npaths * sizeof(vgx_draw)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), npaths * sizeof(vgx_draw), hipMemcpyHostToDevice);

	// record: tessellate once, localize
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, npaths, &sz, nullptr));
	vgx_mesh_out rec;
	memset(&rec, 0, sizeof(rec));
	rec.cap_vertices = sz.num_vertices; rec.cap_indices = sz.num_indices; rec.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&rec.pos, rec.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&rec.color, rec.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&rec.idx, rec.cap_indices * sizeof(uint16_t));
	if (hipMalloc(&rec.meshes, rec.cap_meshes * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, npaths, &rec, nullptr));
	CHECK(vgx_cache_localize(ctx, devDraws, npaths, rec.pos, rec.meshes, sz.num_meshes, nullptr));
	const vgx_cache_desc cache = { rec.pos, rec.color, rec.idx, rec.meshes, sz.num_meshes, sz.num_vertices, sz.num_indices };

	// the frame: the drawing on a grid whose pitch is 0.6 of its size, so that every drawing lies over its left and upper neighbours
	const uint32_t grid = 12, ninst = grid * grid;
	const float pitch = 0.6f * drawingSize;
	std::vector<vgx_cache_instance> inst(ninst);
	for (uint32_t i = 0; i < ninst; ++i) {
		vgx_cache_instance& in = inst[i];
		memset(&in, 0, sizeof(in));
		in.first_mesh = 0; in.num_meshes = (uint32_t)sz.num_meshes; in.color = 0xFFFFFFFFu;
		in.mtx[0] = 1.0f; in.mtx[3] = 1.0f; in.mtx[4] = pitch * (float)(i % grid); in.mtx[5] = pitch * (float)(i / grid);
	}
	vgx_cache_instance* devInst = nullptr;
	(void)hipMalloc(&devInst, ninst * sizeof(vgx_cache_instance));
	(void)hipMemcpy(devInst, inst.data(), ninst * sizeof(vgx_cache_instance), hipMemcpyHostToDevice);
	vgx_mesh_out out;
	memset(&out, 0, sizeof(out));
	out.cap_vertices = sz.num_vertices * ninst; out.cap_indices = sz.num_indices * ninst; out.cap_meshes = sz.num_meshes * ninst;
	(void)hipMalloc(&out.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out.color, out.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, out.cap_indices * sizeof(uint16_t));
	(void)hipMalloc(&out.meshes, out.cap_meshes * sizeof(vgx_mesh));
	vgx_sizes* devSizes = nullptr; uint32_t* devStatus = nullptr;
	(void)hipMalloc(&devSizes, sizeof(vgx_sizes));
	if (hipMalloc(&devStatus, sizeof(uint32_t)) != hipSuccess) { return 1; }
	CHECK(vgx_cache_submit(ctx, &cache, devInst, ninst, &out, devSizes, devStatus, nullptr));
	uint32_t status = 0; vgx_sizes got;
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&got, devSizes, sizeof(got), hipMemcpyDeviceToHost);
	if (status != VGX_OK) { fprintf(stderr, "submit: %s\n", vgx_status_string((int)status)); return 1; }
	printf("frame: %u instances of %llu meshes -> %llu meshes, %llu vertices, %llu indices in device memory\n", ninst,
		(unsigned long long)sz.num_meshes, (unsigned long long)got.num_meshes, (unsigned long long)got.num_vertices, (unsigned long long)got.num_indices);
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, got.num_meshes, got.num_vertices, got.num_indices };

	// where the instances live, and the frame's boxes: both once per submit
	vgx_cache_slot* devSlots = nullptr; float* devBounds = nullptr;
	(void)hipMalloc(&devSlots, (ninst + 1) * sizeof(vgx_cache_slot));
	if (hipMalloc(&devBounds, got.num_meshes * 4 * sizeof(float)) != hipSuccess) { return 1; }
	CHECK(vgx_cache_layout(ctx, &cache, devInst, ninst, devSlots, devStatus, nullptr));
	CHECK(vgx_mesh_bounds(ctx, out.pos, out.meshes, got.num_meshes, devBounds, nullptr));
	std::vector<vgx_cache_slot> slots(ninst + 1);
	(void)hipMemcpy(slots.data(), devSlots, slots.size() * sizeof(vgx_cache_slot), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	if (status != VGX_OK || slots[ninst].first_vertex != got.num_vertices || slots[ninst].first_mesh != got.num_meshes) { fprintf(stderr, "layout disagrees with the submit\n"); return 1; }

	std::vector<float> hpos(2 * got.num_vertices);
	std::vector<uint32_t> hcol(got.num_vertices);
	std::vector<uint16_t> hidx(got.num_indices);
	std::vector<vgx_mesh> hmeshes(got.num_meshes);
	(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
	(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
	if (hipMemcpy(hmeshes.data(), out.meshes, hmeshes.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }

	// the cursor: the first of a few positions that has a drawing under the hit one
	vgx_pick_query* devQ = nullptr; vgx_pick_hit* devHits = nullptr;
	(void)hipMalloc(&devQ, 2 * sizeof(vgx_pick_query));
	if (hipMalloc(&devHits, 2 * sizeof(vgx_pick_hit)) != hipSuccess) { return 1; }
	uint32_t wrong = 0;
	vgx_pick_query cur; vgx_pick_hit top, under;
	memset(&top, 0xFF, sizeof(top)); memset(&under, 0xFF, sizeof(under));
	for (uint32_t k = 0; k < 16 && under.mesh == 0xFFFFFFFFu; ++k) {
		cur.x = pitch * (1.0f + (float)(rnd(seed) % 900) / 100.0f); cur.y = pitch * (1.0f + (float)(rnd(seed) % 900) / 100.0f);
		cur.mesh_end = 0xFFFFFFFFu; cur.flags = 0;
		(void)hipMemcpy(devQ, &cur, sizeof(cur), hipMemcpyHostToDevice);
		CHECK(vgx_pick(ctx, &frame, devBounds, devQ, 1, devHits, nullptr));
		(void)hipMemcpy(&top, devHits, sizeof(top), hipMemcpyDeviceToHost);
		const vgx_pick_hit w = hostPick(hpos, hidx, hmeshes, cur);
		wrong += memcmp(&w, &top, sizeof(w)) != 0;
		if (top.mesh == 0xFFFFFFFFu) { continue; }
		vgx_pick_query below = cur;
		below.mesh_end = (uint32_t)slots[top.draw].first_mesh; // everything in front of the hit instance's first frame mesh
		(void)hipMemcpy(devQ, &below, sizeof(below), hipMemcpyHostToDevice);
		CHECK(vgx_pick(ctx, &frame, devBounds, devQ, 1, devHits, nullptr));
		(void)hipMemcpy(&under, devHits, sizeof(under), hipMemcpyDeviceToHost);
		const vgx_pick_hit w1 = hostPick(hpos, hidx, hmeshes, below);
		wrong += memcmp(&w1, &under, sizeof(w1)) != 0;
	}
	if (under.mesh == 0xFFFFFFFFu) { fprintf(stderr, "no cursor with two drawings under it\n"); return 1; }
	const uint32_t hit = top.draw;
	printf("cursor (%.1f, %.1f): instance %u, under it instance %u\n", cur.x, cur.y, hit, under.draw);

	// the edit: the hit instance dragged to the right of the grid and recoloured; one record changes, one index is listed
	const float dx = pitch * (float)grid + drawingSize, dy = 0.25f * drawingSize;
	inst[hit].mtx[4] += dx; inst[hit].mtx[5] += dy; inst[hit].color = 0xFF00FF00u;
	(void)hipMemcpy(devInst + hit, &inst[hit], sizeof(vgx_cache_instance), hipMemcpyHostToDevice);
	uint32_t* devDirty = nullptr;
	if (hipMalloc(&devDirty, sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDirty, &hit, sizeof(hit), hipMemcpyHostToDevice);
	vgx_update_frame uf;
	uf.pos = out.pos; uf.color = out.color; uf.num_vertices = got.num_vertices; uf.num_meshes = got.num_meshes; uf.mesh_bounds = devBounds;
	CHECK(vgx_cache_update(ctx, &cache, devInst, ninst, devSlots, devDirty, 1, nullptr, &uf, devStatus, nullptr));
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	if (status != VGX_OK) { fprintf(stderr, "update: %s\n", vgx_status_string((int)status)); return 1; }

	// pick again, with the refreshed boxes: the old position and the new one in one call
	vgx_pick_query q2[2] = { cur, cur };
	q2[1].x += dx; q2[1].y += dy;
	vgx_pick_hit after[2];
	(void)hipMemcpy(devQ, q2, sizeof(q2), hipMemcpyHostToDevice);
	CHECK(vgx_pick(ctx, &frame, devBounds, devQ, 2, devHits, nullptr));
	(void)hipMemcpy(after, devHits, sizeof(after), hipMemcpyDeviceToHost);
	(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
	if (hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	for (int k = 0; k < 2; ++k) {
		const vgx_pick_hit w = hostPick(hpos, hidx, hmeshes, q2[k]);
		wrong += memcmp(&w, &after[k], sizeof(w)) != 0;
	}
	wrong += after[0].draw != under.draw; // the drawing that lay beneath
	wrong += after[1].draw != hit;        // the moved drawing

	// the updated frame and its boxes against a fresh submit / vgx_mesh_bounds of the edited array
	vgx_mesh_out out2 = out;
	float* devBounds2 = nullptr;
	(void)hipMalloc(&out2.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out2.color, out.cap_vertices * sizeof(uint32_t));
	if (hipMalloc(&devBounds2, got.num_meshes * 4 * sizeof(float)) != hipSuccess) { return 1; }
	out2.idx = out.idx; out2.meshes = out.meshes; // the same bytes again
	CHECK(vgx_cache_submit(ctx, &cache, devInst, ninst, &out2, devSizes, devStatus, nullptr));
	CHECK(vgx_mesh_bounds(ctx, out2.pos, out2.meshes, got.num_meshes, devBounds2, nullptr));
	std::vector<float> fpos(hpos.size()), b0(4 * got.num_meshes), b1(4 * got.num_meshes);
	std::vector<uint32_t> fcol(hcol.size());
	(void)hipMemcpy(fpos.data(), out2.pos, fpos.size() * sizeof(float), hipMemcpyDeviceToHost);
	(void)hipMemcpy(fcol.data(), out2.color, fcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
	(void)hipMemcpy(b0.data(), devBounds, b0.size() * sizeof(float), hipMemcpyDeviceToHost);
	if (hipMemcpy(b1.data(), devBounds2, b1.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	uint64_t differ = 0, recoloured = 0;
	for (size_t i = 0; i < hpos.size(); ++i) { differ += memcmp(&hpos[i], &fpos[i], 4) != 0; }
	for (size_t i = 0; i < hcol.size(); ++i) { differ += hcol[i] != fcol[i]; }
	for (size_t i = 0; i < b0.size(); ++i) { differ += memcmp(&b0[i], &b1[i], 4) != 0; }
	for (uint64_t v = slots[hit].first_vertex; v < slots[hit + 1].first_vertex; ++v) { recoloured += hcol[v] == 0xFF00FF00u; }
	const uint64_t moved = slots[hit + 1].first_vertex - slots[hit].first_vertex;
	printf("instance %u moved by (%.0f, %.0f) and recoloured: %llu of %llu vertices rewritten, %llu of them take the new colour\n", hit, dx, dy,
		(unsigned long long)moved, (unsigned long long)got.num_vertices, (unsigned long long)recoloured);
	printf("update: at the old cursor instance %u answers, at the new one instance %u; %u answers differ from the host loop, %llu words differ from a fresh submit\n",
		after[0].draw, after[1].draw, wrong, (unsigned long long)differ);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return wrong == 0 && differ == 0 && recoloured > 0 && recoloured < moved ? 0 : 1;
}
