// vgx_marquee_example.cpp -- pick tolerance and marquee (rubber-band) selection on the device, through the C-ABI (no Python, no torch).
// One drawing of closed rings and one hairline (an AAThin stroke) tessellated ONCE, ONE frame of 8 x 8 instances of the drawing and one
// of the hairline (vgx_cache_submit). Then
//   vgx_pick           a cursor 1.6 units beside the hairline: the point test misses it
//   vgx_pick_rect      the same cursor as a +-2-unit square: the hairline's instance answers
//   vgx_pick_rect      one marquee, as a crossing and as a window selection, VGX_PICK_RECT_BY_DRAW: one entry per instance
//   vgx_cache_update   the instances the marquee crosses recoloured, those wholly inside it in another colour
//   vgx_raster         the frame as an image, written as a PPM
// Every selection is checked against a plain host loop over the downloaded frame (the rule of include/vgx.h in its four-corner form).
//   hipcc -O2 -I include examples/vgx_marquee_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_marquee_example
//   ./vgx_marquee_example [out.ppm]
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

// The rule of include/vgx.h for one triangle and one valid rectangle: the box overlap in binary32, then per edge "some corner of the
// rectangle lies on the triangle's side" in binary64 without FMA.
static bool touches(const float* a, const float* b, const float* c, const vgx_pick_rect_query& q)
{
#pragma clang fp contract(off)
	const float lox = fminf(fminf(a[0], b[0]), c[0]), hix = fmaxf(fmaxf(a[0], b[0]), c[0]);
	const float loy = fminf(fminf(a[1], b[1]), c[1]), hiy = fmaxf(fmaxf(a[1], b[1]), c[1]);
	if (!(q.x1 >= lox && q.x0 <= hix && q.y1 >= loy && q.y0 <= hiy)) { return false; }
	const double P[3][2] = { { a[0], a[1] }, { b[0], b[1] }, { c[0], c[1] } };
	const double A = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0]);
	if (!(A > 0.0) && !(A < 0.0)) { return false; }
	const double X[4] = { q.x0, q.x1, q.x1, q.x0 }, Y[4] = { q.y0, q.y0, q.y1, q.y1 };
	for (int k = 0; k < 3; ++k) {
		const double* u = P[k];
		const double* v = P[(k + 1) % 3];
		bool pass = false;
		for (int n = 0; n < 4; ++n) {
			const double e = (v[0] - u[0]) * (Y[n] - u[1]) - (v[1] - u[1]) * (X[n] - u[0]);
			pass = pass || (A > 0.0 ? e >= 0.0 : e <= 0.0);
		}
		if (!pass) { return false; }
	}
	return true;
}

// The instances (runs of equal vgx_mesh::draw) a rectangle selects, by their first mesh: crossing, or window with the boxes of the frame
static std::vector<uint32_t> hostSelect(const std::vector<float>& pos, const std::vector<uint16_t>& idx, const std::vector<vgx_mesh>& meshes, const vgx_pick_rect_query& q)
{
	std::vector<uint32_t> sel;
	for (size_t m = 0; m < meshes.size();) {
		size_t end = m + 1;
		while (end < meshes.size() && meshes[end].draw == meshes[m].draw) { ++end; }
		bool touch = false, inside = true;
		for (size_t j = m; j < end; ++j) {
			const vgx_mesh& me = meshes[j];
			const float* p = pos.data() + 2 * me.first_vertex;
			const uint16_t* ip = idx.data() + me.first_index;
			for (uint32_t v = 0; v < me.num_vertices; ++v) { inside = inside && p[2 * v] >= q.x0 && p[2 * v] <= q.x1 && p[2 * v + 1] >= q.y0 && p[2 * v + 1] <= q.y1; }
			for (uint32_t t = 0; t < me.num_indices / 3 && !touch; ++t) {
				const uint32_t i0 = ip[3 * t], i1 = ip[3 * t + 1], i2 = ip[3 * t + 2];
				if (i0 >= me.num_vertices || i1 >= me.num_vertices || i2 >= me.num_vertices) { continue; }
				touch = touches(p + 2 * i0, p + 2 * i1, p + 2 * i2, q);
			}
		}
		if (touch && (!(q.flags & VGX_PICK_RECT_WINDOW) || inside)) { sel.push_back((uint32_t)m); }
		m = end;
	}
	return sel;
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_marquee_example.ppm";
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));

	// the drawing: 40 closed rings inside a 100 x 100 box; behind them one more path, a hairline of 80 units
	const uint32_t nrings = 40, npaths = nrings + 1;
	const float drawingSize = 100.0f;
	std::vector<uint8_t> cmdType;
	std::vector<uint32_t> cmdArgOff(1, 0u), pathCmdBegin(1, 0u);
	std::vector<float> args;
	uint32_t seed = 77u;
	for (uint32_t p = 0; p < nrings; ++p) {
		const uint32_t n = 8 + rnd(seed) % 17;
		const float r = 4.0f + (float)(rnd(seed) % 12);
		const float cx = r + (float)(rnd(seed) % (uint32_t)(drawingSize - 2.0f * r)), cy = r + (float)(rnd(seed) % (uint32_t)(drawingSize - 2.0f * r));
		for (uint32_t k = 0; k < n; ++k) {
			const float a = 6.2831853f * (float)k / (float)n;
			cmdType.push_back(k == 0 ? VGX_CMD_MOVE_TO : VGX_CMD_LINE_TO);
			args.push_back(cx + r * cosf(a)); args.push_back(cy + r * sinf(a));
			cmdArgOff.push_back((uint32_t)args.size());
		}
		cmdType.push_back(VGX_CMD_CLOSE); cmdArgOff.push_back((uint32_t)args.size());
		pathCmdBegin.push_back((uint32_t)cmdType.size());
	}
	cmdType.push_back(VGX_CMD_MOVE_TO); args.push_back(10.0f); args.push_back(50.0f); cmdArgOff.push_back((uint32_t)args.size());
	cmdType.push_back(VGX_CMD_LINE_TO); args.push_back(90.0f); args.push_back(53.0f); cmdArgOff.push_back((uint32_t)args.size());
	pathCmdBegin.push_back((uint32_t)cmdType.size());
	vgx_pathset_desc desc = { cmdType.data(), cmdArgOff.data(), args.data(), pathCmdBegin.data(), npaths, (uint32_t)cmdType.size() };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	std::vector<vgx_draw> draws(npaths);
	for (uint32_t p = 0; p < npaths; ++p) {
		vgx_draw d;
		memset(&d, 0, sizeof(d));
		d.path = p;
		if (p < nrings) { d.fill_flags = VGX_FILL_ENABLE; d.fill_color = 0xFF000000u | (0x404040u + (rnd(seed) & 0x7F7F7Fu)); }
		else { d.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 1); d.stroke_color = 0xFF000000u; d.stroke_width = 1.0f; }
		d.scale = 1.0f; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = 1.0f; d.mtx[3] = 1.0f;
		draws[p] = d;
	}
	vgx_draw* devDraws = nullptr;
	if (hipMalloc(&devDraws, npaths * sizeof(vgx_draw)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), npaths * sizeof(vgx_draw), hipMemcpyHostToDevice);

	// record: tessellate once, localize; the hairline's meshes are the last draw's
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
	std::vector<vgx_mesh> cmeshes(sz.num_meshes);
	if (hipMemcpy(cmeshes.data(), rec.meshes, cmeshes.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	uint32_t ringMeshes = 0;
	while (ringMeshes < cmeshes.size() && cmeshes[ringMeshes].draw < nrings) { ++ringMeshes; }
	if (ringMeshes == 0 || ringMeshes == cmeshes.size()) { fprintf(stderr, "the cache has no rings or no hairline\n"); return 1; }

	// the frame: the rings on a grid of pitch 1.25 of their size, the hairline to the right of the grid
	const uint32_t grid = 8, ninst = grid * grid + 1, hairline = grid * grid;
	const float pitch = 1.25f * drawingSize;
	std::vector<vgx_cache_instance> inst(ninst);
	for (uint32_t i = 0; i < ninst; ++i) {
		vgx_cache_instance& in = inst[i];
		memset(&in, 0, sizeof(in));
		in.color = 0xFFFFFFFFu;
		in.mtx[0] = 1.0f; in.mtx[3] = 1.0f;
		if (i < hairline) { in.first_mesh = 0; in.num_meshes = ringMeshes; in.mtx[4] = pitch * (float)(i % grid); in.mtx[5] = pitch * (float)(i / grid); }
		else { in.first_mesh = ringMeshes; in.num_meshes = (uint32_t)sz.num_meshes - ringMeshes; in.mtx[4] = pitch * (float)grid; in.mtx[5] = 0.0f; }
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
	printf("frame: %u instances -> %llu meshes, %llu vertices, %llu indices in device memory\n", ninst, (unsigned long long)got.num_meshes,
		(unsigned long long)got.num_vertices, (unsigned long long)got.num_indices);
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, got.num_meshes, got.num_vertices, got.num_indices };
	vgx_cache_slot* devSlots = nullptr; float* devBounds = nullptr;
	(void)hipMalloc(&devSlots, (ninst + 1) * sizeof(vgx_cache_slot));
	if (hipMalloc(&devBounds, got.num_meshes * 4 * sizeof(float)) != hipSuccess) { return 1; }
	CHECK(vgx_cache_layout(ctx, &cache, devInst, ninst, devSlots, devStatus, nullptr));
	CHECK(vgx_mesh_bounds(ctx, out.pos, out.meshes, got.num_meshes, devBounds, nullptr));
	std::vector<float> hpos(2 * got.num_vertices);
	std::vector<uint16_t> hidx(got.num_indices);
	std::vector<vgx_mesh> hmeshes(got.num_meshes);
	(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
	(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
	if (hipMemcpy(hmeshes.data(), out.meshes, hmeshes.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }

	// pick tolerance: a cursor 1.6 units beside the middle of the hairline (its two fringes reach one unit to either side)
	const float cx = pitch * (float)grid + 50.0f, cy = 51.5f + 1.6f;
	vgx_pick_query pq = { cx, cy, 0xFFFFFFFFu, 0u };
	vgx_pick_query* devPQ = nullptr; vgx_pick_hit* devHits = nullptr;
	(void)hipMalloc(&devPQ, sizeof(pq));
	if (hipMalloc(&devHits, 4 * sizeof(vgx_pick_hit)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devPQ, &pq, sizeof(pq), hipMemcpyHostToDevice);
	CHECK(vgx_pick(ctx, &frame, devBounds, devPQ, 1, devHits, nullptr));
	vgx_pick_hit pointHit;
	(void)hipMemcpy(&pointHit, devHits, sizeof(pointHit), hipMemcpyDeviceToHost);

	// the same cursor as a square, and the marquee as a crossing and as a window selection, in one call
	const uint32_t cap = 64;
	vgx_pick_rect_query rq[3];
	memset(rq, 0, sizeof(rq));
	rq[0].x0 = cx - 2.0f; rq[0].y0 = cy - 2.0f; rq[0].x1 = cx + 2.0f; rq[0].y1 = cy + 2.0f; rq[0].mesh_end = 0xFFFFFFFFu; rq[0].flags = VGX_PICK_RECT_BY_DRAW;
	rq[1].x0 = 1.5f * pitch; rq[1].y0 = 1.5f * pitch; rq[1].x1 = 4.4f * pitch; rq[1].y1 = 3.4f * pitch; rq[1].mesh_end = 0xFFFFFFFFu; rq[1].flags = VGX_PICK_RECT_BY_DRAW;
	rq[2] = rq[1]; rq[2].flags |= VGX_PICK_RECT_WINDOW;
	vgx_pick_rect_query* devRQ = nullptr;
	vgx_pick_rect_out ro;
	memset(&ro, 0, sizeof(ro));
	ro.list_cap = cap;
	(void)hipMalloc(&devRQ, sizeof(rq));
	(void)hipMalloc(&ro.top, 3 * sizeof(vgx_pick_hit));
	(void)hipMalloc(&ro.list, 3 * cap * sizeof(uint32_t));
	if (hipMalloc(&ro.count, 3 * sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devRQ, rq, sizeof(rq), hipMemcpyHostToDevice);
	CHECK(vgx_pick_rect(ctx, &frame, devBounds, devRQ, 3, &ro, nullptr));
	vgx_pick_hit tops[3]; uint32_t counts[3];
	std::vector<uint32_t> lists(3 * cap);
	(void)hipMemcpy(tops, ro.top, sizeof(tops), hipMemcpyDeviceToHost);
	(void)hipMemcpy(counts, ro.count, sizeof(counts), hipMemcpyDeviceToHost);
	if (hipMemcpy(lists.data(), ro.list, lists.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	printf("cursor (%.1f, %.1f): the point pick finds %s, the +-2 square instance %u (%u entr%s)\n", cx, cy, pointHit.mesh == 0xFFFFFFFFu ? "nothing" : "a mesh",
		tops[0].draw, counts[0], counts[0] == 1 ? "y" : "ies");
	uint32_t wrong = 0;
	wrong += pointHit.mesh != 0xFFFFFFFFu;
	wrong += counts[0] != 1 || tops[0].draw != hairline;
	for (int k = 0; k < 3; ++k) {
		const std::vector<uint32_t> want = hostSelect(hpos, hidx, hmeshes, rq[k]);
		bool same = counts[k] == want.size() && counts[k] <= cap;
		for (size_t i = 0; same && i < want.size(); ++i) { same = lists[k * cap + i] == want[i]; }
		wrong += same ? 0u : 1u;
	}
	printf("marquee (%.0f, %.0f)-(%.0f, %.0f): %u instances crossed, %u wholly inside\n", rq[1].x0, rq[1].y0, rq[1].x1, rq[1].y1, counts[1], counts[2]);
	wrong += !(counts[2] > 0 && counts[2] < counts[1]);

	// recolour: crossed instances red, those wholly inside green; the entries name an instance by its first mesh
	std::vector<uint32_t> dirty;
	for (uint32_t i = 0; i < counts[1] && i < cap; ++i) { const uint32_t k = hmeshes[lists[cap + i]].draw; inst[k].color = 0xFF4040FFu; dirty.push_back(k); }
	for (uint32_t i = 0; i < counts[2] && i < cap; ++i) { inst[hmeshes[lists[2 * cap + i]].draw].color = 0xFF40C040u; }
	(void)hipMemcpy(devInst, inst.data(), ninst * sizeof(vgx_cache_instance), hipMemcpyHostToDevice);
	uint32_t* devDirty = nullptr;
	if (hipMalloc(&devDirty, (dirty.size() + 1) * sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDirty, dirty.data(), dirty.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
	vgx_update_frame uf;
	uf.pos = out.pos; uf.color = out.color; uf.num_vertices = got.num_vertices; uf.num_meshes = got.num_meshes; uf.mesh_bounds = devBounds;
	CHECK(vgx_cache_update(ctx, &cache, devInst, ninst, devSlots, devDirty, dirty.size(), nullptr, &uf, devStatus, nullptr));
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	if (status != VGX_OK) { fprintf(stderr, "update: %s\n", vgx_status_string((int)status)); return 1; }

	// the picture
	const uint32_t width = (uint32_t)(pitch * (float)(grid + 1)), height = (uint32_t)(pitch * (float)grid);
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFFFFFFFu;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	status = VGX_E_GROWN;
	for (uint32_t calls = 0; status == VGX_E_GROWN && calls < 3; ++calls) {
		CHECK(vgx_raster(ctx, &frame, devBounds, 0, got.num_meshes, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster: %s\n", vgx_status_string((int)status)); return 1; }
	std::vector<uint32_t> pixels((size_t)width * height);
	if (hipMemcpy(pixels.data(), tgt.pixels, pixels.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	std::vector<uint8_t> rgb(pixels.size() * 3);
	uint32_t painted = 0;
	for (size_t k = 0; k < pixels.size(); ++k) {
		const uint32_t c = pixels[k];
		rgb[3 * k] = (uint8_t)c; rgb[3 * k + 1] = (uint8_t)(c >> 8); rgb[3 * k + 2] = (uint8_t)(c >> 16);
		painted += c != 0xFFFFFFFFu;
	}
	FILE* f = fopen(ppmPath, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppmPath); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	fwrite(rgb.data(), 1, rgb.size(), f);
	fclose(f);
	printf("recoloured %zu instances, rendered %u x %u (%u pixels painted) to %s; %u answers differ from the host loop\n", dirty.size(), width, height, painted, ppmPath, wrong);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return wrong == 0 && painted > 0 ? 0 : 1;
}
