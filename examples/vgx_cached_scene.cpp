// vgx_cached_scene.cpp -- a grid of cached drawings under a moving camera through the C-ABI (no Python, no torch): what a caller of the
// reference does with a cacheable command list (clCacheRender, src/vg.cpp:5845-6135), plus the view culling the reference does not have.
// One tiger-like drawing (120 rings, filled and stroked) is tessellated ONCE, kept in local space (vgx_cache_localize) and given its
// per-mesh boxes (vgx_mesh_bounds). A frame places it on a 24 x 24 grid under the camera's transform and runs
//   vgx_cache_cull   (instances against the canvas rectangle: culled records get num_meshes = 0, the array keeps its length)
//   vgx_cache_submit (the same array, the same count: nothing comes back from the device in between)
// and reads num_kept and the frame's totals only to print them.
//   hipcc -O2 -I include examples/vgx_cached_scene.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_cached_scene
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

int main(int argc, char** argv)
{
	const int frames = argc > 1 ? atoi(argv[1]) : 40;
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
		d.fill_flags = VGX_FILL_ENABLE | VGX_FILL_AA; d.fill_color = 0xFF000000u | rnd(seed);
		if (p % 3 == 0) { d.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0); d.stroke_color = 0xFF000000u | rnd(seed); d.stroke_width = 2.0f; }
		d.scale = 1.0f; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = 1.0f; d.mtx[3] = 1.0f;
		draws[p] = d;
	}
	vgx_draw* devDraws = nullptr;
	if (hipMalloc(&devDraws, npaths * sizeof(vgx_draw)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), npaths * sizeof(vgx_draw), hipMemcpyHostToDevice);

	// record: tessellate once, localize, boxes
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, npaths, &sz, nullptr));
	vgx_mesh_out rec;
	memset(&rec, 0, sizeof(rec));
	rec.cap_vertices = sz.num_vertices; rec.cap_indices = sz.num_indices; rec.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&rec.pos, rec.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&rec.color, rec.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&rec.idx, rec.cap_indices * sizeof(uint16_t));
	(void)hipMalloc(&rec.meshes, rec.cap_meshes * sizeof(vgx_mesh));
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, npaths, &rec, nullptr));
	CHECK(vgx_cache_localize(ctx, devDraws, npaths, rec.pos, rec.meshes, sz.num_meshes, nullptr));
	float* meshBounds = nullptr;
	(void)hipMalloc(&meshBounds, sz.num_meshes * 4 * sizeof(float));
	CHECK(vgx_mesh_bounds(ctx, rec.pos, rec.meshes, sz.num_meshes, meshBounds, nullptr));
	const vgx_cache_desc cache = { rec.pos, rec.color, rec.idx, rec.meshes, sz.num_meshes, sz.num_vertices, sz.num_indices };

	// the scene: the drawing on a grid, one instance per drawing; room for the frame that shows all of it
	const uint32_t grid = 24, ninst = grid * grid;
	const float pitch = 1.25f * drawingSize, canvasW = 1920.0f, canvasH = 1080.0f;
	std::vector<vgx_cache_instance> inst(ninst);
	vgx_cache_instance* devInst = nullptr;
	(void)hipMalloc(&devInst, ninst * sizeof(vgx_cache_instance));
	vgx_mesh_out out;
	memset(&out, 0, sizeof(out));
	out.cap_vertices = sz.num_vertices * ninst; out.cap_indices = sz.num_indices * ninst; out.cap_meshes = sz.num_meshes * ninst;
	(void)hipMalloc(&out.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out.color, out.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, out.cap_indices * sizeof(uint16_t));
	(void)hipMalloc(&out.meshes, out.cap_meshes * sizeof(vgx_mesh));
	const float view[4] = { 0.0f, 0.0f, canvasW, canvasH }; // the canvas (a caller with a scissor puts the scissor rectangle here)
	float* devView = nullptr; uint64_t* devKept = nullptr; vgx_sizes* devSizes = nullptr; uint32_t* devStatus = nullptr;
	(void)hipMalloc(&devView, sizeof(view)); (void)hipMalloc(&devKept, sizeof(uint64_t)); (void)hipMalloc(&devSizes, sizeof(vgx_sizes));
	if (hipMalloc(&devStatus, 2 * sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devView, view, sizeof(view), hipMemcpyHostToDevice);
	printf("drawing: %u paths -> %llu meshes, %llu vertices; scene: %u instances, %llu vertices when all of it is submitted\n", npaths,
		(unsigned long long)sz.num_meshes, (unsigned long long)sz.num_vertices, ninst, (unsigned long long)(sz.num_vertices * ninst));

	vgx_cull_out cull;
	memset(&cull, 0, sizeof(cull));
	cull.inst = devInst; // in place
	cull.num_kept = devKept;
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	unsigned long long keptMin = ~0ull, keptMax = 0;
	float usTotal = 0.0f;
	for (int f = 0; f < frames; ++f) {
		// the camera pans over the scene, turns slowly and zooms in and out
		const float a = 0.01f * (float)f, z = 0.6f + 0.4f * sinf(0.25f * (float)f), c = z * cosf(a), s = z * sinf(a);
		const float px = 0.5f * pitch * (float)grid * (1.0f + 0.8f * cosf(0.13f * (float)f)), py = 0.5f * pitch * (float)grid * (1.0f + 0.8f * sinf(0.17f * (float)f));
		for (uint32_t i = 0; i < ninst; ++i) {
			const float ox = pitch * (float)(i % grid) - px, oy = pitch * (float)(i / grid) - py; // the drawing's origin seen from the camera
			vgx_cache_instance& in = inst[i];
			in.first_mesh = 0; in.num_meshes = (uint32_t)sz.num_meshes; in.color = 0xFFFFFFFFu;
			in.mtx[0] = c; in.mtx[1] = s; in.mtx[2] = -s; in.mtx[3] = c;
			in.mtx[4] = 0.5f * canvasW + (c * ox - s * oy); in.mtx[5] = 0.5f * canvasH + (s * ox + c * oy);
		}
		(void)hipMemcpyAsync(devInst, inst.data(), ninst * sizeof(vgx_cache_instance), hipMemcpyHostToDevice, nullptr);
		(void)hipEventRecord(e0, nullptr);
		CHECK(vgx_cache_cull(ctx, &cache, meshBounds, devInst, ninst, devView, 1, nullptr, &cull, devStatus + 1, nullptr));
		CHECK(vgx_cache_submit(ctx, &cache, devInst, ninst, &out, devSizes, devStatus, nullptr));
		(void)hipEventRecord(e1, nullptr);
		uint32_t status[2] = { 0, 0 }; uint64_t kept = 0; vgx_sizes got;
		(void)hipMemcpy(status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
		(void)hipMemcpy(&kept, devKept, sizeof(kept), hipMemcpyDeviceToHost);
		(void)hipMemcpy(&got, devSizes, sizeof(got), hipMemcpyDeviceToHost);
		if (status[0] != VGX_OK || status[1] != VGX_OK) { fprintf(stderr, "frame %d: submit %s, cull %s\n", f, vgx_status_string((int)status[0]), vgx_status_string((int)status[1])); return 1; }
		if (got.num_vertices != kept * sz.num_vertices) { fprintf(stderr, "frame %d: %llu vertices for %llu kept instances\n", f, (unsigned long long)got.num_vertices, (unsigned long long)kept); return 1; }
		float ms = 0.0f;
		(void)hipEventElapsedTime(&ms, e0, e1);
		if (f >= 3) { usTotal += ms * 1000.0f; }
		keptMin = kept < keptMin ? kept : keptMin; keptMax = kept > keptMax ? kept : keptMax;
		if (f < 3 || f == frames - 1) { printf("frame %d: zoom %.2f, %llu of %u instances kept, %llu vertices submitted\n", f, z, (unsigned long long)kept, ninst, (unsigned long long)got.num_vertices); }
	}
	printf("%d frames culled and submitted: %.1f us per frame on the device; instances kept per frame %llu .. %llu of %u\n",
		frames, frames > 3 ? usTotal / (float)(frames - 3) : 0.0f, keptMin, keptMax, ninst);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return keptMax < ninst && keptMax > 0 ? 0 : 1;
}
