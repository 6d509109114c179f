// vgx_raster_example.cpp -- what does the frame look like? through the C-ABI (no Python, no torch, no display GPU). One tiger-like
// drawing (60 rings, filled with translucent colours, every third one stroked) is tessellated into device memory, then
//   vgx_raster   draws the frame's mesh streams into a 256 x 256 RGBA8 image in device memory, over a white clear. A fresh context
//                guesses its bin scratch: the first call may end with VGX_E_GROWN in dev_status, having written nothing; the same
//                call again succeeds (vgx_raster_reserve ahead of the first call would avoid the round trip)
// The image comes back once, is written as a binary PPM and summed into a digest (FNV-1a over the pixel words) that the test suite
// compares with the numpy model of the specification in include/vgx.h for the same frame.
//   hipcc -O2 -I include examples/vgx_raster_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_raster_example
//   ./vgx_raster_example [out.ppm [frame.bin]]     frame.bin: the mesh streams as raw arrays, for whoever wants to check the picture
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
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_raster_example.ppm";
	const char* framePath = argc > 2 ? argv[2] : nullptr;
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));

	// the drawing: 60 closed rings of 8-40 points inside a 256 x 256 box
	const uint32_t npaths = 60, width = 256, height = 256;
	std::vector<uint8_t> cmdType;
	std::vector<uint32_t> cmdArgOff(1, 0u), pathCmdBegin(1, 0u);
	std::vector<float> args;
	uint32_t seed = 2025u;
	for (uint32_t p = 0; p < npaths; ++p) {
		const uint32_t n = 8 + rnd(seed) % 33;
		const float r = 8.0f + (float)(rnd(seed) % 40);
		const float cx = r + (float)(rnd(seed) % (uint32_t)((float)width - 2.0f * r)), cy = r + (float)(rnd(seed) % (uint32_t)((float)height - 2.0f * r));
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
		d.fill_flags = VGX_FILL_ENABLE | VGX_FILL_AA; d.fill_color = (0x60000000u + ((rnd(seed) & 0x7Fu) << 24)) | (rnd(seed) & 0xFFFFFFu);
		if (p % 3 == 0) { d.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0); d.stroke_color = 0xFF000000u | (rnd(seed) & 0x7F7F7Fu); d.stroke_width = 2.0f; }
		d.scale = 1.0f; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = 1.0f; d.mtx[3] = 1.0f;
		draws[p] = d;
	}
	vgx_draw* devDraws = nullptr;
	if (hipMalloc(&devDraws, npaths * sizeof(vgx_draw)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), npaths * sizeof(vgx_draw), hipMemcpyHostToDevice);

	// tessellate: the frame lives in device memory
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, npaths, &sz, nullptr));
	vgx_mesh_out out;
	memset(&out, 0, sizeof(out));
	out.cap_vertices = sz.num_vertices; out.cap_indices = sz.num_indices; out.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&out.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out.color, out.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, out.cap_indices * sizeof(uint16_t));
	if (hipMalloc(&out.meshes, out.cap_meshes * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, npaths, &out, nullptr));
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, sz.num_meshes, sz.num_vertices, sz.num_indices };
	printf("frame: %llu meshes, %llu vertices, %llu indices in device memory\n", (unsigned long long)sz.num_meshes,
		(unsigned long long)sz.num_vertices, (unsigned long long)sz.num_indices);

	// render
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFFFFFFFu;
	uint32_t* devStatus = nullptr;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess || hipMalloc(&devStatus, sizeof(uint32_t)) != hipSuccess) { return 1; }
	uint32_t status = VGX_E_GROWN, calls = 0;
	while (status == VGX_E_GROWN && calls < 3) {
		CHECK(vgx_raster(ctx, &frame, nullptr, 0, sz.num_meshes, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		++calls;
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster: %s\n", vgx_status_string((int)status)); return 1; }
	std::vector<uint32_t> pixels((size_t)width * height);
	if (hipMemcpy(pixels.data(), tgt.pixels, pixels.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }

	// the picture and its digest
	uint64_t digest = 1469598103934665603ull;
	uint32_t painted = 0;
	std::vector<uint8_t> rgb(pixels.size() * 3);
	for (size_t k = 0; k < pixels.size(); ++k) {
		const uint32_t c = pixels[k];
		for (int b = 0; b < 4; ++b) { digest = (digest ^ ((c >> (8 * b)) & 255u)) * 1099511628211ull; }
		rgb[3 * k] = (uint8_t)c; rgb[3 * k + 1] = (uint8_t)(c >> 8); rgb[3 * k + 2] = (uint8_t)(c >> 16);
		painted += c != 0xFFFFFFFFu;
	}
	FILE* f = fopen(ppmPath, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppmPath); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	fwrite(rgb.data(), 1, rgb.size(), f);
	fclose(f);
	if (framePath) { // header of six uint64 (meshes, vertices, indices, width, height, 0), then pos, color, idx, meshes
		std::vector<float> hpos(2 * sz.num_vertices); std::vector<uint32_t> hcol(sz.num_vertices); std::vector<uint16_t> hidx(sz.num_indices); std::vector<vgx_mesh> hm(sz.num_meshes);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hm.data(), out.meshes, hm.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[6] = { sz.num_meshes, sz.num_vertices, sz.num_indices, width, height, 0 };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(hm.data(), sizeof(vgx_mesh), hm.size(), g);
		fclose(g);
	}
	printf("rendered %u x %u in %u call%s: %u pixels painted, written to %s\n", width, height, calls, calls == 1 ? "" : "s", painted, ppmPath);
	printf("digest %016llx\n", (unsigned long long)digest);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return painted > 1000 ? 0 : 1;
}
