// vgx_gradient_example.cpp -- a command list with gradient and image-pattern paints, from its bytes to pixels, through the C-ABI (no
// Python, no torch, no display GPU):
//   bytes of a command list (written here by hand in the reference's wire format): a button with a linear gradient over the drop shadow
//   a box gradient makes, a radial glow, and a badge filled with an image pattern
//   -> vgx_cmdlist_decode (host): paths + draws + per-draw state + one vgx_paint per Create* command
//   -> vgx_paint_tables (host): the paints scattered into the gradient table and the pattern table, indexed by handle
//   -> vgx_tessellate_count / _emit (device): the meshes of the frame
//   -> vgx_raster_painted (device): the frame in a 256 x 128 RGBA8 image; every painted mesh takes its colour from its draw's paint
// The image comes back once, is written as a binary PPM and summed into a digest (FNV-1a over the pixel words) that the test suite
// compares with the numpy model of the specification in include/vgx.h for the same frame.
//   hipcc -O2 -I include examples/vgx_gradient_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_gradient_example
//   ./vgx_gradient_example [out.ppm [frame.bin]]     frame.bin: streams, draws, paints and the image as raw arrays, for whoever wants to check
#include <hip/hip_runtime.h>
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

// vg::CommandType values used here and the record layout: CommandHeader{uint32 type, uint32 size} padded to 16 bytes, then the payload
// padded to 16 bytes
enum { CT_BeginPath = 0, CT_RoundedRect = 8, CT_Circle = 10, CT_FillPathGradient = 15, CT_FillPathImagePattern = 16, CT_CreateLinearGradient = 24,
       CT_CreateBoxGradient = 25, CT_CreateRadialGradient = 26, CT_CreateImagePattern = 27 };
struct ListWriter
{
	std::vector<uint8_t> b;
	void cmd(uint32_t type, const void* payload, uint32_t n)
	{
		const uint32_t padded = (n + 15u) & ~15u;
		const uint32_t hdr[4] = { type, padded, 0, 0 };
		b.insert(b.end(), (const uint8_t*)hdr, (const uint8_t*)hdr + 16);
		b.insert(b.end(), (const uint8_t*)payload, (const uint8_t*)payload + n);
		b.insert(b.end(), padded - n, 0);
	}
	void roundedRect(float x, float y, float w, float h, float r) { const float a[5] = { x, y, w, h, r }; cmd(CT_BeginPath, nullptr, 0); cmd(CT_RoundedRect, a, 20); }
	void circle(float x, float y, float r) { const float a[3] = { x, y, r }; cmd(CT_BeginPath, nullptr, 0); cmd(CT_Circle, a, 12); }
	// clCreateLinearGradient / RadialGradient: four floats, two colours; BoxGradient: six floats, two colours
	void gradient(uint32_t type, const float* f, uint32_t nf, uint32_t inner, uint32_t outer)
	{
		uint8_t p[32];
		memcpy(p, f, nf * 4); memcpy(p + nf * 4, &inner, 4); memcpy(p + nf * 4 + 4, &outer, 4);
		cmd(type, p, nf * 4 + 8);
	}
	// clCreateImagePattern: cx, cy, w, h, angle, uint16 image
	void imagePattern(float cx, float cy, float w, float h, float angle, uint16_t image)
	{
		uint8_t p[22];
		const float f[5] = { cx, cy, w, h, angle };
		memcpy(p, f, 20); memcpy(p + 20, &image, 2);
		cmd(CT_CreateImagePattern, p, 22);
	}
	// clFillPathGradient: uint32 flags, uint16 handle, uint16 handle flags; the handles of this list count from 0
	void fillGradient(uint16_t handle) { uint8_t p[8]; const uint32_t aa = 4u; const uint16_t hf = 0; memcpy(p, &aa, 4); memcpy(p + 4, &handle, 2); memcpy(p + 6, &hf, 2); cmd(CT_FillPathGradient, p, 8); }
	// clFillPathImagePattern: uint32 flags, Color (the tint), uint16 handle, uint16 handle flags
	void fillPattern(uint32_t tint, uint16_t handle)
	{
		uint8_t p[12];
		const uint32_t aa = 4u; const uint16_t hf = 0;
		memcpy(p, &aa, 4); memcpy(p + 4, &tint, 4); memcpy(p + 8, &handle, 2); memcpy(p + 10, &hf, 2);
		cmd(CT_FillPathImagePattern, p, 12);
	}
};

template <class T>
static T* upload(const std::vector<T>& v)
{
	T* d = nullptr;
	if (hipMalloc(&d, (v.size() + 1) * sizeof(T)) != hipSuccess) { return nullptr; }
	if (!v.empty()) { (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); }
	return d;
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_gradient_example.ppm";
	const char* framePath = argc > 2 ? argv[2] : nullptr;
	const uint32_t width = 256, height = 128, side = 8;

	// ---- the list ----
	ListWriter L;
	const float shadow[6] = { 20.0f, 26.0f, 130.0f, 60.0f, 12.0f, 16.0f };       // x, y, w, h, corner radius, feather
	L.gradient(CT_CreateBoxGradient, shadow, 6, 0xC0000000u, 0x00000000u);        // gradient 0: the drop shadow
	L.roundedRect(8.0f, 14.0f, 154.0f, 84.0f, 4.0f); L.fillGradient(0);
	const float lin[4] = { 0.0f, 20.0f, 0.0f, 80.0f };                            // from (sx, sy) to (ex, ey)
	L.gradient(CT_CreateLinearGradient, lin, 4, 0xFFFFB060u, 0xFFC03010u);        // gradient 1: the button's face
	L.roundedRect(16.0f, 20.0f, 130.0f, 60.0f, 10.0f); L.fillGradient(1);
	const float glow[4] = { 200.0f, 44.0f, 6.0f, 38.0f };                         // centre, inner and outer radius
	L.gradient(CT_CreateRadialGradient, glow, 4, 0xFFFFFFFFu, 0x0040C0FFu);       // gradient 2: a glow
	L.circle(200.0f, 44.0f, 40.0f); L.fillGradient(2);
	L.imagePattern(170.0f, 84.0f, 24.0f, 24.0f, 0.35f, 0);                        // pattern 0: image 0, one repeat per 24 units, turned
	L.roundedRect(168.0f, 82.0f, 76.0f, 38.0f, 8.0f); L.fillPattern(0xFFFFFFFFu, 0);

	// ---- host: decode (count pass, then store pass), then the paint tables ----
	vgx_cmdlist_state st = {};
	st.mtx[0] = 1.0f; st.mtx[3] = 1.0f; st.global_alpha = 1.0f; st.tess_tol = 0.25f; st.fringe = 1.0f;
	st.canvas_width = (float)width; st.canvas_height = (float)height;
	vgx_cmdlist_out o = {};
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));
	std::vector<uint8_t> cmdType(o.num_cmds + 1);
	std::vector<uint32_t> argOff(o.num_cmds + 1), pathBegin(o.num_paths + 1);
	std::vector<float> args(o.num_args + 1);
	std::vector<vgx_draw> draws(o.num_draws);
	std::vector<vgx_draw_state> dstate(o.num_draws);
	std::vector<vgx_paint> paints(o.num_paints);
	o.cmd_type = cmdType.data(); o.cmd_arg_off = argOff.data(); o.args = args.data(); o.path_cmd_begin = pathBegin.data();
	o.draws = draws.data(); o.draw_state = dstate.data(); o.paints = paints.data();
	o.cap_cmds = o.num_cmds; o.cap_args = o.num_args; o.cap_paths = o.num_paths; o.cap_draws = o.num_draws; o.cap_paints = o.num_paints;
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));
	printf("list: %zu bytes -> %u draws, %u paints, %u skipped\n", L.b.size(), o.num_draws, o.num_paints, o.num_skipped);
	if (o.num_draws != 4 || o.num_paints != 4 || o.next_gradient != 3 || o.next_image_pattern != 1) { fprintf(stderr, "unexpected decode\n"); return 1; }
	std::vector<vgx_paint> gradients(o.next_gradient), patterns(o.next_image_pattern);
	CHECK(vgx_paint_tables(paints.data(), o.num_paints, gradients.data(), (uint32_t)gradients.size(), patterns.data(), (uint32_t)patterns.size()));

	// ---- the pattern's image: an 8 x 8 tile of two colours with a diagonal ----
	std::vector<uint32_t> tile(side * side);
	for (uint32_t k = 0; k < side * side; ++k) {
		const uint32_t x = k % side, y = k / side;
		tile[k] = x == y ? 0xFFFFFFFFu : (((x / 4 + y / 4) % 2) ? 0xFF30C0FFu : 0xFF2020A0u);
	}

	// ---- device ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = upload(draws);
	vgx_draw_state* devState = upload(dstate);
	vgx_paint* devGradients = upload(gradients);
	vgx_paint* devPatterns = upload(patterns);
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, o.num_draws, &sz, nullptr));
	const uint64_t nv = sz.num_vertices, ni = sz.num_indices, nm = sz.num_meshes;
	vgx_mesh_out out = {};
	out.cap_vertices = nv; out.cap_indices = ni; out.cap_meshes = nm;
	(void)hipMalloc(&out.pos, (nv + 1) * 2 * sizeof(float));
	(void)hipMalloc(&out.color, (nv + 1) * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, (ni + 1) * sizeof(uint16_t));
	if (hipMalloc(&out.meshes, (nm + 1) * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, o.num_draws, &out, nullptr));
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, nm, nv, ni };
	printf("frame: %llu meshes, %llu vertices, %llu indices in device memory\n", (unsigned long long)nm, (unsigned long long)nv, (unsigned long long)ni);

	// ---- render ----
	vgx_raster_image image = { upload(tile), side, side, side, 0u /* linear, repeat */ };
	vgx_raster_image* devImages = nullptr;
	uint32_t* devUV = nullptr; // no mesh of this frame is sampled: the stream is never read, but a range that is not empty needs one
	uint32_t* devStatus = nullptr;
	if (!image.pixels || hipMalloc(&devImages, sizeof(image)) != hipSuccess || hipMalloc(&devUV, (nv + 1) * sizeof(uint32_t)) != hipSuccess
	    || hipMalloc(&devStatus, sizeof(uint32_t)) != hipSuccess) {
		return 1;
	}
	(void)hipMemcpy(devImages, &image, sizeof(image), hipMemcpyHostToDevice);
	const vgx_raster_draws rdraws = { devDraws, devState, o.num_draws, 0 };
	const vgx_raster_textures rtex = { devUV, devImages, 4, 1 };
	const vgx_raster_paints rpaints = { devGradients, devPatterns, (uint32_t)gradients.size(), (uint32_t)patterns.size() };
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFE8E0D8u;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	uint32_t calls = 0, status = VGX_E_GROWN;
	while (status == VGX_E_GROWN && calls < 3) {
		CHECK(vgx_raster_painted(ctx, &frame, nullptr, 0, nm, &rdraws, &rtex, &rpaints, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		++calls;
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_painted: %s\n", vgx_status_string((int)status)); return 1; }
	std::vector<uint32_t> pixels((size_t)width * height);
	if (hipMemcpy(pixels.data(), tgt.pixels, pixels.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }

	// the picture and its digest
	uint64_t digest = 1469598103934665603ull;
	uint32_t painted = 0;
	std::vector<uint8_t> rgb(pixels.size() * 3);
	for (size_t k = 0; k < pixels.size(); ++k) {
		const uint32_t c = pixels[k];
		for (int s = 0; s < 4; ++s) { digest = (digest ^ ((c >> (8 * s)) & 255u)) * 1099511628211ull; }
		rgb[3 * k] = (uint8_t)c; rgb[3 * k + 1] = (uint8_t)(c >> 8); rgb[3 * k + 2] = (uint8_t)(c >> 16);
		painted += c != tgt.clear_color;
	}
	FILE* f = fopen(ppmPath, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppmPath); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	fwrite(rgb.data(), 1, rgb.size(), f);
	fclose(f);
	if (framePath) { // eight uint64 (meshes, vertices, indices, width, height, draws, paints, image side), then pos, color, idx, meshes, draws, draw states, paints, image
		std::vector<float> hpos(2 * nv); std::vector<uint32_t> hcol(nv); std::vector<uint16_t> hidx(ni); std::vector<vgx_mesh> hm(nm);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hm.data(), out.meshes, hm.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[8] = { nm, nv, ni, width, height, o.num_draws, o.num_paints, side };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(hm.data(), sizeof(vgx_mesh), hm.size(), g);
		fwrite(draws.data(), sizeof(vgx_draw), draws.size(), g); fwrite(dstate.data(), sizeof(vgx_draw_state), dstate.size(), g);
		fwrite(paints.data(), sizeof(vgx_paint), paints.size(), g); fwrite(tile.data(), sizeof(uint32_t), tile.size(), g);
		fclose(g);
	}
	printf("rendered %u x %u in %u call%s: %u pixels painted, written to %s\n", width, height, calls, calls == 1 ? "" : "s", painted, ppmPath);
	printf("digest %016llx\n", (unsigned long long)digest);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return painted > 1000 ? 0 : 1;
}
