// vgx_text_raster_example.cpp -- a command list with a label and a user mesh, from its bytes to pixels, through the C-ABI (no Python, no
// torch, no display GPU, no font file):
//   bytes of a command list (written here by hand in the reference's wire format): a filled rectangle, a Text command, an
//   IndexedTriList on image 1
//   -> vgx_cmdlist_decode_text (host): paths + draws + per-draw state, the Text command as a vgx_text_cmd, the user mesh in tri_*
//   -> vgx_tessellate_count / _emit (device): the meshes of the path draws = sequence A
//   -> the caller's shaper, played by a fixed-advance stand-in: one glyph quad per character, its UVs the character's 8 x 8 cell of a
//      128 x 128 atlas made up here (every cell a pattern of its own: a glyph is recognisable, a font it is not)
//   -> vgx_text_quads (device): the run's mesh at its place in sequence B, in front of the user mesh the decoder handed over
//   -> vgx_merge_uv_stream (device): A and B interleaved by draw, B's UVs in a UV stream beside pos / color
//   -> vgx_raster_textured (device): the frame in a 256 x 128 RGBA8 image; text and user mesh sampled from their images
// The image comes back once, is written as a binary PPM and summed into a digest (FNV-1a over the pixel words) that the test suite
// compares with the numpy model of the specification in include/vgx.h for the same frame.
//   hipcc -O2 -I include examples/vgx_text_raster_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_text_raster_example
//   ./vgx_text_raster_example [out.ppm [frame.bin]]     frame.bin: streams, draws and images as raw arrays, for whoever wants to check
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
enum { CT_BeginPath = 0, CT_Rect = 7, CT_FillPathColor = 14, CT_IndexedTriList = 20, CT_Text = 40 };
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
	void rect(float x, float y, float w, float h) { const float a[4] = { x, y, w, h }; cmd(CT_BeginPath, nullptr, 0); cmd(CT_Rect, a, 16); }
	void fill(uint32_t color) { const uint32_t p[2] = { 4u /* AA */, color }; cmd(CT_FillPathColor, p, 8); }
	// clText: TextConfig{uint16 font, float size, uint32 alignment, Color}, float x, y, uint32 string offset, length
	void text(float size, uint32_t color, float x, float y, uint32_t offset, uint32_t len)
	{
		uint8_t p[32] = { 0 };
		const uint32_t align = 1u | 64u; // left, baseline
		memcpy(p + 4, &size, 4); memcpy(p + 8, &align, 4); memcpy(p + 12, &color, 4); memcpy(p + 16, &x, 4); memcpy(p + 20, &y, 4);
		memcpy(p + 24, &offset, 4); memcpy(p + 28, &len, 4);
		cmd(CT_Text, p, 32);
	}
	// clIndexedTriList: uint32 nv, float2 pos[nv], uint32 nuv, int16x2 uv[nuv], uint32 nc, Color col[nc], uint32 ni, uint16 idx[ni], uint16 image
	void triList(const float* pos, const int16_t* uv, uint32_t nv, const uint32_t* col, uint32_t nc, const uint16_t* idx, uint32_t ni, uint16_t image)
	{
		std::vector<uint8_t> p;
		auto put = [&](const void* src, size_t n) { p.insert(p.end(), (const uint8_t*)src, (const uint8_t*)src + n); };
		put(&nv, 4); put(pos, (size_t)nv * 8); put(&nv, 4); put(uv, (size_t)nv * 4);
		put(&nc, 4); put(col, (size_t)nc * 4); put(&ni, 4); put(idx, (size_t)ni * 2); put(&image, 2);
		cmd(CT_IndexedTriList, p.data(), (uint32_t)p.size());
	}
};

template <class T>
static T* upload(const std::vector<T>& v, size_t extra = 0)
{
	T* d = nullptr;
	if (hipMalloc(&d, (v.size() + extra + 1) * sizeof(T)) != hipSuccess) { return nullptr; }
	if (!v.empty()) { (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); }
	return d;
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_text_raster_example.ppm";
	const char* framePath = argc > 2 ? argv[2] : nullptr;
	const uint32_t width = 256, height = 128;

	// ---- the list: a shape, a label on it, a user mesh beside it ----
	const char label[] = "VGX draws TEXT 0123";
	const uint32_t labelLen = (uint32_t)strlen(label);
	ListWriter L;
	L.rect(12.0f, 20.0f, 232.0f, 56.0f); L.fill(0xFF804020u);
	L.text(16.0f, 0xFFFFFFFFu, 20.0f, 56.0f, 0, labelLen);
	const float q[8] = { 150.0f, 70.0f, 240.0f, 64.0f, 246.0f, 120.0f, 144.0f, 114.0f };
	const int16_t quv[8] = { 0, 0, 32767, 0, 32767, 32767, 0, 32767 };
	const uint32_t qcol[4] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xC080FFFFu, 0x80FFFFFFu };
	const uint16_t qidx[6] = { 0, 1, 2, 0, 2, 3 };
	L.triList(q, quv, 4, qcol, 4, qidx, 6, 1);

	// ---- host: decode (count pass, then store pass) ----
	vgx_cmdlist_state st = {};
	st.mtx[0] = 1.0f; st.mtx[3] = 1.0f; st.global_alpha = 1.0f; st.tess_tol = 0.25f; st.fringe = 1.0f;
	st.canvas_width = (float)width; st.canvas_height = (float)height;
	st.font_image = 0; // the atlas is image 0 of the table below
	vgx_cmdlist_out o = {};
	vgx_cmdlist_text tx = {};
	tx.strings = label; tx.strings_size = labelLen; tx.device_pixel_ratio = 1.0f;
	CHECK(vgx_cmdlist_decode_text(L.b.data(), (uint32_t)L.b.size(), &st, &o, &tx));
	std::vector<uint8_t> cmdType(o.num_cmds + 1);
	std::vector<uint32_t> argOff(o.num_cmds + 1), pathBegin(o.num_paths + 1);
	std::vector<float> args(o.num_args + 1);
	std::vector<vgx_draw> draws(o.num_draws);
	std::vector<vgx_draw_state> dstate(o.num_draws);
	std::vector<vgx_text_cmd> texts(tx.num_texts);
	std::vector<float> triPos(o.num_tri_vertices * 2);
	std::vector<uint32_t> triCol(o.num_tri_vertices), triUV(o.num_tri_vertices);
	std::vector<uint16_t> triIdx(o.num_tri_indices);
	std::vector<vgx_mesh> triMesh(o.num_tri_meshes);
	o.cmd_type = cmdType.data(); o.cmd_arg_off = argOff.data(); o.args = args.data(); o.path_cmd_begin = pathBegin.data();
	o.draws = draws.data(); o.draw_state = dstate.data();
	o.cap_cmds = o.num_cmds; o.cap_args = o.num_args; o.cap_paths = o.num_paths; o.cap_draws = o.num_draws;
	o.tri_pos = triPos.data(); o.tri_color = triCol.data(); o.tri_uv = triUV.data(); o.tri_idx = triIdx.data(); o.tri_meshes = triMesh.data();
	o.cap_tri_vertices = o.num_tri_vertices; o.cap_tri_indices = o.num_tri_indices; o.cap_tri_meshes = o.num_tri_meshes;
	tx.texts = texts.data(); tx.cap_texts = tx.num_texts;
	CHECK(vgx_cmdlist_decode_text(L.b.data(), (uint32_t)L.b.size(), &st, &o, &tx));
	printf("list: %zu bytes -> %u draws: %u text command(s), %u user mesh(es), %u skipped\n", L.b.size(), o.num_draws, tx.num_texts, o.num_tri_meshes, o.num_skipped);
	if (tx.num_texts != 1 || o.num_tri_meshes != 1 || texts[0].draw >= triMesh[0].draw) { fprintf(stderr, "unexpected decode\n"); return 1; }

	// ---- the atlas: 16 x 16 cells of 8 x 8 texels, white, the pattern in the alpha channel; and a checker for the user mesh ----
	const uint32_t aw = 128, cw = 8;
	std::vector<uint32_t> atlas(aw * aw), checker(8 * 8);
	for (uint32_t y = 0; y < aw; ++y) {
		for (uint32_t x = 0; x < aw; ++x) {
			const uint32_t cell = (y / cw) * 16 + x / cw, lx = x % cw, ly = y % cw;
			uint64_t h = (cell + 1) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
			const bool frame = lx == 0 || ly == 0 || lx == cw - 1 || ly == cw - 1;                // an empty border: neighbours do not bleed in
			const bool on = !frame && ((h >> ((ly - 1) * 6 + (lx - 1))) & 1u) != 0;
			atlas[y * aw + x] = on ? 0xFFFFFFFFu : 0x00FFFFFFu;
		}
	}
	for (uint32_t k = 0; k < 64; ++k) { checker[k] = ((k % 8 + k / 8) % 2) ? 0xFF30C0FFu : 0xFF2020A0u; }

	// ---- the shaper's part: fixed advance, one quad per character that is not a blank (FONSquad: x0 y0 x1 y1 s0 t0 s1 t1) ----
	const vgx_text_cmd& tc = texts[0];
	const float size = tc.font_size * tc.scale, adv = size * 0.7f;
	std::vector<float> quads;
	for (uint32_t k = 0; k < tc.string_len; ++k) {
		const uint8_t c = (uint8_t)label[tc.string_offset + k];
		if (c == ' ') { continue; }
		const float x0 = adv * (float)k, s0 = (float)(c % 16) / 16.0f, t0 = (float)(c / 16) / 16.0f;
		const float rec[8] = { x0, -0.8f * size, x0 + 0.9f * adv, 0.2f * size, s0, t0, s0 + 1.0f / 16.0f, t0 + 1.0f / 16.0f };
		quads.insert(quads.end(), rec, rec + 8);
	}
	const uint32_t nquads = (uint32_t)(quads.size() / 8);
	vgx_text_run run = {};
	run.first_quad = 0; run.num_quads = nquads; run.color = tc.color; memcpy(run.mtx, tc.mtx, sizeof(run.mtx));
	run.x = tc.x; run.y = tc.y; run.dx = 0.0f; run.dy = 0.0f; run.scale = tc.scale; run.draw = tc.draw;
	run.first_vertex = 0; run.first_index = 0; // sequence B: the run first (its draw comes first), the user mesh behind it

	// ---- device ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = upload(draws);
	vgx_draw_state* devState = upload(dstate);
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, o.num_draws, &sz, nullptr));
	vgx_mesh_out seqA = {};
	seqA.cap_vertices = sz.num_vertices; seqA.cap_indices = sz.num_indices; seqA.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&seqA.pos, (sz.num_vertices + 1) * 2 * sizeof(float));
	(void)hipMalloc(&seqA.color, (sz.num_vertices + 1) * sizeof(uint32_t));
	(void)hipMalloc(&seqA.idx, (sz.num_indices + 1) * sizeof(uint16_t));
	if (hipMalloc(&seqA.meshes, (sz.num_meshes + 1) * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, o.num_draws, &seqA, nullptr));
	const vgx_cache_desc a = { seqA.pos, seqA.color, seqA.idx, seqA.meshes, sz.num_meshes, sz.num_vertices, sz.num_indices };

	// sequence B: [the run: 4 n vertices, 6 n indices][the user mesh as the decoder handed it over]
	const uint64_t bv = 4ull * nquads + o.num_tri_vertices, bi = 6ull * nquads + o.num_tri_indices;
	vgx_mesh_out seqB = {};
	seqB.cap_vertices = bv; seqB.cap_indices = bi; seqB.cap_meshes = 2;
	uint32_t* bUV = nullptr;
	(void)hipMalloc(&seqB.pos, bv * 2 * sizeof(float)); (void)hipMalloc(&seqB.color, bv * sizeof(uint32_t)); (void)hipMalloc(&bUV, bv * sizeof(uint32_t));
	(void)hipMalloc(&seqB.idx, (bi + 1) * sizeof(uint16_t));
	if (hipMalloc(&seqB.meshes, 2 * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	vgx_mesh um = triMesh[0];
	um.first_vertex += 4ull * nquads; um.first_index += 6ull * nquads;
	(void)hipMemcpy(seqB.pos + 8ull * nquads, triPos.data(), triPos.size() * sizeof(float), hipMemcpyHostToDevice);
	(void)hipMemcpy(seqB.color + 4ull * nquads, triCol.data(), triCol.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
	(void)hipMemcpy(bUV + 4ull * nquads, triUV.data(), triUV.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
	(void)hipMemcpy(seqB.idx + 6ull * nquads, triIdx.data(), triIdx.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
	(void)hipMemcpy(seqB.meshes + 1, &um, sizeof(um), hipMemcpyHostToDevice);
	float* devQuads = nullptr; vgx_text_run* devRun = nullptr;
	vgx_sizes* devSizes = nullptr; uint32_t* devStatus = nullptr;
	(void)hipMalloc(&devQuads, quads.size() * sizeof(float) + 16); (void)hipMalloc(&devRun, sizeof(run));
	(void)hipMalloc(&devSizes, sizeof(vgx_sizes));
	if (hipMalloc(&devStatus, sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devQuads, quads.data(), quads.size() * sizeof(float), hipMemcpyHostToDevice);
	(void)hipMemcpy(devRun, &run, sizeof(run), hipMemcpyHostToDevice);
	uint32_t status = 1;
	CHECK(vgx_text_quads(ctx, devQuads, nquads, devRun, 1, 0, &seqB, bUV, 4, devSizes, devStatus, nullptr));
	if (hipMemcpy(&status, devStatus, 4, hipMemcpyDeviceToHost) != hipSuccess || status != VGX_OK) { fprintf(stderr, "vgx_text_quads: device status %u\n", status); return 1; }
	const vgx_cache_desc b = { seqB.pos, seqB.color, seqB.idx, seqB.meshes, 2, bv, bi };

	// the frame: both sequences interleaved by draw, B's UVs beside them
	const uint64_t nv = sz.num_vertices + bv, ni = sz.num_indices + bi, nm = sz.num_meshes + 2;
	vgx_mesh_out out = {};
	out.cap_vertices = nv; out.cap_indices = ni; out.cap_meshes = nm;
	uint32_t* outUV = nullptr;
	(void)hipMalloc(&out.pos, nv * 2 * sizeof(float)); (void)hipMalloc(&out.color, nv * sizeof(uint32_t)); (void)hipMalloc(&outUV, nv * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, (ni + 1) * sizeof(uint16_t));
	if (hipMalloc(&out.meshes, nm * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	(void)hipMemset(outUV, 0, nv * sizeof(uint32_t)); // only the vertices of B's meshes are written; the others are never read
	CHECK(vgx_merge_uv_stream(ctx, &a, &b, nullptr, bUV, 4, devDraws, o.num_draws, &out, outUV, devSizes, devStatus, nullptr));
	if (hipMemcpy(&status, devStatus, 4, hipMemcpyDeviceToHost) != hipSuccess || status != VGX_OK) { fprintf(stderr, "vgx_merge_uv_stream: device status %u\n", status); return 1; }
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, nm, nv, ni };
	printf("frame: %llu meshes (%llu from paths, a run of %u glyphs, a user mesh), %llu vertices, %llu indices in device memory\n", (unsigned long long)nm,
		(unsigned long long)sz.num_meshes, nquads, (unsigned long long)nv, (unsigned long long)ni);

	// ---- render ----
	vgx_raster_image images[2] = { { upload(atlas), aw, aw, aw, 0u /* linear, repeat */ }, { upload(checker), 8, 8, 8, VGX_IMAGE_NEAREST } };
	vgx_raster_image* devImages = nullptr;
	if (!images[0].pixels || !images[1].pixels || hipMalloc(&devImages, sizeof(images)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devImages, images, sizeof(images), hipMemcpyHostToDevice);
	const vgx_raster_draws rdraws = { devDraws, devState, o.num_draws, 0 };
	const vgx_raster_textures rtex = { outUV, devImages, 4, 2 };
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFFFFFFFu;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	uint32_t calls = 0;
	status = VGX_E_GROWN;
	while (status == VGX_E_GROWN && calls < 3) {
		CHECK(vgx_raster_textured(ctx, &frame, nullptr, 0, nm, &rdraws, &rtex, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		++calls;
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_textured: %s\n", vgx_status_string((int)status)); return 1; }
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
		painted += c != 0xFFFFFFFFu;
	}
	FILE* f = fopen(ppmPath, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppmPath); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	fwrite(rgb.data(), 1, rgb.size(), f);
	fclose(f);
	if (framePath) { // eight uint64 (meshes, vertices, indices, width, height, draws, atlas side, 0), then pos, color, uv, idx, meshes, draws, draw states, atlas, checker
		std::vector<float> hpos(2 * nv); std::vector<uint32_t> hcol(nv), huv(nv); std::vector<uint16_t> hidx(ni); std::vector<vgx_mesh> hm(nm);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(huv.data(), outUV, huv.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hm.data(), out.meshes, hm.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[8] = { nm, nv, ni, width, height, o.num_draws, aw, 0 };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g); fwrite(huv.data(), sizeof(uint32_t), huv.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(hm.data(), sizeof(vgx_mesh), hm.size(), g);
		fwrite(draws.data(), sizeof(vgx_draw), draws.size(), g); fwrite(dstate.data(), sizeof(vgx_draw_state), dstate.size(), g);
		fwrite(atlas.data(), sizeof(uint32_t), atlas.size(), g); fwrite(checker.data(), sizeof(uint32_t), checker.size(), g);
		fclose(g);
	}
	printf("rendered %u x %u in %u call%s: %u pixels painted, written to %s\n", width, height, calls, calls == 1 ? "" : "s", painted, ppmPath);
	printf("digest %016llx\n", (unsigned long long)digest);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return painted > 1000 ? 0 : 1;
}
