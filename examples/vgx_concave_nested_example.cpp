// vgx_concave_nested_example.cpp -- outlined TEXT and a target with islands as triangles without libtess2 and without leaving the
// device, through the C-ABI (no Python, no torch, no display GPU): a command list with the word "oBioBio" as ONE path of sixteen
// outlines and a target of five nested squares, from its bytes to a draw-command table, pixels and three picks.
//   bytes of a command list (written here by hand in the reference's wire format)
//   -> vgx_cmdlist_decode (host): paths + draws + per-draw state; the word and the target are draws with VGX_FILL_CONCAVE of sixteen
//      and five sub-paths
//   -> vgx_tessellate_count / _emit (device): the mesh of the convex backdrop (sequence a)
//   -> vgx_flatten_count / _emit (device): the transformed polylines and sub-paths of the frame's draws
//   -> vgx_concave_triangulate_nested (device): the word is nine groups (three "o" and two "B" with their counters, two stems and two
//      dots), the target three (an island in a hole in an island); both come out as triangles, the target behind its AA fringe.
//      vgx_concave_triangulate_rings would refuse both as VGX_TRI_REFUSED_NESTING. The routes are the only thing the host reads back.
//   -> vgx_pick on the triangles: the dot of the first "i" and the innermost square hit, the counter of the first "o" does not
//   -> vgx_merge under vgx_set_assembly (VGX_ASM_SPLIT_STATE): vertex buffers, ONE index buffer, the draw-command table
//   -> vgx_raster_cmds_from_assembly -> vgx_raster_commands: a 160 x 64 RGBA8 image, written as a binary PPM, and its digest (FNV-1a)
//   hipcc -O2 -I include examples/vgx_concave_nested_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_concave_nested_example
//   ./vgx_concave_nested_example [out.ppm]
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

// vg::CommandType values used here and the record layout: CommandHeader{uint32 type, uint32 size} padded to 16 bytes, then the payload
// padded to 16 bytes
enum { CT_BeginPath = 0, CT_MoveTo = 1, CT_LineTo = 2, CT_Rect = 7, CT_ClosePath = 13, CT_FillPathColor = 14 };
enum { FF_Concave = 1u, FF_AA = 4u }; // VG_FILL_FLAGS (include/vg/vg.h:229): PathType in bit 0, AA in bit 2
struct ListWriter
{
	std::vector<uint8_t> b;
	void cmd(uint32_t type, const void* payload, uint32_t n)
	{
		const uint32_t padded = (n + 15u) & ~15u;
		const uint32_t hdr[4] = { type, padded, 0, 0 };
		b.insert(b.end(), (const uint8_t*)hdr, (const uint8_t*)hdr + 16);
		if (n) { b.insert(b.end(), (const uint8_t*)payload, (const uint8_t*)payload + n); }
		b.insert(b.end(), padded - n, 0);
	}
	void polygon(const float* xy, int n)
	{
		cmd(CT_BeginPath, nullptr, 0);
		for (int k = 0; k < n; ++k) { cmd(k ? CT_LineTo : CT_MoveTo, xy + 2 * k, 8); }
		cmd(CT_ClosePath, nullptr, 0);
	}
	// one path of several closed sub-paths: n[k] points each, back to back in xy
	void rings(const float* xy, const int* n, int nrings)
	{
		cmd(CT_BeginPath, nullptr, 0);
		for (int r = 0; r < nrings; ++r) {
			for (int k = 0; k < n[r]; ++k) { cmd(k ? CT_LineTo : CT_MoveTo, xy + 2 * k, 8); }
			cmd(CT_ClosePath, nullptr, 0);
			xy += 2 * n[r];
		}
	}
	void rect(float x, float y, float w, float h) { const float a[4] = { x, y, w, h }; cmd(CT_BeginPath, nullptr, 0); cmd(CT_Rect, a, 16); }
	void fillColor(uint32_t flags, uint32_t color) { const uint32_t p[2] = { flags, color }; cmd(CT_FillPathColor, p, 8); }
};

template <class T>
static T* upload(const std::vector<T>& v)
{
	T* d = nullptr;
	if (hipMalloc(&d, (v.size() + 1) * sizeof(T)) != hipSuccess) { return nullptr; }
	if (!v.empty()) { (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); }
	return d;
}

static bool allocMeshOut(vgx_mesh_out* out, uint64_t nv, uint64_t ni, uint64_t nm)
{
	memset(out, 0, sizeof(*out));
	out->cap_vertices = nv; out->cap_indices = ni; out->cap_meshes = nm;
	return hipMalloc(&out->pos, (nv + 1) * 2 * sizeof(float)) == hipSuccess && hipMalloc(&out->color, (nv + 1) * sizeof(uint32_t)) == hipSuccess
	    && hipMalloc(&out->idx, (ni + 1) * sizeof(uint16_t)) == hipSuccess && hipMalloc(&out->meshes, (nm + 1) * sizeof(vgx_mesh)) == hipSuccess;
}

static const char* routeName(uint32_t r)
{
	static const char* names[] = { "no mesh", "triangles", "refused: several sub-paths", "refused: too long", "refused: not finite", "refused: degenerate",
	                               "refused: not simple", "refused: no ear found", "refused: nesting", "refused: no bridge" };
	return r < 10u ? names[r] : "?";
}

// a rectangular ring: counter-clockwise as the outlines below, or reversed as a hole
static void square(float* xy, float x, float y, float w, float h, bool hole)
{
	const float p[8] = { x, y, x + w, y, x + w, y + h, x, y + h };
	for (int k = 0; k < 4; ++k) { const int s = hole ? 3 - k : k; xy[2 * k] = p[2 * s]; xy[2 * k + 1] = p[2 * s + 1]; }
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_concave_nested_example.ppm";
	const uint32_t width = 160, height = 64;

	// ---- the list ----
	ListWriter L;
	L.rect(0.0f, 0.0f, 160.0f, 64.0f); L.fillColor(0u, 0xFF302820u);                                    // 0 the backdrop: a convex fill
	float xy[2 * 64];
	int four[16];
	int nr = 0;
	for (int k = 0; k < 7; ++k) { // "oBioBio": every glyph's outlines and counters, all in ONE path
		const float x = 2.0f + 13.0f * (float)k;
		const char ch = "oBioBio"[k];
		if (ch == 'o') {
			square(xy + 8 * nr++, x, 10.0f, 10.0f, 10.0f, false); square(xy + 8 * nr++, x + 2.5f, 12.5f, 5.0f, 5.0f, true);
		} else if (ch == 'B') {
			square(xy + 8 * nr++, x, 10.0f, 10.0f, 14.0f, false); square(xy + 8 * nr++, x + 2.0f, 12.0f, 3.5f, 3.5f, true); square(xy + 8 * nr++, x + 2.0f, 18.0f, 3.5f, 3.5f, true);
		} else {
			square(xy + 8 * nr++, x + 3.0f, 15.0f, 4.0f, 10.0f, false); square(xy + 8 * nr++, x + 3.0f, 9.0f, 4.0f, 4.0f, false); // the stem, the dot
		}
	}
	for (int r = 0; r < 16; ++r) { four[r] = 4; }
	L.rings(xy, four, nr); L.fillColor(FF_Concave, 0xC020C0FFu);                                        // 1 the word: 16 sub-paths, 9 groups
	for (int r = 0; r < 5; ++r) { square(xy + 8 * r, 100.0f + 4.0f * (float)r, 4.0f + 4.0f * (float)r, 56.0f - 8.0f * (float)r, 56.0f - 8.0f * (float)r, (r & 1) != 0); }
	L.rings(xy, four, 5); L.fillColor(FF_Concave | FF_AA, 0xC0FF8020u);                                 // 2 the target: 5 nested squares, 3 groups, anti-aliased

	// ---- host: decode (count pass, then store pass) ----
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
	o.cmd_type = cmdType.data(); o.cmd_arg_off = argOff.data(); o.args = args.data(); o.path_cmd_begin = pathBegin.data();
	o.draws = draws.data(); o.draw_state = dstate.data();
	o.cap_cmds = o.num_cmds; o.cap_args = o.num_args; o.cap_paths = o.num_paths; o.cap_draws = o.num_draws;
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));
	if (nr != 16 || o.num_draws != 3 || o.num_skipped != 0) { fprintf(stderr, "unexpected decode\n"); return 1; }
	const uint32_t nd = o.num_draws;

	// ---- device: sequence a, the polylines, the routes ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = upload(draws);
	vgx_draw_state* devState = upload(dstate);
	vgx_sizes sa, sf;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, nd, &sa, nullptr));
	vgx_mesh_out A;
	if (!allocMeshOut(&A, sa.num_vertices, sa.num_indices, sa.num_meshes)) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, nd, &A, nullptr));
	CHECK(vgx_flatten_count(ctx, ps, devDraws, nd, &sf, nullptr));
	vgx_flat_out flat = {};
	flat.cap_poly_vertices = sf.num_poly_vertices; flat.cap_subpaths = sf.num_subpaths;
	if (hipMalloc(&flat.poly, (sf.num_poly_vertices + 1) * 2 * sizeof(float)) != hipSuccess || hipMalloc(&flat.subpaths, (sf.num_subpaths + 1) * sizeof(vgx_subpath)) != hipSuccess
	    || hipMalloc(&flat.draw_info, (nd + 1) * sizeof(vgx_draw_info)) != hipSuccess) {
		return 1;
	}
	CHECK(vgx_flatten_emit(ctx, ps, devDraws, nd, 1 /* transformed */, &flat, nullptr));
	// capacities that need no look at the output: 3 vertices and 11 indices per polyline vertex cover both routes (6 V of fringe and
	// fewer than 5 V of triangles), 2 meshes per draw
	vgx_mesh_out B;
	if (!allocMeshOut(&B, 3 * sf.num_poly_vertices, 11 * sf.num_poly_vertices, 2ull * nd)) { return 1; }
	vgx_sizes* devSizes = nullptr;
	uint32_t* devWords = nullptr; // [0] a status, [1] a command count, [2 ..] the routes
	if (hipMalloc(&devSizes, sizeof(vgx_sizes)) != hipSuccess || hipMalloc(&devWords, (2 + nd) * sizeof(uint32_t)) != hipSuccess) { return 1; }
	std::vector<uint32_t> words(2 + nd);
	vgx_sizes sb;
	CHECK(vgx_concave_triangulate_nested(ctx, flat.poly, flat.subpaths, flat.draw_info, devDraws, nd, &B, devWords + 2, devSizes, devWords, nullptr));
	if (hipMemcpy(&sb, devSizes, sizeof(sb), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(words.data(), devWords, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (words[0] != VGX_OK) { fprintf(stderr, "vgx_concave_triangulate_nested: %s\n", vgx_status_string((int)words[0])); return 1; }
	for (uint32_t d = 0; d < nd; ++d) { printf("draw %u: %s\n", d, routeName(words[2 + d])); }
	if (words[2] != 0u || words[3] != VGX_TRI_ROUTE_TRIANGLES || words[4] != VGX_TRI_ROUTE_TRIANGLES) {
		fprintf(stderr, "unexpected routes\n");
		return 1;
	}
	const vgx_cache_desc seqA = { A.pos, A.color, A.idx, A.meshes, sa.num_meshes, sa.num_vertices, sa.num_indices };
	const vgx_cache_desc seqB = { B.pos, B.color, B.idx, B.meshes, sb.num_meshes, sb.num_vertices, sb.num_indices };

	// ---- three picks on the triangles: the dot of the first "i", the counter of the first "o", the innermost square of the target ----
	const vgx_pick_query queries[3] = { { 33.0f, 11.0f, 0xFFFFFFFFu, 0u }, { 7.0f, 15.0f, 0xFFFFFFFFu, 0u }, { 128.0f, 32.0f, 0xFFFFFFFFu, 0u } };
	vgx_pick_query* devQueries = nullptr;
	vgx_pick_hit* devHits = nullptr;
	if (hipMalloc(&devQueries, sizeof(queries)) != hipSuccess || hipMalloc(&devHits, 3 * sizeof(vgx_pick_hit)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devQueries, queries, sizeof(queries), hipMemcpyHostToDevice);
	CHECK(vgx_pick(ctx, &seqB, nullptr, devQueries, 3, devHits, nullptr));
	vgx_pick_hit hits[3];
	if (hipMemcpy(hits, devHits, sizeof(hits), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	printf("pick (33, 11) on the dot of the i: mesh %d of draw %d\n", (int)hits[0].mesh, (int)hits[0].draw);
	printf("pick (7, 15) in the counter of the o: %s\n", hits[1].mesh == 0xFFFFFFFFu ? "nothing" : "a mesh");
	printf("pick (128, 32) on the innermost square: mesh %d of draw %d\n", (int)hits[2].mesh, (int)hits[2].draw);
	if (hits[0].mesh != 0u || hits[0].draw != 1u || hits[1].mesh != 0xFFFFFFFFu || hits[2].mesh != 1u || hits[2].draw != 2u) { fprintf(stderr, "unexpected picks\n"); return 1; }

	// ---- merge under an armed assembly ----
	const uint64_t capCmds = 64;
	const uint64_t nv = sa.num_vertices + sb.num_vertices, ni = sa.num_indices + sb.num_indices, nm = sa.num_meshes + sb.num_meshes;
	vgx_assembly as;
	memset(&as, 0, sizeof(as));
	as.cap_drawcmds = capCmds; as.max_vb_vertices = 512; as.flags = VGX_ASM_SPLIT_STATE;
	as.uv_bytes = 4; as.uv_value[0] = 0x40004000u; // int16 x 2: (0.5, 0.5) of the white image below
	if (hipMalloc(&as.drawcmds, capCmds * sizeof(vgx_drawcmd)) != hipSuccess || hipMalloc(&as.dev_num_drawcmds, sizeof(uint64_t)) != hipSuccess
	    || hipMalloc(&as.uv, (size_t)(nv + 1) * 4) != hipSuccess) {
		return 1;
	}
	vgx_mesh_out out;
	if (!allocMeshOut(&out, nv, ni, nm)) { return 1; }
	CHECK(vgx_set_assembly(ctx, &as));
	CHECK(vgx_merge(ctx, &seqA, &seqB, nullptr, devDraws, nd, &out, nullptr, devWords, nullptr));
	CHECK(vgx_set_assembly(ctx, nullptr));
	uint32_t status = 77;
	if (hipMemcpy(&status, devWords, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (status != VGX_OK) { fprintf(stderr, "vgx_merge: %s\n", vgx_status_string((int)status)); return 1; }

	// ---- the command table and the image ----
	const vgx_raster_draws state = { devDraws, devState, nd, 0 };
	vgx_raster_cmd* devCmds = nullptr;
	if (hipMalloc(&devCmds, capCmds * sizeof(vgx_raster_cmd)) != hipSuccess) { return 1; }
	CHECK(vgx_raster_cmds_from_assembly(ctx, as.drawcmds, capCmds, as.dev_num_drawcmds, out.meshes, nm, &state, devCmds, devWords + 1, devWords, nullptr));
	if (hipMemcpy(words.data(), devWords, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (words[0] != VGX_OK) { fprintf(stderr, "vgx_raster_cmds_from_assembly: %s\n", vgx_status_string((int)words[0])); return 1; }
	printf("assembled frame: %llu meshes, %llu vertices, %llu indices -> %u draw commands\n", (unsigned long long)nm, (unsigned long long)nv, (unsigned long long)ni, words[1]);
	const uint32_t white[4] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
	uint32_t* devWhite = nullptr;
	vgx_raster_image* devImages = nullptr;
	if (hipMalloc(&devWhite, sizeof(white)) != hipSuccess || hipMalloc(&devImages, sizeof(vgx_raster_image)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devWhite, white, sizeof(white), hipMemcpyHostToDevice);
	const vgx_raster_image image = { devWhite, 2, 2, 2, VGX_IMAGE_NEAREST }; // the white pixel every colour command samples
	(void)hipMemcpy(devImages, &image, sizeof(image), hipMemcpyHostToDevice);
	vgx_raster_streams streams;
	memset(&streams, 0, sizeof(streams));
	streams.pos = out.pos; streams.color = out.color; streams.uv = as.uv; streams.idx = out.idx;
	streams.num_vertices = nv; streams.num_indices = ni; streams.uv_bytes = 4;
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFE8E0D8u;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	uint32_t calls = 0;
	status = VGX_E_GROWN;
	while (status == VGX_E_GROWN && calls < 3) {
		CHECK(vgx_raster_commands(ctx, &streams, devCmds, (uint32_t)capCmds, devWords + 1, devImages, 1, nullptr, &tgt, devWords, nullptr));
		if (hipMemcpy(&status, devWords, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		++calls;
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_commands: %s\n", vgx_status_string((int)status)); return 1; }
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
		painted += c != 0xFF302820u;
	}
	FILE* f = fopen(ppmPath, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppmPath); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	fwrite(rgb.data(), 1, rgb.size(), f);
	fclose(f);
	printf("rendered %u x %u in %u call%s: %u pixels off the backdrop, written to %s\n", width, height, calls, calls == 1 ? "" : "s", painted, ppmPath);
	printf("digest %016llx\n", (unsigned long long)digest);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return painted > 1500 ? 0 : 1;
}
