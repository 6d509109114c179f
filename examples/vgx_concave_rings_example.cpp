// vgx_concave_rings_example.cpp -- fills with HOLES as triangles without libtess2 and without leaving the device, through the C-ABI (no
// Python, no torch, no display GPU): a command list with a donut, a "B" and a framed picture, from its bytes to a draw-command table,
// pixels and two picks.
//   bytes of a command list (written here by hand in the reference's wire format)
//   -> vgx_cmdlist_decode (host): paths + draws + per-draw state; the three fills with holes are draws with VGX_FILL_CONCAVE of two or
//      three sub-paths each
//   -> vgx_tessellate_count / _emit (device): the meshes of the convex draws (sequence a)
//   -> vgx_flatten_count / _emit (device): the transformed polylines and sub-paths of the frame's draws
//   -> vgx_concave_triangulate_rings (device): every one of the three is one outer ring with holes directly inside it and comes out as
//      triangles (the "B" and the frame behind their AA fringes). vgx_concave_triangulate would refuse all three as
//      VGX_TRI_REFUSED_MULTI. The routes are the only thing the host reads back here.
//   -> vgx_pick on the triangles: a point on the donut's rim hits its mesh, a point in its hole hits nothing
//   -> vgx_merge under vgx_set_assembly (VGX_ASM_SPLIT_STATE): vertex buffers, ONE index buffer, the draw-command table
//   -> vgx_raster_cmds_from_assembly -> vgx_raster_commands: a 160 x 64 RGBA8 image, written as a binary PPM, and its digest (FNV-1a)
//   hipcc -O2 -I include examples/vgx_concave_rings_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_concave_rings_example
//   ./vgx_concave_rings_example [out.ppm]
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

// a square ring: counter-clockwise as the outer rings below, or reversed as a hole
static void square(float* xy, float x, float y, float w, float h, bool hole)
{
	const float p[8] = { x, y, x + w, y, x + w, y + h, x, y + h };
	for (int k = 0; k < 4; ++k) { const int s = hole ? 3 - k : k; xy[2 * k] = p[2 * s]; xy[2 * k + 1] = p[2 * s + 1]; }
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_concave_rings_example.ppm";
	const uint32_t width = 160, height = 64;

	// ---- the list ----
	ListWriter L;
	L.rect(0.0f, 0.0f, 160.0f, 64.0f); L.fillColor(0u, 0xFF302820u);                                    // 0 the backdrop: a convex fill
	const int four[3] = { 4, 4, 4 };
	float xy[24];
	square(xy, 8.0f, 8.0f, 40.0f, 40.0f, false); square(xy + 8, 18.0f, 18.0f, 20.0f, 20.0f, true);
	L.rings(xy, four, 2); L.fillColor(FF_Concave, 0xC020C0FFu);                                         // 1 a donut
	square(xy, 60.0f, 8.0f, 40.0f, 48.0f, false); square(xy + 8, 68.0f, 14.0f, 14.0f, 14.0f, true); square(xy + 16, 68.0f, 34.0f, 18.0f, 16.0f, true);
	L.rings(xy, four, 3); L.fillColor(FF_Concave | FF_AA, 0xC0FF8020u);                                 // 2 a "B": two counters, anti-aliased
	square(xy, 110.0f, 8.0f, 42.0f, 48.0f, false); square(xy + 8, 116.0f, 14.0f, 30.0f, 36.0f, true);
	L.rings(xy, four, 2); L.fillColor(FF_Concave | FF_AA, 0xFF60E0E0u);                                 // 3 a picture frame, anti-aliased
	L.rect(119.0f, 17.0f, 24.0f, 30.0f); L.fillColor(0u, 0xFF4060C0u);                                  // 4 the picture: a convex fill

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
	if (o.num_draws != 5 || o.num_skipped != 0) { fprintf(stderr, "unexpected decode\n"); return 1; }
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
	CHECK(vgx_concave_triangulate_rings(ctx, flat.poly, flat.subpaths, flat.draw_info, devDraws, nd, &B, devWords + 2, devSizes, devWords, nullptr));
	if (hipMemcpy(&sb, devSizes, sizeof(sb), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(words.data(), devWords, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (words[0] != VGX_OK) { fprintf(stderr, "vgx_concave_triangulate_rings: %s\n", vgx_status_string((int)words[0])); return 1; }
	for (uint32_t d = 0; d < nd; ++d) { printf("draw %u: %s\n", d, routeName(words[2 + d])); }
	if (words[2] != 0u || words[3] != VGX_TRI_ROUTE_TRIANGLES || words[4] != VGX_TRI_ROUTE_TRIANGLES || words[5] != VGX_TRI_ROUTE_TRIANGLES || words[6] != 0u) {
		fprintf(stderr, "unexpected routes\n");
		return 1;
	}
	const vgx_cache_desc seqA = { A.pos, A.color, A.idx, A.meshes, sa.num_meshes, sa.num_vertices, sa.num_indices };
	const vgx_cache_desc seqB = { B.pos, B.color, B.idx, B.meshes, sb.num_meshes, sb.num_vertices, sb.num_indices };

	// ---- two picks on the triangles: the donut's rim, the donut's hole ----
	const vgx_pick_query queries[2] = { { 12.0f, 12.0f, 0xFFFFFFFFu, 0u }, { 28.0f, 28.0f, 0xFFFFFFFFu, 0u } };
	vgx_pick_query* devQueries = nullptr;
	vgx_pick_hit* devHits = nullptr;
	if (hipMalloc(&devQueries, sizeof(queries)) != hipSuccess || hipMalloc(&devHits, 2 * sizeof(vgx_pick_hit)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devQueries, queries, sizeof(queries), hipMemcpyHostToDevice);
	CHECK(vgx_pick(ctx, &seqB, nullptr, devQueries, 2, devHits, nullptr));
	vgx_pick_hit hits[2];
	if (hipMemcpy(hits, devHits, sizeof(hits), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	printf("pick (12, 12) on the rim: mesh %d of draw %d\n", (int)hits[0].mesh, (int)hits[0].draw);
	printf("pick (28, 28) in the hole: %s\n", hits[1].mesh == 0xFFFFFFFFu ? "nothing" : "a mesh");
	if (hits[0].mesh != 0u || hits[0].draw != 1u || hits[1].mesh != 0xFFFFFFFFu) { fprintf(stderr, "unexpected picks\n"); return 1; }

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
	return painted > 2000 ? 0 : 1;
}
