// vgx_concave_triangulate_example.cpp -- concave fills as TRIANGLES without libtess2 and without leaving the device, through the C-ABI
// (no Python, no torch, no display GPU): a command list with a star, an anti-aliased L and a bow-tie, from its bytes to a draw-command
// table and pixels.
//   bytes of a command list (written here by hand in the reference's wire format)
//   -> vgx_cmdlist_decode (host): paths + draws + per-draw state; the three concave fills are draws with VGX_FILL_CONCAVE and no mesh
//   -> vgx_tessellate_count / _emit (device): the meshes of every other draw (sequence a)
//   -> vgx_flatten_count / _emit (device): the transformed polylines and sub-paths of the frame's draws
//   -> vgx_concave_triangulate (device): the star and the L are simple rings and come out as triangles (the L behind its AA fringe);
//      the bow-tie crosses itself, is refused with VGX_TRI_REFUSED_NOT_SIMPLE and holds vgx_concave_contours' edge mesh. The routes are
//      the only thing the host reads back here.
//   A draw-command table holds triangles: vgx_raster_cmds_from_assembly refuses a frame with an edge mesh. So the refused draw is taken
//   out of the assembled frame (its VGX_FILL_CONCAVE bit cleared: it makes no mesh) -- it stays with the contour route
//   (examples/vgx_concave_raster_example.cpp) or with libtess2 -- and the call is repeated for sequence b.
//   -> vgx_merge under vgx_set_assembly (VGX_ASM_SPLIT_STATE): vertex buffers, ONE index buffer, the draw-command table
//   -> vgx_raster_cmds_from_assembly -> vgx_raster_commands: a 128 x 96 RGBA8 image, written as a binary PPM, and its digest (FNV-1a)
//   hipcc -O2 -I include examples/vgx_concave_triangulate_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_concave_triangulate_example
//   ./vgx_concave_triangulate_example [out.ppm]
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
	                               "refused: not simple", "refused: no ear found" };
	return r < 8u ? names[r] : "?";
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_concave_triangulate_example.ppm";
	const uint32_t width = 128, height = 96;

	// ---- the list ----
	ListWriter L;
	L.rect(0.0f, 0.0f, 128.0f, 96.0f); L.fillColor(0u, 0xFF302820u);                                    // 0 the backdrop: a convex fill
	float star[20];
	for (int k = 0; k < 10; ++k) {
		const float a = (float)k * 0.62831853f - 1.5707963f, r = (k % 2) ? 10.0f : 26.0f;
		star[2 * k] = 34.0f + r * cosf(a); star[2 * k + 1] = 32.0f + r * sinf(a);
	}
	L.polygon(star, 10); L.fillColor(FF_Concave, 0xC020C0FFu);                                          // 1 a star
	const float ell[12] = { 70.0f, 8.0f, 120.0f, 8.0f, 120.0f, 26.0f, 90.0f, 26.0f, 90.0f, 58.0f, 70.0f, 58.0f };
	L.polygon(ell, 6); L.fillColor(FF_Concave | FF_AA, 0xC0FF8020u);                                    // 2 an L, anti-aliased
	const float bow[8] = { 12.0f, 64.0f, 60.0f, 90.0f, 60.0f, 64.0f, 12.0f, 90.0f };
	L.polygon(bow, 4); L.fillColor(FF_Concave, 0xC060E060u);                                            // 3 a bow-tie: it crosses itself

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
	if (o.num_draws != 4 || o.num_skipped != 0) { fprintf(stderr, "unexpected decode\n"); return 1; }
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
	// capacities that need no look at the output: 3 vertices and 9 indices per polyline vertex cover both routes, 2 meshes per draw
	vgx_mesh_out B;
	if (!allocMeshOut(&B, 3 * sf.num_poly_vertices, 9 * sf.num_poly_vertices, 2ull * nd)) { return 1; }
	vgx_sizes* devSizes = nullptr;
	uint32_t* devWords = nullptr; // [0] a status, [1] a command count, [2 ..] the routes
	if (hipMalloc(&devSizes, sizeof(vgx_sizes)) != hipSuccess || hipMalloc(&devWords, (2 + nd) * sizeof(uint32_t)) != hipSuccess) { return 1; }
	std::vector<uint32_t> words(2 + nd);
	vgx_sizes sb;
	for (int pass = 0; pass < 2; ++pass) {
		CHECK(vgx_concave_triangulate(ctx, flat.poly, flat.subpaths, flat.draw_info, devDraws, nd, &B, devWords + 2, devSizes, devWords, nullptr));
		if (hipMemcpy(&sb, devSizes, sizeof(sb), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(words.data(), devWords, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		if (words[0] != VGX_OK) { fprintf(stderr, "vgx_concave_triangulate: %s\n", vgx_status_string((int)words[0])); return 1; }
		if (pass == 1) { break; }
		uint32_t refused = 0;
		for (uint32_t d = 0; d < nd; ++d) {
			printf("draw %u: %s\n", d, routeName(words[2 + d]));
			if (words[2 + d] > VGX_TRI_ROUTE_TRIANGLES) { draws[d].fill_flags &= ~(uint32_t)VGX_FILL_CONCAVE; ++refused; } // not in the assembled frame
		}
		if (words[2] != 0u || words[3] != VGX_TRI_ROUTE_TRIANGLES || words[4] != VGX_TRI_ROUTE_TRIANGLES || words[5] != VGX_TRI_REFUSED_NOT_SIMPLE) {
			fprintf(stderr, "unexpected routes\n");
			return 1;
		}
		printf("first call: %llu meshes (the refused draw's is an edge mesh); %u draw left to the contour route\n", (unsigned long long)sb.num_meshes, refused);
		(void)hipMemcpy(devDraws, draws.data(), nd * sizeof(vgx_draw), hipMemcpyHostToDevice);
	}

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
	const vgx_cache_desc seqA = { A.pos, A.color, A.idx, A.meshes, sa.num_meshes, sa.num_vertices, sa.num_indices };
	const vgx_cache_desc seqB = { B.pos, B.color, B.idx, B.meshes, sb.num_meshes, sb.num_vertices, sb.num_indices };
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
