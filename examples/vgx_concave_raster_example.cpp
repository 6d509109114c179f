// vgx_concave_raster_example.cpp -- a command list with concave fills, from its bytes to pixels, through the C-ABI (no Python, no torch,
// no display GPU, no libtess2):
//   bytes of a command list (written here by hand in the reference's wire format): a star under both fill rules, a ring with a hole, an
//   anti-aliased concave shape under a linear gradient, and a concave clip region with a bar drawn inside it
//   -> vgx_cmdlist_decode (host): paths + draws + per-draw state + paints; the concave fills are draws with VGX_FILL_CONCAVE and no mesh
//   -> vgx_tessellate_count / _emit (device): the meshes of every other draw (sequence a)
//   -> vgx_flatten_count / _emit (device): the transformed polylines and sub-paths of the frame's draws
//   -> vgx_concave_contours (device): contour meshes -- directed edges, no triangles -- for the concave draws (sequence b)
//   -> vgx_merge (device): both sequences interleaved by draw
//   -> vgx_raster_concave (device): the frame in a 192 x 128 RGBA8 image; a contour mesh is filled by the winding number of its edges
// Between decode and image only totals come back to the host (the counts every sequence's descriptor carries); no contour, vertex or
// index leaves the device. The image comes back once, is written as a binary PPM and summed into a digest (FNV-1a over the pixel words)
// that the test suite compares with the numpy model of the specification in include/vgx.h for the same frame.
//   hipcc -O2 -I include examples/vgx_concave_raster_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_concave_raster_example
//   ./vgx_concave_raster_example [out.ppm [frame.bin]]     frame.bin: streams, draws and paints as raw arrays, for whoever wants to check
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
enum { CT_BeginPath = 0, CT_MoveTo = 1, CT_LineTo = 2, CT_Rect = 7, CT_ClosePath = 13, CT_FillPathColor = 14, CT_FillPathGradient = 15, CT_BeginClip = 21,
       CT_EndClip = 22, CT_ResetClip = 23, CT_CreateLinearGradient = 24 };
// VG_FILL_FLAGS (include/vg/vg.h:229): PathType in bit 0, AA in bit 2, FillRule in bit 4
enum { FF_Concave = 1u, FF_AA = 4u, FF_EvenOdd = 16u };
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
	void point(uint32_t type, float x, float y) { const float a[2] = { x, y }; cmd(type, a, 8); }
	// a closed polygon of n points on two alternating radii; step > 1 joins every step-th point (a star polygon that crosses itself)
	void star(float cx, float cy, float r0, float r1, int n, int step)
	{
		cmd(CT_BeginPath, nullptr, 0);
		for (int k = 0; k < n; ++k) {
			const int v = (k * step) % n;
			const float a = (float)v * 6.2831853f / (float)n - 1.5707963f, r = (v % 2) ? r1 : r0;
			point(k ? CT_LineTo : CT_MoveTo, cx + r * cosf(a), cy + r * sinf(a));
		}
		cmd(CT_ClosePath, nullptr, 0);
	}
	void rect(float x, float y, float w, float h) { const float a[4] = { x, y, w, h }; cmd(CT_Rect, a, 16); }
	void fillColor(uint32_t flags, uint32_t color) { const uint32_t p[2] = { flags, color }; cmd(CT_FillPathColor, p, 8); }
	void fillGradient(uint32_t flags, uint16_t handle) { uint8_t p[8] = {}; memcpy(p, &flags, 4); memcpy(p + 4, &handle, 2); cmd(CT_FillPathGradient, p, 8); }
	void linearGradient(float sx, float sy, float ex, float ey, uint32_t inner, uint32_t outer)
	{
		uint8_t p[24];
		const float f[4] = { sx, sy, ex, ey };
		memcpy(p, f, 16); memcpy(p + 16, &inner, 4); memcpy(p + 20, &outer, 4);
		cmd(CT_CreateLinearGradient, p, 24);
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

static bool allocMeshOut(vgx_mesh_out* out, uint64_t nv, uint64_t ni, uint64_t nm)
{
	memset(out, 0, sizeof(*out));
	out->cap_vertices = nv; out->cap_indices = ni; out->cap_meshes = nm;
	return hipMalloc(&out->pos, (nv + 1) * 2 * sizeof(float)) == hipSuccess && hipMalloc(&out->color, (nv + 1) * sizeof(uint32_t)) == hipSuccess
	    && hipMalloc(&out->idx, (ni + 1) * sizeof(uint16_t)) == hipSuccess && hipMalloc(&out->meshes, (nm + 1) * sizeof(vgx_mesh)) == hipSuccess;
}

int main(int argc, char** argv)
{
	const char* ppmPath = argc > 1 ? argv[1] : "vgx_concave_raster_example.ppm";
	const char* framePath = argc > 2 ? argv[2] : nullptr;
	const uint32_t width = 192, height = 128;

	// ---- the list ----
	ListWriter L;
	L.cmd(CT_BeginPath, nullptr, 0); L.rect(0.0f, 0.0f, 192.0f, 128.0f); L.fillColor(0u, 0xFF302820u);                     // the backdrop: a convex fill
	L.star(34.0f, 34.0f, 28.0f, 28.0f, 5, 2); L.fillColor(FF_Concave, 0xE020C0FFu);                                       // a pentagram, NonZero: solid
	L.star(96.0f, 34.0f, 28.0f, 28.0f, 5, 2); L.fillColor(FF_Concave | FF_EvenOdd, 0xE0FF8020u);                          // ... EvenOdd: hollow centre
	L.cmd(CT_BeginPath, nullptr, 0); L.rect(132.0f, 8.0f, 52.0f, 52.0f); L.rect(146.0f, 22.0f, 24.0f, 24.0f);
	L.fillColor(FF_Concave | FF_EvenOdd | FF_AA, 0xFF60E060u);                                                           // a ring with a hole, AA
	L.linearGradient(8.0f, 70.0f, 88.0f, 120.0f, 0xFF20C0FFu, 0xFFFF4020u);                                               // gradient 0
	L.star(48.0f, 96.0f, 28.0f, 12.0f, 12, 1); L.fillGradient(FF_Concave | FF_AA, 0);                                     // an AA concave shape under it
	const uint32_t in = 0u;
	L.cmd(CT_BeginClip, &in, 4);
	L.star(140.0f, 96.0f, 30.0f, 13.0f, 10, 1); L.fillColor(FF_Concave, 0xFF000000u);                                     // a concave clip region ...
	L.cmd(CT_EndClip, nullptr, 0);
	L.cmd(CT_BeginPath, nullptr, 0); L.rect(104.0f, 84.0f, 84.0f, 24.0f); L.fillColor(0u, 0xF0F0F020u);                    // ... and a bar drawn In it
	L.cmd(CT_ResetClip, nullptr, 0);

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
	uint32_t concave = 0;
	for (const vgx_draw& d : draws) { concave += (d.fill_flags & VGX_FILL_CONCAVE) ? 1u : 0u; }
	printf("list: %zu bytes -> %u draws (%u concave), %u paints, %u skipped\n", L.b.size(), o.num_draws, concave, o.num_paints, o.num_skipped);
	if (o.num_draws != 7 || concave != 5 || o.num_paints != 1 || o.num_skipped != 0) { fprintf(stderr, "unexpected decode\n"); return 1; }
	std::vector<vgx_paint> gradients(o.next_gradient), patterns(o.next_image_pattern);
	CHECK(vgx_paint_tables(paints.data(), o.num_paints, gradients.data(), (uint32_t)gradients.size(), patterns.data(), (uint32_t)patterns.size()));

	// ---- device: sequence a, the contours, sequence b, the merged frame ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = upload(draws);
	vgx_draw_state* devState = upload(dstate);
	vgx_paint* devGradients = upload(gradients);
	vgx_sizes sa, sf;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, o.num_draws, &sa, nullptr));
	vgx_mesh_out A;
	if (!allocMeshOut(&A, sa.num_vertices, sa.num_indices, sa.num_meshes)) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, o.num_draws, &A, nullptr));
	CHECK(vgx_flatten_count(ctx, ps, devDraws, o.num_draws, &sf, nullptr));
	vgx_flat_out flat = {};
	flat.cap_poly_vertices = sf.num_poly_vertices; flat.cap_subpaths = sf.num_subpaths;
	if (hipMalloc(&flat.poly, (sf.num_poly_vertices + 1) * 2 * sizeof(float)) != hipSuccess || hipMalloc(&flat.subpaths, (sf.num_subpaths + 1) * sizeof(vgx_subpath)) != hipSuccess
	    || hipMalloc(&flat.draw_info, (o.num_draws + 1) * sizeof(vgx_draw_info)) != hipSuccess) {
		return 1;
	}
	CHECK(vgx_flatten_emit(ctx, ps, devDraws, o.num_draws, 1 /* transformed */, &flat, nullptr));
	// capacities that need no look at the output: 3 vertices and 8 indices per polyline vertex, 2 meshes per draw
	vgx_mesh_out B;
	if (!allocMeshOut(&B, 3 * sf.num_poly_vertices, 8 * sf.num_poly_vertices, 2ull * o.num_draws)) { return 1; }
	vgx_sizes* devSizes = nullptr;
	uint32_t* devStatus = nullptr;
	if (hipMalloc(&devSizes, sizeof(vgx_sizes)) != hipSuccess || hipMalloc(&devStatus, sizeof(uint32_t)) != hipSuccess) { return 1; }
	CHECK(vgx_concave_contours(ctx, flat.poly, flat.subpaths, flat.draw_info, devDraws, o.num_draws, &B, devSizes, devStatus, nullptr));
	vgx_sizes sb;
	uint32_t status = 0;
	if (hipMemcpy(&sb, devSizes, sizeof(sb), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (status != VGX_OK) { fprintf(stderr, "vgx_concave_contours: %s\n", vgx_status_string((int)status)); return 1; }
	const vgx_cache_desc seqA = { A.pos, A.color, A.idx, A.meshes, sa.num_meshes, sa.num_vertices, sa.num_indices };
	const vgx_cache_desc seqB = { B.pos, B.color, B.idx, B.meshes, sb.num_meshes, sb.num_vertices, sb.num_indices };
	const uint64_t nv = sa.num_vertices + sb.num_vertices, ni = sa.num_indices + sb.num_indices, nm = sa.num_meshes + sb.num_meshes;
	vgx_mesh_out out;
	if (!allocMeshOut(&out, nv, ni, nm)) { return 1; }
	CHECK(vgx_merge(ctx, &seqA, &seqB, nullptr, devDraws, o.num_draws, &out, nullptr, devStatus, nullptr));
	if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (status != VGX_OK) { fprintf(stderr, "vgx_merge: %s\n", vgx_status_string((int)status)); return 1; }
	const vgx_cache_desc frame = { out.pos, out.color, out.idx, out.meshes, nm, nv, ni };
	printf("frame: %llu meshes (%llu from contours), %llu vertices, %llu indices in device memory\n", (unsigned long long)nm, (unsigned long long)sb.num_meshes,
	       (unsigned long long)nv, (unsigned long long)ni);

	// ---- render ----
	uint32_t* devUV = nullptr; // no mesh of this frame is sampled: the stream is never read, but a range that is not empty needs one
	if (hipMalloc(&devUV, (nv + 1) * sizeof(uint32_t)) != hipSuccess) { return 1; }
	const vgx_raster_draws rdraws = { devDraws, devState, o.num_draws, 0 };
	const vgx_raster_textures rtex = { devUV, nullptr, 4, 0 };
	const vgx_raster_paints rpaints = { devGradients, nullptr, (uint32_t)gradients.size(), 0 };
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0xFFE8E0D8u;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	uint32_t calls = 0;
	status = VGX_E_GROWN;
	while (status == VGX_E_GROWN && calls < 3) {
		CHECK(vgx_raster_concave(ctx, &frame, nullptr, 0, nm, &rdraws, &rtex, &rpaints, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		++calls;
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_concave: %s\n", vgx_status_string((int)status)); return 1; }
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
	if (framePath) { // eight uint64 (meshes, vertices, indices, width, height, draws, paints, 0), then pos, color, idx, meshes, draws, draw states, paints
		std::vector<float> hpos(2 * nv); std::vector<uint32_t> hcol(nv); std::vector<uint16_t> hidx(ni); std::vector<vgx_mesh> hm(nm);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hm.data(), out.meshes, hm.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[8] = { nm, nv, ni, width, height, o.num_draws, o.num_paints, 0 };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(hm.data(), sizeof(vgx_mesh), hm.size(), g);
		fwrite(draws.data(), sizeof(vgx_draw), draws.size(), g); fwrite(dstate.data(), sizeof(vgx_draw_state), dstate.size(), g);
		fwrite(paints.data(), sizeof(vgx_paint), paints.size(), g);
		fclose(g);
	}
	printf("rendered %u x %u in %u call%s: %u pixels off the backdrop, written to %s\n", width, height, calls, calls == 1 ? "" : "s", painted, ppmPath);
	printf("digest %016llx\n", (unsigned long long)digest);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return painted > 3000 ? 0 : 1;
}
