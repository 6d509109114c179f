// vgx_pick_frame_example.cpp -- what is under the cursor in the image of a decoded frame, through the C-ABI (no Python, no torch, no
// display GPU, no libtess2):
//   bytes of a command list (written here by hand in the reference's wire format): a backdrop, a square under a scissor, a bar under an In
//   region, a bar under an Out region, and a concave star
//   -> vgx_cmdlist_decode (host) -> vgx_tessellate_count / _emit -> vgx_flatten_count / _emit -> vgx_concave_contours -> vgx_merge (device):
//      the frame, as in vgx_concave_raster_example.cpp
//   -> vgx_raster_concave (device): the ID image -- the frame with every vertex colour of mesh m set to 0xFF000000 | (m + 1), drawn over a
//      clear of 0: a pixel holds the mesh that is visible there
//   -> vgx_pick (device): what bare triangles say at a few points, and vgx_pick_frame (device): what the image says
// vgx_pick hits the square where its scissor cut it away, the bars where their regions refuse them, and the clip meshes themselves, and it
// never hits the star (a contour mesh has no triangles). vgx_pick_frame names the mesh the ID image holds -- at the few points printed, and
// at EVERY pixel centre of the image: the example exits non-zero if one of them disagrees.
//   hipcc -O2 -I include examples/vgx_pick_frame_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_pick_frame_example
//   ./vgx_pick_frame_example [frame.bin]     frame.bin: streams and draws as raw arrays, for whoever wants to check
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
enum { CT_BeginPath = 0, CT_MoveTo = 1, CT_LineTo = 2, CT_Rect = 7, CT_ClosePath = 13, CT_FillPathColor = 14, CT_BeginClip = 21, CT_EndClip = 22,
       CT_ResetClip = 23, CT_ResetScissor = 30, CT_SetScissor = 31 };
enum { FF_Concave = 1u };
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
	void star(float cx, float cy, float r0, float r1, int n)
	{
		cmd(CT_BeginPath, nullptr, 0);
		for (int k = 0; k < n; ++k) {
			const float a = (float)k * 6.2831853f / (float)n - 1.5707963f, r = (k % 2) ? r1 : r0;
			point(k ? CT_LineTo : CT_MoveTo, cx + r * cosf(a), cy + r * sinf(a));
		}
		cmd(CT_ClosePath, nullptr, 0);
	}
	void rect(float x, float y, float w, float h) { cmd(CT_BeginPath, nullptr, 0); const float a[4] = { x, y, w, h }; cmd(CT_Rect, a, 16); }
	void fill(uint32_t flags, uint32_t color) { const uint32_t p[2] = { flags, color }; cmd(CT_FillPathColor, p, 8); }
	void clip(uint32_t rule) { cmd(CT_BeginClip, &rule, 4); }
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
	const char* framePath = argc > 1 ? argv[1] : nullptr;
	const uint32_t width = 96, height = 64;

	// ---- the list ----
	ListWriter L;
	L.rect(0.0f, 0.0f, 96.0f, 64.0f); L.fill(0u, 0xFF302820u);                      // draw 0: the backdrop
	const float sc[4] = { 8.0f, 8.0f, 16.0f, 16.0f };
	L.cmd(CT_SetScissor, sc, 16);
	L.rect(4.0f, 4.0f, 36.0f, 24.0f); L.fill(0u, 0xFF20C0FFu);                      // draw 1: a square, all but 16 x 16 pixels of it cut by the scissor
	L.cmd(CT_ResetScissor, nullptr, 0);
	L.clip(0u);
	L.rect(52.0f, 6.0f, 20.0f, 20.0f); L.fill(0u, 0xFF000000u);                     // draw 2: an In region ...
	L.cmd(CT_EndClip, nullptr, 0);
	L.rect(46.0f, 12.0f, 44.0f, 8.0f); L.fill(0u, 0xF0F0F020u);                     // draw 3: ... and a bar that shows inside it only
	L.cmd(CT_ResetClip, nullptr, 0);
	L.clip(1u);
	L.rect(12.0f, 38.0f, 16.0f, 18.0f); L.fill(0u, 0xFF000000u);                    // draw 4: an Out region ...
	L.cmd(CT_EndClip, nullptr, 0);
	L.rect(4.0f, 44.0f, 36.0f, 6.0f); L.fill(0u, 0xF020F0F0u);                      // draw 5: ... and a bar that shows outside it only
	L.cmd(CT_ResetClip, nullptr, 0);
	L.star(70.0f, 44.0f, 17.0f, 7.0f, 10); L.fill(FF_Concave, 0xE0FF8020u);        // draw 6: a concave star: a contour mesh

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
	std::vector<vgx_paint> paints(o.num_paints + 1);
	o.cmd_type = cmdType.data(); o.cmd_arg_off = argOff.data(); o.args = args.data(); o.path_cmd_begin = pathBegin.data();
	o.draws = draws.data(); o.draw_state = dstate.data(); o.paints = paints.data();
	o.cap_cmds = o.num_cmds; o.cap_args = o.num_args; o.cap_paths = o.num_paths; o.cap_draws = o.num_draws; o.cap_paints = o.num_paints;
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));
	printf("list: %zu bytes -> %u draws, %u skipped\n", L.b.size(), o.num_draws, o.num_skipped);
	if (o.num_draws != 7 || o.num_skipped != 0) { fprintf(stderr, "unexpected decode\n"); return 1; }

	// ---- device: the frame ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = upload(draws);
	vgx_draw_state* devState = upload(dstate);
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

	// ---- the ID image: the same streams with the colour of mesh m = 0xFF000000 | (m + 1), over a clear of 0 ----
	std::vector<vgx_mesh> meshes(nm);
	if (hipMemcpy(meshes.data(), out.meshes, nm * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	std::vector<uint32_t> idColor(nv, 0u);
	for (uint64_t m = 0; m < nm; ++m) {
		for (uint32_t v = 0; v < meshes[m].num_vertices; ++v) { idColor[meshes[m].first_vertex + v] = 0xFF000000u | (uint32_t)(m + 1); }
	}
	vgx_cache_desc idFrame = frame;
	idFrame.color = upload(idColor);
	// every draw of this list is a colour draw (type 0) or a Clip draw (type 3): no draw needs retyping and no kind carries UVs
	uint32_t* devUV = nullptr; // never read: no mesh is sampled
	if (hipMalloc(&devUV, (nv + 1) * sizeof(uint32_t)) != hipSuccess) { return 1; }
	const vgx_raster_draws rdraws = { devDraws, devState, o.num_draws, 0 };
	const vgx_raster_textures rtex = { devUV, nullptr, 4, 0 };
	const vgx_raster_paints rpaints = { nullptr, nullptr, 0, 0 };
	vgx_raster_target tgt;
	memset(&tgt, 0, sizeof(tgt));
	tgt.width = width; tgt.height = height; tgt.stride = width;
	tgt.scissor[2] = width; tgt.scissor[3] = height;
	tgt.flags = VGX_RASTER_CLEAR; tgt.clear_color = 0u;
	if (hipMalloc(&tgt.pixels, (size_t)width * height * sizeof(uint32_t)) != hipSuccess) { return 1; }
	status = VGX_E_GROWN;
	for (int calls = 0; status == VGX_E_GROWN && calls < 3; ++calls) {
		CHECK(vgx_raster_concave(ctx, &idFrame, nullptr, 0, nm, &rdraws, &rtex, &rpaints, &tgt, devStatus, nullptr));
		if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	}
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_concave: %s\n", vgx_status_string((int)status)); return 1; }
	std::vector<uint32_t> ids((size_t)width * height);
	if (hipMemcpy(ids.data(), tgt.pixels, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	const auto visible = [&](uint32_t i, uint32_t j) { const uint32_t c = ids[(size_t)j * width + i]; return c ? (c & 0xFFFFFFu) - 1u : 0xFFFFFFFFu; };

	// ---- a few points: vgx_pick against vgx_pick_frame ----
	struct Named { uint32_t i, j; const char* what; };
	const Named named[] = {
		{ 12, 12, "the square, inside its scissor" },     { 32, 20, "the square, cut away by its scissor" },
		{ 60, 16, "the bar, inside its In region" },      { 82, 16, "the bar, outside its In region" },
		{ 60, 8, "the In region's clip mesh alone" },     { 20, 46, "the bar, inside its Out region" },
		{ 34, 46, "the bar, outside its Out region" },    { 70, 44, "the middle of the star" },
		{ 70, 30, "a point of the star" },                { 90, 60, "the backdrop" },
	};
	const uint32_t nn = (uint32_t)(sizeof(named) / sizeof(named[0]));
	std::vector<vgx_pick_query> q(VGX_PICK_MAX_QUERIES);
	std::vector<vgx_pick_hit> hOld(VGX_PICK_MAX_QUERIES), hNew(VGX_PICK_MAX_QUERIES);
	vgx_pick_query* devQ = nullptr;
	vgx_pick_hit* devH = nullptr;
	if (hipMalloc(&devQ, q.size() * sizeof(vgx_pick_query)) != hipSuccess || hipMalloc(&devH, hNew.size() * sizeof(vgx_pick_hit)) != hipSuccess) { return 1; }
	for (uint32_t k = 0; k < nn; ++k) { q[k].x = (float)named[k].i + 0.5f; q[k].y = (float)named[k].j + 0.5f; q[k].mesh_end = 0xFFFFFFFFu; q[k].flags = 0u; }
	if (hipMemcpy(devQ, q.data(), nn * sizeof(vgx_pick_query), hipMemcpyHostToDevice) != hipSuccess) { return 1; }
	CHECK(vgx_pick(ctx, &frame, nullptr, devQ, nn, devH, nullptr));
	if (hipMemcpy(hOld.data(), devH, nn * sizeof(vgx_pick_hit), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	CHECK(vgx_pick_frame(ctx, &frame, nullptr, 0, nm, &rdraws, devQ, nn, devH, devStatus, nullptr));
	if (hipMemcpy(hNew.data(), devH, nn * sizeof(vgx_pick_hit), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	uint32_t differ = 0, wrong = 0;
	for (uint32_t k = 0; k < nn; ++k) {
		const uint32_t vis = visible(named[k].i, named[k].j);
		printf("point (%5.1f, %5.1f) %-38s vgx_pick: draw %2d mesh %2d   vgx_pick_frame: draw %2d mesh %2d   image: mesh %2d\n", q[k].x, q[k].y, named[k].what,
		       (int)hOld[k].draw, (int)hOld[k].mesh, (int)hNew[k].draw, (int)hNew[k].mesh, (int)vis);
		differ += hOld[k].mesh != hNew[k].mesh;
		wrong += hNew[k].mesh != vis;
	}

	// ---- every pixel centre: vgx_pick_frame against the ID image ----
	uint32_t checked = 0;
	for (uint32_t first = 0; first < width * height; first += VGX_PICK_MAX_QUERIES) {
		const uint32_t n = width * height - first < VGX_PICK_MAX_QUERIES ? width * height - first : VGX_PICK_MAX_QUERIES;
		for (uint32_t k = 0; k < n; ++k) { q[k].x = (float)((first + k) % width) + 0.5f; q[k].y = (float)((first + k) / width) + 0.5f; q[k].mesh_end = 0xFFFFFFFFu; q[k].flags = 0u; }
		if (hipMemcpy(devQ, q.data(), n * sizeof(vgx_pick_query), hipMemcpyHostToDevice) != hipSuccess) { return 1; }
		CHECK(vgx_pick_frame(ctx, &frame, nullptr, 0, nm, &rdraws, devQ, n, devH, devStatus, nullptr));
		if (hipMemcpy(hNew.data(), devH, n * sizeof(vgx_pick_hit), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		for (uint32_t k = 0; k < n; ++k) { wrong += hNew[k].mesh != visible((first + k) % width, (first + k) / width); ++checked; }
	}
	if (hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess || status != VGX_OK) { return 1; }
	printf("%u of %u named points differ between vgx_pick and vgx_pick_frame\n", differ, nn);
	printf("%u pixel centres checked against the ID image: %u disagree\n", checked, wrong);

	if (framePath) { // eight uint64 (meshes, vertices, indices, width, height, draws, 0, 0), then pos, color, idx, meshes, draws, draw states, the ID image
		std::vector<float> hpos(2 * nv); std::vector<uint32_t> hcol(nv); std::vector<uint16_t> hidx(ni);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[8] = { nm, nv, ni, width, height, o.num_draws, 0, 0 };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(meshes.data(), sizeof(vgx_mesh), meshes.size(), g);
		fwrite(draws.data(), sizeof(vgx_draw), draws.size(), g); fwrite(dstate.data(), sizeof(vgx_draw_state), dstate.size(), g);
		fwrite(ids.data(), sizeof(uint32_t), ids.size(), g);
		fclose(g);
	}
	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return wrong == 0 && differ >= 4 ? 0 : 1;
}
