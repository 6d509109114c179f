// vgx_pick_commands_example.cpp -- what is under the cursor in an ASSEMBLED frame, and what lies below it, through the C-ABI (no Python, no
// torch, no display GPU). The program writes command-list bytes as vg::clXxx records them -- a backdrop and four discs that overlap under the
// cursor -- then
//   vgx_cmdlist_decode              host: paths, draws and one vgx_draw_state per draw
//   vgx_set_assembly                VGX_ASM_SPLIT_STATE: vertex streams, ONE index buffer with command-relative indices, the draw-command table
//   vgx_tessellate_count / _emit    all five drawings share their state, so they land in ONE draw command
//   vgx_raster_cmds_from_assembly   device: the table vgx_raster_commands draws and vgx_pick_commands hit-tests
//   vgx_pick_commands               with the frame's mesh table as `owners`: the hit names the command, the triangle inside it, and the mesh
//                                   and the draw that own the triangle
// and walks the stack down twice: the next query stops below the mesh that was hit, INSIDE the command (cmd_end = the command, tri_end = the
// first triangle of the hit mesh). The test suite checks the printed hits against the numpy model of the specification in include/vgx.h.
//   hipcc -O2 -I include examples/vgx_pick_commands_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_pick_commands_example
//   ./vgx_pick_commands_example [frame.bin]     frame.bin: streams, command table and mesh table as raw arrays, for whoever wants to check
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
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
enum { CT_BeginPath = 0, CT_Rect = 7, CT_Circle = 10, CT_FillPathColor = 14 };
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
	void f(uint32_t type, std::initializer_list<float> v) { std::vector<float> a(v); cmd(type, a.data(), (uint32_t)a.size() * 4); }
	void fill(uint32_t color) { const uint32_t p[2] = { 0u, color }; cmd(CT_FillPathColor, p, 8); } // no AA: one mesh per drawing
	void rect(float x, float y, float w, float h, uint32_t color) { cmd(CT_BeginPath, nullptr, 0); f(CT_Rect, { x, y, w, h }); fill(color); }
	void circle(float x, float y, float r, uint32_t color) { cmd(CT_BeginPath, nullptr, 0); f(CT_Circle, { x, y, r }); fill(color); }
};

int main(int argc, char** argv)
{
	const char* framePath = argc > 1 ? argv[1] : nullptr;
	const uint32_t width = 256, height = 192;
	const float cursor[2] = { 128.5f, 96.5f };

	// ---- the frame: a backdrop (draw 0) and four discs (draws 1 .. 4) that all hold the cursor ----
	ListWriter L;
	L.rect(0.0f, 0.0f, 256.0f, 192.0f, 0xFFF0E8E0u);
	L.circle(110.0f, 90.0f, 40.0f, 0xFF2040C0u);
	L.circle(140.0f, 84.0f, 36.0f, 0xFF20C040u);
	L.circle(128.0f, 116.0f, 34.0f, 0xFFC04020u);
	L.circle(134.0f, 100.0f, 12.0f, 0xFF00C0C0u);

	vgx_cmdlist_state st = {};
	st.mtx[0] = 1.0f; st.mtx[3] = 1.0f; st.global_alpha = 1.0f; st.tess_tol = 0.25f; st.fringe = 1.0f;
	st.canvas_width = (float)width; st.canvas_height = (float)height;
	vgx_cmdlist_out o = {};
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));
	std::vector<uint8_t> cmdType(o.num_cmds + 1);
	std::vector<uint32_t> argOff(o.num_cmds + 1), pathBegin(o.num_paths + 1);
	std::vector<float> args(o.num_args + 1);
	std::vector<vgx_draw> draws(o.num_draws + 1);
	std::vector<vgx_draw_state> dstate(o.num_draws + 1);
	o.cmd_type = cmdType.data(); o.cmd_arg_off = argOff.data(); o.args = args.data(); o.path_cmd_begin = pathBegin.data();
	o.draws = draws.data(); o.draw_state = dstate.data();
	o.cap_cmds = o.num_cmds; o.cap_args = o.num_args; o.cap_paths = o.num_paths; o.cap_draws = o.num_draws;
	CHECK(vgx_cmdlist_decode(L.b.data(), (uint32_t)L.b.size(), &st, &o));

	// ---- device: tessellate under an armed assembly ----
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	vgx_pathset_desc desc = { cmdType.data(), argOff.data(), args.data(), pathBegin.data(), o.num_paths, o.num_cmds };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* devDraws = nullptr;
	vgx_draw_state* devState = nullptr;
	if (hipMalloc(&devDraws, o.num_draws * sizeof(vgx_draw)) != hipSuccess || hipMalloc(&devState, o.num_draws * sizeof(vgx_draw_state)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), o.num_draws * sizeof(vgx_draw), hipMemcpyHostToDevice);
	(void)hipMemcpy(devState, dstate.data(), o.num_draws * sizeof(vgx_draw_state), hipMemcpyHostToDevice);
	const uint64_t capCmds = 64;
	vgx_assembly as;
	memset(&as, 0, sizeof(as));
	as.cap_drawcmds = capCmds; as.max_vb_vertices = 65535; as.flags = VGX_ASM_SPLIT_STATE; // no UV stream: a hit needs none
	if (hipMalloc(&as.drawcmds, capCmds * sizeof(vgx_drawcmd)) != hipSuccess || hipMalloc(&as.dev_num_drawcmds, sizeof(uint64_t)) != hipSuccess) { return 1; }
	CHECK(vgx_set_assembly(ctx, &as));
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, o.num_draws, &sz, nullptr));
	if (sz.num_drawcmds > capCmds) { fprintf(stderr, "the frame outgrew the example's buffers\n"); return 1; }
	vgx_mesh_out out;
	memset(&out, 0, sizeof(out));
	out.cap_vertices = sz.num_vertices; out.cap_indices = sz.num_indices; out.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&out.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out.color, out.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, out.cap_indices * sizeof(uint16_t));
	if (hipMalloc(&out.meshes, out.cap_meshes * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, o.num_draws, &out, nullptr));
	CHECK(vgx_set_assembly(ctx, nullptr));

	// ---- the command table, on the device ----
	const vgx_raster_draws state = { devDraws, devState, o.num_draws, 0 };
	vgx_raster_cmd* devCmds = nullptr;
	uint32_t* devWords = nullptr; // [0] the command count, [1] a status
	if (hipMalloc(&devCmds, capCmds * sizeof(vgx_raster_cmd)) != hipSuccess || hipMalloc(&devWords, 2 * sizeof(uint32_t)) != hipSuccess) { return 1; }
	CHECK(vgx_raster_cmds_from_assembly(ctx, as.drawcmds, capCmds, as.dev_num_drawcmds, out.meshes, sz.num_meshes, &state, devCmds, devWords, devWords + 1, nullptr));
	uint32_t words[2] = { 0, 77 };
	if (hipMemcpy(words, devWords, sizeof(words), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	if (words[1] != VGX_OK) { fprintf(stderr, "vgx_raster_cmds_from_assembly: %s\n", vgx_status_string((int)words[1])); return 1; }
	const uint32_t numCmds = words[0];
	std::vector<vgx_raster_cmd> cmds(numCmds);
	std::vector<vgx_mesh> meshes(sz.num_meshes);
	if (hipMemcpy(cmds.data(), devCmds, numCmds * sizeof(vgx_raster_cmd), hipMemcpyDeviceToHost) != hipSuccess
	 || hipMemcpy(meshes.data(), out.meshes, meshes.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	uint64_t triangles = 0;
	for (uint32_t c = 0; c < numCmds; ++c) { triangles += cmds[c].num_indices / 3u; }
	printf("list: %zu bytes -> %u draws -> %llu meshes in %u draw command%s, %llu triangles\n", L.b.size(), o.num_draws, (unsigned long long)sz.num_meshes, numCmds,
	       numCmds == 1 ? "" : "s", (unsigned long long)triangles);

	// ---- pick, then walk the stack down twice ----
	vgx_raster_streams streams;
	memset(&streams, 0, sizeof(streams));
	streams.pos = out.pos; streams.color = out.color; streams.idx = out.idx;
	streams.num_vertices = sz.num_vertices; streams.num_indices = sz.num_indices;
	const vgx_pick_owners owners = { out.meshes, sz.num_meshes };
	vgx_pick_cmd_query* devQ = nullptr;
	vgx_pick_cmd_hit* devH = nullptr;
	if (hipMalloc(&devQ, sizeof(vgx_pick_cmd_query)) != hipSuccess || hipMalloc(&devH, sizeof(vgx_pick_cmd_hit)) != hipSuccess) { return 1; }
	vgx_pick_cmd_query q;
	memset(&q, 0, sizeof(q));
	q.x = cursor[0]; q.y = cursor[1]; q.cmd_end = 0xFFFFFFFFu; q.tri_end = 0u;
	uint32_t walked[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
	for (int step = 0; step < 3; ++step) {
		vgx_pick_cmd_hit h;
		uint32_t status = 77;
		if (hipMemcpy(devQ, &q, sizeof(q), hipMemcpyHostToDevice) != hipSuccess) { return 1; }
		CHECK(vgx_pick_commands(ctx, &streams, devCmds, (uint32_t)capCmds, devWords, &owners, devQ, 1, devH, devWords + 1, nullptr));
		if (hipMemcpy(&h, devH, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&status, devWords + 1, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		if (status != VGX_OK) { fprintf(stderr, "vgx_pick_commands: %s\n", vgx_status_string((int)status)); return 1; }
		if (h.cmd == 0xFFFFFFFFu || h.mesh == 0xFFFFFFFFu) { printf("%s: nothing\n", step ? "below" : "cursor"); break; }
		printf("%s (%.1f, %.1f) limit (%d, %u): command %u triangle %u mesh %u draw %u\n", step ? "below " : "cursor", q.x, q.y, (int)q.cmd_end, q.tri_end, h.cmd, h.triangle,
		       h.mesh, h.draw);
		walked[step] = h.draw;
		q.cmd_end = h.cmd;
		q.tri_end = (uint32_t)((meshes[h.mesh].first_index - cmds[h.cmd].first_index) / 3u); // the first triangle of the hit mesh: stop below it
	}

	if (framePath) { // six uint64 (vertices, indices, commands, meshes, width, height), then pos, color, idx, the command table, the mesh table
		std::vector<float> hpos(2 * sz.num_vertices); std::vector<uint32_t> hcol(sz.num_vertices); std::vector<uint16_t> hidx(sz.num_indices);
		(void)hipMemcpy(hpos.data(), out.pos, hpos.size() * sizeof(float), hipMemcpyDeviceToHost);
		(void)hipMemcpy(hcol.data(), out.color, hcol.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
		if (hipMemcpy(hidx.data(), out.idx, hidx.size() * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
		const uint64_t head[6] = { sz.num_vertices, sz.num_indices, numCmds, sz.num_meshes, width, height };
		FILE* g = fopen(framePath, "wb");
		if (!g) { fprintf(stderr, "cannot write %s\n", framePath); return 1; }
		fwrite(head, sizeof(head), 1, g);
		fwrite(hpos.data(), sizeof(float), hpos.size(), g); fwrite(hcol.data(), sizeof(uint32_t), hcol.size(), g);
		fwrite(hidx.data(), sizeof(uint16_t), hidx.size(), g); fwrite(cmds.data(), sizeof(vgx_raster_cmd), cmds.size(), g);
		fwrite(meshes.data(), sizeof(vgx_mesh), meshes.size(), g);
		fclose(g);
	}
	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return walked[0] == 4u && walked[1] == 3u && walked[2] == 2u ? 0 : 1;
}
