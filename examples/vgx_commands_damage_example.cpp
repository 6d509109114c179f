// vgx_commands_damage_example.cpp -- pick a cached drawing in an ASSEMBLED frame, drag it, and redraw only the tiles the drag can have
// changed, through the C-ABI (no Python, no torch). One drawing tessellated ONCE, ONE frame of 6 x 5 instances submitted under
// vgx_set_assembly (vertex buffers of 4 096 vertices, one index buffer with command-relative indices), turned into a draw-command table
// by vgx_raster_cmds_from_assembly. Then
//   vgx_command_bounds            the box of every command, once
//   vgx_raster_commands           the full render
//   vgx_pick_commands_boxed       what is under the cursor: a command whose box misses the point is not opened; the mesh table names the
//                                 drawing (vgx_mesh::draw is the instance)
// and, all on one stream and without a host visit between the edit and the image:
//   hipMemsetAsync                the damage bitmap: one bit per 16 x 16 tile of the image
//   vgx_damage_instances          the tiles the OLD boxes of the dragged drawing's meshes reach (the frame's vgx_mesh_bounds table)
//   vgx_cache_update              its slice of pos / color rewritten, its mesh boxes refreshed
//   vgx_damage_instances          the tiles the NEW boxes reach
//   vgx_command_bounds            over the commands that hold the drawing's meshes: their boxes refreshed, the others left alone
//   vgx_raster_commands_damaged   the marked tiles cleared and redrawn from the commands whose box reaches one, nothing else touched
// The image is checked against a full vgx_raster_commands of the edited frame, byte for byte, and written as a PPM.
//   hipcc -O2 -I include examples/vgx_commands_damage_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_commands_damage_example
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

// a raster call until it no longer asks for room (VGX_E_GROWN writes nothing, so repeating it is safe); false: another status
template <class Call>
static bool untilGrown(Call call, uint32_t* devStatus, const char* what)
{
	for (int k = 0; k < 4; ++k) {
		if (call() != VGX_OK) { return false; }
		uint32_t status = 0;
		(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
		if (status == VGX_OK) { return true; }
		if (status != VGX_E_GROWN) { fprintf(stderr, "%s: %s\n", what, vgx_status_string((int)status)); return false; }
	}
	fprintf(stderr, "%s: still growing\n", what);
	return false;
}

int main(int argc, char** argv)
{
	const char* ppm = argc > 1 ? argv[1] : "vgx_commands_damage_example.ppm";
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));

	// the drawing: 24 closed rings inside an 80 x 80 box, every other fill non-AA (it takes its instance's colour)
	const uint32_t npaths = 24;
	const float drawingSize = 80.0f;
	std::vector<uint8_t> cmdType;
	std::vector<uint32_t> cmdArgOff(1, 0u), pathCmdBegin(1, 0u);
	std::vector<float> args;
	uint32_t seed = 77u;
	for (uint32_t p = 0; p < npaths; ++p) {
		const uint32_t n = 8 + rnd(seed) % 17;
		const float r = 5.0f + (float)(rnd(seed) % 12);
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
		d.fill_flags = VGX_FILL_ENABLE | (p % 2 ? VGX_FILL_AA : 0u); d.fill_color = 0xC0000000u | rnd(seed);
		d.scale = 1.0f; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = 1.0f; d.mtx[3] = 1.0f;
		draws[p] = d;
	}
	vgx_draw* devDraws = nullptr;
	if (hipMalloc(&devDraws, npaths * sizeof(vgx_draw)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDraws, draws.data(), npaths * sizeof(vgx_draw), hipMemcpyHostToDevice);
	vgx_sizes sz;
	CHECK(vgx_tessellate_count(ctx, ps, devDraws, npaths, &sz, nullptr));
	vgx_mesh_out rec;
	memset(&rec, 0, sizeof(rec));
	rec.cap_vertices = sz.num_vertices; rec.cap_indices = sz.num_indices; rec.cap_meshes = sz.num_meshes;
	(void)hipMalloc(&rec.pos, rec.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&rec.color, rec.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&rec.idx, rec.cap_indices * sizeof(uint16_t));
	if (hipMalloc(&rec.meshes, rec.cap_meshes * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
	CHECK(vgx_tessellate_emit(ctx, ps, devDraws, npaths, &rec, nullptr));
	CHECK(vgx_cache_localize(ctx, devDraws, npaths, rec.pos, rec.meshes, sz.num_meshes, nullptr));
	const vgx_cache_desc cache = { rec.pos, rec.color, rec.idx, rec.meshes, sz.num_meshes, sz.num_vertices, sz.num_indices };

	// the frame: a 6 x 5 grid whose pitch is a little more than the drawing, in a 512 x 416 image, submitted under an armed assembly
	const uint32_t gridW = 6, gridH = 5, ninst = gridW * gridH, width = 512, height = 416;
	const float pitch = 84.0f;
	std::vector<vgx_cache_instance> inst(ninst);
	for (uint32_t i = 0; i < ninst; ++i) {
		vgx_cache_instance& in = inst[i];
		memset(&in, 0, sizeof(in));
		in.first_mesh = 0; in.num_meshes = (uint32_t)sz.num_meshes; in.color = 0xC0000000u | rnd(seed);
		in.mtx[0] = 1.0f; in.mtx[3] = 1.0f; in.mtx[4] = 4.0f + pitch * (float)(i % gridW); in.mtx[5] = 2.0f + pitch * (float)(i / gridW);
	}
	vgx_cache_instance* devInst = nullptr;
	(void)hipMalloc(&devInst, ninst * sizeof(vgx_cache_instance));
	(void)hipMemcpy(devInst, inst.data(), ninst * sizeof(vgx_cache_instance), hipMemcpyHostToDevice);
	vgx_mesh_out out;
	memset(&out, 0, sizeof(out));
	out.cap_vertices = sz.num_vertices * ninst; out.cap_indices = sz.num_indices * ninst; out.cap_meshes = sz.num_meshes * ninst;
	(void)hipMalloc(&out.pos, out.cap_vertices * 2 * sizeof(float));
	(void)hipMalloc(&out.color, out.cap_vertices * sizeof(uint32_t));
	(void)hipMalloc(&out.idx, out.cap_indices * sizeof(uint16_t));
	(void)hipMalloc(&out.meshes, out.cap_meshes * sizeof(vgx_mesh));
	vgx_sizes* devSizes = nullptr; uint32_t* devStatus = nullptr;
	(void)hipMalloc(&devSizes, sizeof(vgx_sizes));
	if (hipMalloc(&devStatus, 8 * sizeof(uint32_t)) != hipSuccess) { return 1; }
	const uint32_t maxVb = 4096;
	const uint64_t capCmds = 2 * out.cap_vertices / maxVb + 2 + ninst;
	vgx_assembly as;
	memset(&as, 0, sizeof(as));
	as.cap_drawcmds = capCmds; as.max_vb_vertices = maxVb; as.flags = VGX_ASM_SPLIT_STATE;
	as.uv_bytes = 4; as.uv_value[0] = 0x3FFF3FFFu; // every vertex samples the middle of the white image: the colour meshes of the reference
	if (hipMalloc(&as.drawcmds, capCmds * sizeof(vgx_drawcmd)) != hipSuccess || hipMalloc(&as.dev_num_drawcmds, sizeof(uint64_t)) != hipSuccess
	 || hipMalloc(&as.uv, out.cap_vertices * 4) != hipSuccess) { return 1; }
	CHECK(vgx_set_assembly(ctx, &as));
	CHECK(vgx_cache_submit(ctx, &cache, devInst, ninst, &out, devSizes, devStatus, nullptr));
	CHECK(vgx_set_assembly(ctx, nullptr));
	uint32_t status = 0; vgx_sizes got;
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&got, devSizes, sizeof(got), hipMemcpyDeviceToHost);
	if (status != VGX_OK) { fprintf(stderr, "submit: %s\n", vgx_status_string((int)status)); return 1; }
	vgx_cache_slot* devSlots = nullptr; float* devMeshBounds = nullptr;
	(void)hipMalloc(&devSlots, (ninst + 1) * sizeof(vgx_cache_slot));
	if (hipMalloc(&devMeshBounds, got.num_meshes * 4 * sizeof(float)) != hipSuccess) { return 1; }
	CHECK(vgx_cache_layout(ctx, &cache, devInst, ninst, devSlots, devStatus, nullptr));
	CHECK(vgx_mesh_bounds(ctx, out.pos, out.meshes, got.num_meshes, devMeshBounds, nullptr));

	// the command table: a cached frame is drawn with one plain draw per instance (vgx_cache_submit leaves the instance's index in vgx_mesh::draw)
	std::vector<vgx_draw_state> fstate(ninst);
	memset(fstate.data(), 0, ninst * sizeof(vgx_draw_state));
	for (uint32_t i = 0; i < ninst; ++i) { fstate[i].scissor[2] = 0xFFFFu; fstate[i].scissor[3] = 0xFFFFu; fstate[i].clip_first_draw = 0xFFFFFFFFu; }
	vgx_draw_state* devFState = nullptr;
	(void)hipMalloc(&devFState, ninst * sizeof(vgx_draw_state));
	(void)hipMemcpy(devFState, fstate.data(), ninst * sizeof(vgx_draw_state), hipMemcpyHostToDevice);
	const vgx_raster_draws state = { nullptr, devFState, ninst, 0 };
	vgx_raster_cmd* devCmds = nullptr; uint32_t* devNumCmds = nullptr; float* devCmdBounds = nullptr;
	if (hipMalloc(&devCmds, capCmds * sizeof(vgx_raster_cmd)) != hipSuccess || hipMalloc(&devNumCmds, sizeof(uint32_t)) != hipSuccess
	 || hipMalloc(&devCmdBounds, capCmds * 4 * sizeof(float)) != hipSuccess) { return 1; }
	CHECK(vgx_raster_cmds_from_assembly(ctx, as.drawcmds, capCmds, as.dev_num_drawcmds, out.meshes, got.num_meshes, &state, devCmds, devNumCmds, devStatus, nullptr));
	uint32_t numCmds = 0;
	(void)hipMemcpy(&numCmds, devNumCmds, sizeof(numCmds), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	if (status != VGX_OK) { fprintf(stderr, "vgx_raster_cmds_from_assembly: %s\n", vgx_status_string((int)status)); return 1; }
	std::vector<vgx_drawcmd> drawcmds(numCmds);
	std::vector<vgx_cache_slot> slots(ninst + 1);
	if (hipMemcpy(drawcmds.data(), as.drawcmds, numCmds * sizeof(vgx_drawcmd), hipMemcpyDeviceToHost) != hipSuccess
	 || hipMemcpy(slots.data(), devSlots, slots.size() * sizeof(vgx_cache_slot), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	printf("frame: %u instances of %llu meshes -> %llu meshes, %llu vertices in %u draw commands\n", ninst, (unsigned long long)sz.num_meshes,
		(unsigned long long)got.num_meshes, (unsigned long long)got.num_vertices, numCmds);

	vgx_raster_streams streams;
	memset(&streams, 0, sizeof(streams));
	streams.pos = out.pos; streams.color = out.color; streams.uv = as.uv; streams.idx = out.idx;
	streams.num_vertices = got.num_vertices; streams.num_indices = got.num_indices; streams.uv_bytes = 4;
	CHECK(vgx_command_bounds(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, 0, 0xFFFFFFFFu, devCmdBounds, devStatus, nullptr));

	// the white image every command samples (type 0, handle 0)
	uint32_t* devWhite = nullptr; vgx_raster_image* devImages = nullptr;
	const uint32_t whitePixels[4] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
	if (hipMalloc(&devWhite, sizeof(whitePixels)) != hipSuccess || hipMalloc(&devImages, sizeof(vgx_raster_image)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devWhite, whitePixels, sizeof(whitePixels), hipMemcpyHostToDevice);
	const vgx_raster_image white = { devWhite, 2, 2, 2, VGX_IMAGE_NEAREST };
	(void)hipMemcpy(devImages, &white, sizeof(white), hipMemcpyHostToDevice);

	uint32_t* devImage = nullptr; uint32_t* devFull = nullptr; uint32_t* devBits = nullptr;
	const size_t pixels = (size_t)width * height;
	(void)hipMalloc(&devImage, pixels * sizeof(uint32_t));
	(void)hipMalloc(&devFull, pixels * sizeof(uint32_t));
	const uint64_t words = vgx_damage_words(width, height);
	if (hipMalloc(&devBits, words * sizeof(uint32_t)) != hipSuccess) { return 1; }
	vgx_raster_target target;
	memset(&target, 0, sizeof(target));
	target.pixels = devImage; target.width = width; target.height = height; target.stride = width;
	target.scissor[2] = width; target.scissor[3] = height;
	target.flags = VGX_RASTER_CLEAR; target.clear_color = 0xFF201810u;
	if (!untilGrown([&] { return vgx_raster_commands(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, devImages, 1, nullptr, &target, devStatus, nullptr); },
	                devStatus, "render")) { return 1; }

	// ---- pick: the drawing under the cursor ----
	const vgx_pick_owners owners = { out.meshes, got.num_meshes };
	const uint32_t nq = 16; // a 4 x 4 lattice over the drawing in column 2, row 1: the rings leave gaps, the first point that hits decides
	vgx_pick_cmd_query q[nq];
	memset(q, 0, sizeof(q));
	for (uint32_t k = 0; k < nq; ++k) {
		q[k].x = 4.0f + pitch * 2.0f + 10.5f + 20.0f * (float)(k % 4); q[k].y = 2.0f + pitch * 1.0f + 10.5f + 20.0f * (float)(k / 4);
		q[k].cmd_end = 0xFFFFFFFFu;
	}
	vgx_pick_cmd_query* devQ = nullptr; vgx_pick_cmd_hit* devH = nullptr;
	if (hipMalloc(&devQ, sizeof(q)) != hipSuccess || hipMalloc(&devH, nq * sizeof(vgx_pick_cmd_hit)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devQ, q, sizeof(q), hipMemcpyHostToDevice);
	CHECK(vgx_pick_commands_boxed(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, devCmdBounds, &owners, devQ, nq, devH, devStatus, nullptr));
	vgx_pick_cmd_hit hits[nq];
	(void)hipMemcpy(hits, devH, sizeof(hits), hipMemcpyDeviceToHost);
	(void)hipMemcpy(&status, devStatus, sizeof(status), hipMemcpyDeviceToHost);
	uint32_t first = nq, hitCount = 0;
	for (uint32_t k = 0; k < nq; ++k) {
		if (hits[k].cmd != 0xFFFFFFFFu) { first = first == nq ? k : first; ++hitCount; }
	}
	if (status != VGX_OK || first == nq || hits[first].draw >= ninst) { fprintf(stderr, "pick: status %u, %u hits\n", status, hitCount); return 1; }
	const vgx_pick_cmd_hit hit = hits[first];
	const uint32_t dragged = hit.draw;
	printf("cursor (%.1f, %.1f), %u of %u points hit: command %u triangle %u mesh %u -> drawing %u\n", q[first].x, q[first].y, hitCount, nq, hit.cmd, hit.triangle,
		hit.mesh, dragged);

	// ---- the edit: that drawing dragged by a few pixels ----
	inst[dragged].mtx[4] += 13.0f; inst[dragged].mtx[5] += 7.0f;
	(void)hipMemcpy(devInst, inst.data(), ninst * sizeof(vgx_cache_instance), hipMemcpyHostToDevice);
	uint32_t* devDirty = nullptr;
	if (hipMalloc(&devDirty, sizeof(uint32_t)) != hipSuccess) { return 1; }
	(void)hipMemcpy(devDirty, &dragged, sizeof(dragged), hipMemcpyHostToDevice);
	// the commands that hold the drawing's meshes: a draw command holds the meshes [first_mesh, first_mesh + num_meshes), ascending over the table
	uint32_t cmdBegin = numCmds, cmdEnd = 0;
	for (uint32_t c = 0; c < numCmds; ++c) {
		if (drawcmds[c].first_mesh < slots[dragged + 1].first_mesh && drawcmds[c].first_mesh + drawcmds[c].num_meshes > slots[dragged].first_mesh) {
			cmdBegin = c < cmdBegin ? c : cmdBegin; cmdEnd = c + 1;
		}
	}
	vgx_update_frame uf;
	uf.pos = out.pos; uf.color = out.color; uf.num_vertices = got.num_vertices; uf.num_meshes = got.num_meshes; uf.mesh_bounds = devMeshBounds;
	vgx_raster_damage damage = { devBits, 0, 0 };
	(void)hipMemsetAsync(devBits, 0, words * sizeof(uint32_t), nullptr);
	CHECK(vgx_damage_instances(ctx, devMeshBounds, got.num_meshes, devSlots, ninst, devDirty, 1, nullptr, &target, devBits, devStatus + 1, nullptr));
	CHECK(vgx_cache_update(ctx, &cache, devInst, ninst, devSlots, devDirty, 1, nullptr, &uf, devStatus + 2, nullptr));
	CHECK(vgx_damage_instances(ctx, devMeshBounds, got.num_meshes, devSlots, ninst, devDirty, 1, nullptr, &target, devBits, devStatus + 3, nullptr));
	CHECK(vgx_command_bounds(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, cmdBegin, cmdEnd, devCmdBounds, devStatus + 4, nullptr));
	if (!untilGrown([&] { return vgx_raster_commands_damaged(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, devCmdBounds, devImages, 1, nullptr, &target, &damage,
	                                                        devStatus, nullptr); }, devStatus, "damaged")) { return 1; }
	uint32_t chain[5];
	(void)hipMemcpy(chain, devStatus, sizeof(chain), hipMemcpyDeviceToHost);
	if (chain[1] != VGX_OK || chain[2] != VGX_OK || chain[3] != VGX_OK || chain[4] != VGX_OK) {
		fprintf(stderr, "mark / update / mark / boxes: %u %u %u %u\n", chain[1], chain[2], chain[3], chain[4]);
		return 1;
	}

	// a full redraw of the edited frame, to compare with
	vgx_raster_target fullTarget = target;
	fullTarget.pixels = devFull;
	if (!untilGrown([&] { return vgx_raster_commands(ctx, &streams, devCmds, (uint32_t)capCmds, devNumCmds, devImages, 1, nullptr, &fullTarget, devStatus, nullptr); },
	                devStatus, "full")) { return 1; }
	std::vector<uint32_t> image(pixels), full(pixels), bits(words);
	(void)hipMemcpy(image.data(), devImage, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost);
	(void)hipMemcpy(full.data(), devFull, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost);
	if (hipMemcpy(bits.data(), devBits, words * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { return 1; }
	uint64_t differ = 0, marked = 0;
	for (size_t k = 0; k < pixels; ++k) { differ += image[k] != full[k]; }
	const uint32_t tiles = ((width + 15) / 16) * ((height + 15) / 16);
	for (uint32_t k = 0; k < tiles; ++k) { marked += (bits[k >> 5] >> (k & 31)) & 1u; }
	printf("damage: commands [%u, %u) of %u refreshed; %llu of %u tiles marked; %llu pixels differ from a full redraw\n", cmdBegin, cmdEnd, numCmds,
		(unsigned long long)marked, tiles, (unsigned long long)differ);

	FILE* f = fopen(ppm, "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", ppm); return 1; }
	fprintf(f, "P6\n%u %u\n255\n", width, height);
	for (size_t k = 0; k < pixels; ++k) {
		const uint8_t rgb[3] = { (uint8_t)(image[k] & 255u), (uint8_t)((image[k] >> 8) & 255u), (uint8_t)((image[k] >> 16) & 255u) };
		fwrite(rgb, 1, 3, f);
	}
	fclose(f);
	printf("wrote %s\n", ppm);

	vgx_pathset_destroy(ctx, ps);
	vgx_destroy(ctx);
	return differ == 0 && marked > 0 && marked < tiles && cmdBegin < cmdEnd && dragged == 8u ? 0 : 1;
}
