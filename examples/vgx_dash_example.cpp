// vgx_dash_example.cpp -- dashed strokes from plain C++: vgx_flatten -> vgx_subpath_draws -> vgx_dash -> vgx_stroke_count / vgx_stroke_emit.
// Nothing between the flatten and the stroker visits the host; the two counts (vgx_dash_count, vgx_stroke_count) are the only
// host round trips, and a steady-state caller that keeps its buffers skips the first.
//
//   hipcc -O2 -I include examples/vgx_dash_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,vg-renderer_amd -o vgx_dash_example
#include "vgx.h"
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#define CHECK(call)                                                                       \
	do {                                                                                  \
		const int st_ = (call);                                                           \
		if (st_ != VGX_OK) { fprintf(stderr, "%s -> %s\n", #call, vgx_status_string(st_)); return 1; } \
	} while (0)
#define HIP(call)                                                                         \
	do {                                                                                  \
		const hipError_t e_ = (call);                                                     \
		if (e_ != hipSuccess) { fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(e_)); return 1; } \
	} while (0)

template <class T> static T* upload(const std::vector<T>& v)
{
	T* d = nullptr;
	if (hipMalloc((void**)&d, v.size() * sizeof(T) + 16) != hipSuccess) { return nullptr; }
	if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { return nullptr; }
	return d;
}

int main()
{
	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));

	// two paths: a closed square and an open cubic
	const uint8_t cmdType[] = { VGX_CMD_MOVE_TO, VGX_CMD_LINE_TO, VGX_CMD_LINE_TO, VGX_CMD_LINE_TO, VGX_CMD_CLOSE, VGX_CMD_MOVE_TO, VGX_CMD_CUBIC_TO };
	const uint32_t argOff[] = { 0, 2, 4, 6, 8, 8, 10, 16 };
	const float args[] = { 0, 0, 10, 0, 10, 10, 0, 10, 20, 0, 30, 40, 50, -40, 60, 0 };
	const uint32_t pathBegin[] = { 0, 5, 7 };
	vgx_pathset_desc desc;
	desc.cmd_type = cmdType; desc.cmd_arg_off = argOff; desc.args = args; desc.path_cmd_begin = pathBegin; desc.npaths = 2; desc.ncmd = 7;
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));

	// three draws: the square dashed [4,2] with phase 1, the cubic dashed [3,1,1,1], the cubic again solid. Scale 2: user-space
	// lengths times vgx_draw::scale are the device units the pattern is in. Strokes only: fills come from the undashed lists.
	std::vector<vgx_draw> draws(3);
	memset(draws.data(), 0, draws.size() * sizeof(vgx_draw));
	const float scale = 2.0f;
	for (size_t i = 0; i < draws.size(); ++i) {
		vgx_draw& d = draws[i];
		d.path = i == 0 ? 0u : 1u;
		d.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0);
		d.stroke_color = 0xFF2080FFu; d.stroke_width = 1.5f * scale;
		d.scale = scale; d.tess_tol = 0.25f; d.fringe = 1.0f;
		d.mtx[0] = scale; d.mtx[3] = scale; d.mtx[5] = 10.0f * (float)i;
	}
	const float user[] = { 4, 2, 3, 1, 1, 1 };
	std::vector<float> pattern;
	for (float u : user) { pattern.push_back(u * scale); }
	std::vector<struct vgx_dash> dashes(3);
	memset(dashes.data(), 0, dashes.size() * sizeof(struct vgx_dash));
	dashes[0].first = 0; dashes[0].count = 2; dashes[0].phase = 1.0f * scale;
	dashes[1].first = 2; dashes[1].count = 4;
	CHECK(vgx_dash_validate(dashes.data(), dashes.size(), pattern.data(), pattern.size()));

	vgx_draw* dDraws = upload(draws);
	struct vgx_dash* dDashes = upload(dashes);
	float* dPattern = upload(pattern);
	if (!dDraws || !dDashes || !dPattern) { return 1; }

	// flatten (transformed), on the device
	vgx_sizes fs;
	CHECK(vgx_flatten_count(ctx, ps, dDraws, draws.size(), &fs, nullptr));
	vgx_flat_out flat;
	memset(&flat, 0, sizeof(flat));
	flat.cap_poly_vertices = fs.num_poly_vertices; flat.cap_subpaths = fs.num_subpaths;
	HIP(hipMalloc((void**)&flat.poly, (fs.num_poly_vertices + 1) * 2 * sizeof(float)));
	HIP(hipMalloc((void**)&flat.subpaths, (fs.num_subpaths + 1) * sizeof(vgx_subpath)));
	HIP(hipMalloc((void**)&flat.draw_info, draws.size() * sizeof(vgx_draw_info)));
	CHECK(vgx_flatten_emit(ctx, ps, dDraws, draws.size(), 1, &flat, nullptr));
	uint32_t* subDraw = nullptr;
	HIP(hipMalloc((void**)&subDraw, (fs.num_subpaths + 1) * sizeof(uint32_t)));
	CHECK(vgx_subpath_draws(ctx, flat.draw_info, draws.size(), subDraw, fs.num_subpaths, nullptr));

	// dash
	vgx_sizes ds;
	CHECK(vgx_dash_count(ctx, flat.poly, flat.subpaths, subDraw, fs.num_subpaths, dDashes, draws.size(), dPattern, pattern.size(), &ds, nullptr));
	vgx_dash_out pieces;
	memset(&pieces, 0, sizeof(pieces));
	pieces.cap_poly_vertices = ds.num_poly_vertices; pieces.cap_subpaths = ds.num_subpaths;
	HIP(hipMalloc((void**)&pieces.poly, (ds.num_poly_vertices + 1) * 2 * sizeof(float)));
	HIP(hipMalloc((void**)&pieces.subpaths, (ds.num_subpaths + 1) * sizeof(vgx_subpath)));
	HIP(hipMalloc((void**)&pieces.subpath_draw, (ds.num_subpaths + 1) * sizeof(uint32_t)));
	uint32_t* dStatus = nullptr;
	HIP(hipMalloc((void**)&dStatus, sizeof(uint32_t)));
	CHECK(vgx_dash(ctx, flat.poly, flat.subpaths, subDraw, fs.num_subpaths, dDashes, draws.size(), dPattern, pattern.size(), &pieces, nullptr, dStatus, nullptr));

	// stroke the pieces
	vgx_sizes ms;
	CHECK(vgx_stroke_count(ctx, pieces.poly, pieces.subpaths, pieces.subpath_draw, ds.num_subpaths, dDraws, draws.size(), &ms, nullptr));
	vgx_mesh_out mesh;
	memset(&mesh, 0, sizeof(mesh));
	mesh.cap_vertices = ms.num_vertices; mesh.cap_indices = ms.num_indices; mesh.cap_meshes = ms.num_meshes;
	HIP(hipMalloc((void**)&mesh.pos, (ms.num_vertices + 1) * 2 * sizeof(float)));
	HIP(hipMalloc((void**)&mesh.color, (ms.num_vertices + 1) * sizeof(uint32_t)));
	HIP(hipMalloc((void**)&mesh.idx, (ms.num_indices + 1) * sizeof(uint16_t)));
	HIP(hipMalloc((void**)&mesh.meshes, (ms.num_meshes + 1) * sizeof(vgx_mesh)));
	CHECK(vgx_stroke_emit(ctx, pieces.poly, pieces.subpaths, pieces.subpath_draw, ds.num_subpaths, dDraws, draws.size(), &mesh, nullptr));
	HIP(hipDeviceSynchronize());
	uint32_t status = 0;
	HIP(hipMemcpy(&status, dStatus, sizeof(status), hipMemcpyDeviceToHost));
	if (status != VGX_OK) { fprintf(stderr, "vgx_dash (device) -> %s\n", vgx_status_string((int)status)); return 1; }

	std::vector<vgx_subpath> subs(ds.num_subpaths);
	std::vector<uint32_t> pieceDraw(ds.num_subpaths);
	HIP(hipMemcpy(subs.data(), pieces.subpaths, subs.size() * sizeof(vgx_subpath), hipMemcpyDeviceToHost));
	HIP(hipMemcpy(pieceDraw.data(), pieces.subpath_draw, pieceDraw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	unsigned perDraw[3] = { 0, 0, 0 };
	for (uint32_t d : pieceDraw) { if (d < 3) { ++perDraw[d]; } }
	printf("%llu source lists -> %llu pieces (%u / %u / %u per draw), %llu vertices; %llu meshes, %llu mesh vertices, %llu indices\n",
	       (unsigned long long)fs.num_subpaths, (unsigned long long)ds.num_subpaths, perDraw[0], perDraw[1], perDraw[2], (unsigned long long)ds.num_poly_vertices,
	       (unsigned long long)ms.num_meshes, (unsigned long long)ms.num_vertices, (unsigned long long)ms.num_indices);
	// the square has a perimeter of 80 device units and a period of 12: seven pieces; the solid cubic stays one list
	const bool ok = perDraw[0] == 7 && perDraw[2] == 1 && ms.num_meshes == ds.num_subpaths;
	printf(ok ? "ok\n" : "UNEXPECTED\n");

	void* frees[] = { dDraws, dDashes, dPattern, flat.poly, flat.subpaths, flat.draw_info, subDraw, pieces.poly, pieces.subpaths, pieces.subpath_draw, dStatus,
	                  mesh.pos, mesh.color, mesh.idx, mesh.meshes };
	for (void* p : frees) { (void)hipFree(p); }
	CHECK(vgx_pathset_destroy(ctx, ps));
	CHECK(vgx_destroy(ctx));
	return ok ? 0 : 1;
}
