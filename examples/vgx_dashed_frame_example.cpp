// vgx_dashed_frame_example.cpp -- a frame of filled and dashed draws through ONE call from C++: vgx_tessellate_dashed takes the frame's
// vgx_draw records with one `struct vgx_dash` per draw and writes the frame's meshes in submission order -- per draw its fills, then
// either its solid strokes or one stroke mesh per dash. Nothing is counted and the host waits for nothing but the verdict:
//   VGX_OK         the frame is in the buffers
//   VGX_E_NOSPACE  the output buffers are too small: grow them to dev_sizes and call again
//   VGX_E_GROWN    the context's scratch (for the flatten stage, or for the pieces) was too small: call again, the context grows it first
// A first frame takes up to four calls, a steady one takes one; the example prints the trail of the first frame and of a second one, and
// checks that the second frame's meshes of the dashed draws are the pieces dev_dash_sizes counts.
//   hipcc -O2 -I include examples/vgx_dashed_frame_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_dashed_frame_example
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
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
#define HCHECK(call) do { if ((call) != hipSuccess) { fprintf(stderr, "%s failed\n", #call); return 1; } } while (0)

struct Paths
{
	std::vector<uint8_t> type;
	std::vector<uint32_t> off, begin;
	std::vector<float> args;
	void cmd(uint8_t t, std::initializer_list<float> a) { type.push_back(t); off.push_back((uint32_t)args.size()); args.insert(args.end(), a); }
};

struct Buffers
{
	vgx_mesh_out out = {};
	int alloc(uint64_t nv, uint64_t ni, uint64_t nm)
	{
		release();
		if (hipMalloc(&out.pos, (nv + 1) * 8) != hipSuccess || hipMalloc(&out.color, (nv + 1) * 4) != hipSuccess
			|| hipMalloc(&out.idx, (ni + 1) * 2) != hipSuccess || hipMalloc(&out.meshes, (nm + 1) * sizeof(vgx_mesh)) != hipSuccess) { return 1; }
		out.cap_vertices = nv; out.cap_indices = ni; out.cap_meshes = nm;
		return 0;
	}
	void release()
	{
		if (out.pos) { (void)hipFree(out.pos); (void)hipFree(out.color); (void)hipFree(out.idx); (void)hipFree(out.meshes); }
		out = vgx_mesh_out();
	}
};

static uint64_t grow(uint64_t cap, uint64_t need) { return need <= cap ? cap : (need > cap * 3 / 2 ? need : cap * 3 / 2); }

int main()
{
	const int npaths = 96;
	// the drawing: rounded blobs (closed cubics), every third one an open zigzag
	Paths p;
	for (int i = 0; i < npaths; ++i) {
		p.begin.push_back((uint32_t)p.type.size());
		const float cx = 60.0f * (i % 12) + 30.0f, cy = 60.0f * (i / 12) + 30.0f, r = 14.0f + (float)(i % 5);
		if (i % 3 == 2) {
			p.cmd(VGX_CMD_MOVE_TO, { cx - 24.0f, cy });
			for (int j = 1; j <= 8; ++j) { p.cmd(VGX_CMD_LINE_TO, { cx - 24.0f + 6.0f * j, cy + ((j & 1) ? 9.0f : -9.0f) }); }
		} else {
			p.cmd(VGX_CMD_MOVE_TO, { cx + r, cy });
			for (int j = 1; j <= 4; ++j) {
				const float a1 = 1.5707963f * j, am = a1 - 0.7853982f;
				p.cmd(VGX_CMD_CUBIC_TO, { cx + 1.5f * r * cosf(am - 0.35f), cy + 1.5f * r * sinf(am - 0.35f), cx + 1.5f * r * cosf(am + 0.35f),
				                          cy + 1.5f * r * sinf(am + 0.35f), cx + r * cosf(a1), cy + r * sinf(a1) });
			}
			p.cmd(VGX_CMD_CLOSE, {});
		}
	}
	p.begin.push_back((uint32_t)p.type.size());
	p.off.push_back((uint32_t)p.args.size());
	// the frame: every path filled (the zigzags not) and stroked; two draws out of three dashed, with two patterns in DEVICE units
	// (user-space lengths times vgx_draw::scale)
	const float userPattern[6] = { 6.0f, 3.0f, 10.0f, 2.0f, 1.0f, 2.0f };
	std::vector<vgx_draw> draws((size_t)npaths);
	std::vector<struct vgx_dash> dashes((size_t)npaths);
	std::vector<float> pattern;
	uint32_t numDashed = 0;
	for (int i = 0; i < npaths; ++i) {
		vgx_draw& w = draws[(size_t)i];
		memset(&w, 0, sizeof(w));
		w.path = (uint32_t)i;
		if (i % 3 != 2) { w.fill_flags = VGX_FILL_ENABLE | VGX_FILL_AA; w.fill_color = 0xFF2080F0u ^ (uint32_t)(i * 977); }
		w.stroke_flags = VGX_STROKE_FLAGS(i % 3 == 2 ? VGX_CAP_ROUND : VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0);
		w.stroke_color = 0xFF101010u; w.stroke_width = 2.0f;
		w.scale = 1.0f + 0.25f * (float)(i % 2); w.tess_tol = 0.25f; w.fringe = 1.0f;
		w.mtx[0] = w.scale; w.mtx[3] = w.scale; w.mtx[4] = 5.0f; w.mtx[5] = 5.0f;
		struct vgx_dash& d = dashes[(size_t)i];
		memset(&d, 0, sizeof(d));
		if (i % 3 != 0) { // dashed: [6,3] or [10,2,1,2] user units, the phase walks with the draw
			const int first = (i % 3 == 1) ? 0 : 2, count = (i % 3 == 1) ? 2 : 4;
			d.first = (uint32_t)pattern.size(); d.count = (uint32_t)count; d.phase = 0.5f * (float)i * w.scale;
			for (int k = 0; k < count; ++k) { pattern.push_back(userPattern[first + k] * w.scale); }
			++numDashed;
		}
	}
	if (vgx_dash_validate(dashes.data(), dashes.size(), pattern.data(), pattern.size()) != VGX_OK) { fprintf(stderr, "bad dash records\n"); return 1; }

	vgx_ctx* ctx = nullptr;
	CHECK(vgx_create(0, &ctx));
	hipStream_t s;
	HCHECK(hipStreamCreate(&s));
	vgx_pathset_desc desc = { p.type.data(), p.off.data(), p.args.data(), p.begin.data(), (uint32_t)npaths, (uint32_t)p.type.size() };
	vgx_pathset* ps = nullptr;
	CHECK(vgx_pathset_create(ctx, &desc, &ps));
	vgx_draw* dDraws; struct vgx_dash* dDashes; float* dPattern; vgx_sizes* dSizes; vgx_sizes* dDashSizes; uint32_t* dStatus;
	HCHECK(hipMalloc(&dDraws, draws.size() * sizeof(vgx_draw)));
	HCHECK(hipMalloc(&dDashes, dashes.size() * sizeof(struct vgx_dash)));
	HCHECK(hipMalloc(&dPattern, pattern.size() * sizeof(float)));
	HCHECK(hipMalloc(&dSizes, sizeof(vgx_sizes)));
	HCHECK(hipMalloc(&dDashSizes, sizeof(vgx_sizes)));
	HCHECK(hipMalloc(&dStatus, sizeof(uint32_t)));
	HCHECK(hipMemcpyAsync(dDraws, draws.data(), draws.size() * sizeof(vgx_draw), hipMemcpyHostToDevice, s));
	HCHECK(hipMemcpyAsync(dDashes, dashes.data(), dashes.size() * sizeof(struct vgx_dash), hipMemcpyHostToDevice, s));
	HCHECK(hipMemcpyAsync(dPattern, pattern.data(), pattern.size() * sizeof(float), hipMemcpyHostToDevice, s));
	Buffers buf;
	if (buf.alloc(4096, 4096, 256)) { return 1; }
	vgx_sizes z = {}, dz = {};
	int ok = 1;
	for (int frame = 0; frame < 2; ++frame) {
		uint32_t st = VGX_E_GROWN;
		int calls = 0;
		char trail[96] = "";
		while (st != VGX_OK && calls < 4) {
			CHECK(vgx_tessellate_dashed(ctx, ps, dDraws, (uint64_t)npaths, dDashes, dPattern, (uint64_t)pattern.size(), &buf.out, dSizes, dDashSizes, dStatus, s));
			HCHECK(hipMemcpyAsync(&z, dSizes, sizeof(z), hipMemcpyDeviceToHost, s));
			HCHECK(hipMemcpyAsync(&dz, dDashSizes, sizeof(dz), hipMemcpyDeviceToHost, s));
			HCHECK(hipMemcpyAsync(&st, dStatus, sizeof(st), hipMemcpyDeviceToHost, s));
			HCHECK(hipStreamSynchronize(s));
			snprintf(trail + strlen(trail), sizeof(trail) - strlen(trail), "%s%s", calls ? " -> " : "", st == VGX_OK ? "OK" : st == VGX_E_GROWN ? "GROWN" : st == VGX_E_NOSPACE ? "NOSPACE" : "?");
			++calls;
			if (st == VGX_E_NOSPACE) {
				if (buf.alloc(grow(buf.out.cap_vertices, z.num_vertices), grow(buf.out.cap_indices, z.num_indices), grow(buf.out.cap_meshes, z.num_meshes))) { return 1; }
			} else if (st != VGX_OK && st != VGX_E_GROWN) {
				fprintf(stderr, "frame %d: %s\n", frame, vgx_status_string((int)st));
				return 1;
			}
		}
		if (st != VGX_OK) { fprintf(stderr, "frame %d: no VGX_OK within four calls\n", frame); return 1; }
		printf("frame %d: %d draws (%u dashed), %llu meshes, %llu vertices, %llu indices; %llu dashes of %llu vertices (%s)\n", frame, npaths, numDashed,
		       (unsigned long long)z.num_meshes, (unsigned long long)z.num_vertices, (unsigned long long)z.num_indices, (unsigned long long)dz.num_subpaths,
		       (unsigned long long)dz.num_poly_vertices, trail);
		if (frame == 1 && calls != 1) { ok = 0; }
	}
	// the mesh table: the stroke meshes of the dashed draws are the pieces, in draw order
	std::vector<vgx_mesh> meshes((size_t)z.num_meshes);
	HCHECK(hipMemcpy(meshes.data(), buf.out.meshes, meshes.size() * sizeof(vgx_mesh), hipMemcpyDeviceToHost));
	uint64_t pieces = 0;
	for (size_t m = 0; m < meshes.size(); ++m) {
		if (m && meshes[m].draw < meshes[m - 1].draw) { ok = 0; }
		if ((meshes[m].subpath_kind >> 28) >= VGX_MESH_STROKE && dashes[meshes[m].draw].count != 0) { ++pieces; }
	}
	if (pieces != dz.num_subpaths) { ok = 0; }
	printf("%s\n", ok ? "the steady frame took one call; every dash is one stroke mesh at its draw's place" : "INCONSISTENT");
	buf.release();
	(void)hipFree(dDraws); (void)hipFree(dDashes); (void)hipFree(dPattern); (void)hipFree(dSizes); (void)hipFree(dDashSizes); (void)hipFree(dStatus);
	CHECK(vgx_pathset_destroy(ctx, ps));
	(void)hipStreamDestroy(s);
	vgx_destroy(ctx);
	return ok ? 0 : 1;
}
