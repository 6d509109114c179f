// vgx_immediate_example.cpp -- immediate mode from C++: every frame is new content (other paths, other transforms, frame 4 twice the
// draws) and nothing is ever counted. Per frame: vgx_tessellate_immediate; the verdict in dev_status says what to do --
//   VGX_OK         the frame is in the buffers
//   VGX_E_NOSPACE  the output buffers are too small: grow them to dev_sizes (x1.5, as the reference's allocIndices / allocVertices grow
//                  theirs, src/vg.cpp:5321-5357) and call again
//   VGX_E_GROWN    the context's scratch was too small: call again (the context grows it first)
// A steady frame takes one call; the example checks each frame's totals against vgx_tessellate_count on a second context.
//   hipcc -O2 -I include examples/vgx_immediate_example.cpp -L vg-renderer_amd -lvgx -Wl,-rpath,$PWD/vg-renderer_amd -o vgx_immediate_example
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
#define HCHECK(call) do { if ((call) != hipSuccess) { fprintf(stderr, "%s failed\n", #call); return 1; } } while (0)

// The frame's drawing: `npaths` closed blobs of cubics whose shape moves with the frame (what an animated UI records anew every frame)
struct Paths
{
	std::vector<uint8_t> type;
	std::vector<uint32_t> off, begin;
	std::vector<float> args;
	void cmd(uint8_t t, std::initializer_list<float> a) { type.push_back(t); off.push_back((uint32_t)args.size()); args.insert(args.end(), a); }
};

static Paths makePaths(int frame, int npaths)
{
	Paths p;
	for (int i = 0; i < npaths; ++i) {
		p.begin.push_back((uint32_t)p.type.size());
		const float cx = 40.0f * (i % 16), cy = 40.0f * (i / 16), r = 12.0f + 4.0f * sinf(0.3f * frame + i);
		p.cmd(VGX_CMD_MOVE_TO, { cx + r, cy });
		const int k = 3 + (i + frame) % 4; // the number of lobes changes from frame to frame
		for (int j = 1; j <= k; ++j) {
			const float a0 = 6.2831853f * (j - 1) / k, a1 = 6.2831853f * j / k, am = 0.5f * (a0 + a1);
			p.cmd(VGX_CMD_CUBIC_TO, { cx + 1.6f * r * cosf(am - 0.4f), cy + 1.6f * r * sinf(am - 0.4f), cx + 1.6f * r * cosf(am + 0.4f),
			                          cy + 1.6f * r * sinf(am + 0.4f), cx + r * cosf(a1), cy + r * sinf(a1) });
		}
		p.cmd(VGX_CMD_CLOSE, {});
	}
	p.begin.push_back((uint32_t)p.type.size());
	p.off.push_back((uint32_t)p.args.size());
	return p;
}

static std::vector<vgx_draw> makeDraws(int frame, int npaths, int ndraws)
{
	std::vector<vgx_draw> d((size_t)ndraws);
	for (int i = 0; i < ndraws; ++i) {
		vgx_draw& w = d[(size_t)i];
		w.path = (uint32_t)(i % npaths);
		w.fill_flags = VGX_FILL_ENABLE | VGX_FILL_AA; w.fill_color = 0xFF2080F0u ^ (uint32_t)i;
		w.stroke_flags = VGX_STROKE_FLAGS(VGX_CAP_BUTT, VGX_JOIN_MITER, 1, 0); w.stroke_color = 0xFF000000u; w.stroke_width = 1.5f;
		w.scale = 1.0f + 0.5f * (i % 3); w.tess_tol = 0.25f; w.fringe = 1.0f;
		const float a = 0.02f * frame + 0.001f * i, s = w.scale; // every frame its own transforms
		w.mtx[0] = s * cosf(a); w.mtx[1] = s * sinf(a); w.mtx[2] = -s * sinf(a); w.mtx[3] = s * cosf(a);
		w.mtx[4] = 7.0f * frame + (float)(i / npaths) * 13.0f; w.mtx[5] = 3.0f * frame;
		w.state_key = 0;
	}
	return d;
}

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

int main(int argc, char** argv)
{
	const int frames = argc > 1 ? atoi(argv[1]) : 8;
	const int npaths = 64;
	vgx_ctx* ctx = nullptr;
	vgx_ctx* check = nullptr; // a second context: vgx_tessellate_count of the same frames, for comparison only
	CHECK(vgx_create(0, &ctx));
	CHECK(vgx_create(0, &check));
	hipStream_t s;
	HCHECK(hipStreamCreate(&s));
	vgx_sizes* dSizes; uint32_t* dStatus; vgx_draw* dDraws = nullptr; uint64_t capDraws = 0;
	HCHECK(hipMalloc(&dSizes, sizeof(vgx_sizes)));
	HCHECK(hipMalloc(&dStatus, sizeof(uint32_t)));
	Buffers buf;
	if (buf.alloc(4096, 4096, 256)) { return 1; }
	int maxCalls = 0, consistent = 1;
	for (int f = 0; f < frames; ++f) {
		const int ndraws = (f == 4 ? 2 : 1) * 3000; // frame 4: twice the batch
		Paths p = makePaths(f, npaths);
		vgx_pathset_desc desc = { p.type.data(), p.off.data(), p.args.data(), p.begin.data(), (uint32_t)npaths, (uint32_t)p.type.size() };
		vgx_pathset* ps = nullptr;
		CHECK(vgx_pathset_create(ctx, &desc, &ps));
		std::vector<vgx_draw> draws = makeDraws(f, npaths, ndraws);
		if ((uint64_t)ndraws > capDraws) {
			if (dDraws) { HCHECK(hipFree(dDraws)); }
			HCHECK(hipMalloc(&dDraws, draws.size() * sizeof(vgx_draw)));
			capDraws = (uint64_t)ndraws;
		}
		HCHECK(hipMemcpyAsync(dDraws, draws.data(), draws.size() * sizeof(vgx_draw), hipMemcpyHostToDevice, s));
		// the frame: immediate calls until VGX_OK
		uint32_t st = VGX_E_GROWN;
		vgx_sizes z = {};
		int calls = 0;
		char trail[64] = "";
		while (st != VGX_OK && calls < 3) {
			CHECK(vgx_tessellate_immediate(ctx, ps, dDraws, (uint64_t)ndraws, &buf.out, dSizes, dStatus, s));
			HCHECK(hipMemcpyAsync(&z, dSizes, sizeof(z), hipMemcpyDeviceToHost, s));
			HCHECK(hipMemcpyAsync(&st, dStatus, sizeof(st), hipMemcpyDeviceToHost, s));
			HCHECK(hipStreamSynchronize(s));
			snprintf(trail + strlen(trail), sizeof(trail) - strlen(trail), "%s%s", calls ? " -> " : "", st == VGX_OK ? "OK" : st == VGX_E_GROWN ? "GROWN" : st == VGX_E_NOSPACE ? "NOSPACE" : "?");
			++calls;
			if (st == VGX_E_NOSPACE) {
				if (buf.alloc(grow(buf.out.cap_vertices, z.num_vertices), grow(buf.out.cap_indices, z.num_indices), grow(buf.out.cap_meshes, z.num_meshes))) { return 1; }
			} else if (st != VGX_OK && st != VGX_E_GROWN) {
				fprintf(stderr, "frame %d: %s\n", f, vgx_status_string((int)st));
				return 1;
			}
		}
		if (st != VGX_OK) { fprintf(stderr, "frame %d: no VGX_OK within three calls\n", f); return 1; }
		if (calls > maxCalls) { maxCalls = calls; }
		// the same frame counted on the second context
		vgx_pathset* ps2 = nullptr;
		vgx_sizes c = {};
		CHECK(vgx_pathset_create(check, &desc, &ps2));
		CHECK(vgx_tessellate_count(check, ps2, dDraws, (uint64_t)ndraws, &c, s));
		CHECK(vgx_pathset_destroy(check, ps2));
		const bool same = c.num_vertices == z.num_vertices && c.num_indices == z.num_indices && c.num_meshes == z.num_meshes;
		consistent &= same ? 1 : 0;
		printf("frame %d: %d draws, %llu vertices, %llu indices, %llu meshes (%s)%s\n", f, ndraws, (unsigned long long)z.num_vertices,
		       (unsigned long long)z.num_indices, (unsigned long long)z.num_meshes, trail, same ? "" : " INCONSISTENT with the count");
		CHECK(vgx_pathset_destroy(ctx, ps));
	}
	printf("%d frames in immediate mode, at most %d calls per frame, totals %s\n", frames, maxCalls, consistent ? "consistent" : "INCONSISTENT");
	buf.release();
	(void)hipFree(dDraws); (void)hipFree(dSizes); (void)hipFree(dStatus);
	(void)hipStreamDestroy(s);
	vgx_destroy(check);
	vgx_destroy(ctx);
	return consistent ? 0 : 1;
}
