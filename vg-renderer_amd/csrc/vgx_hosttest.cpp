// vgx_hosttest.cpp -- CPU build of the lane-level product code (vgx_lane.h, vgx_pathsim.h) for unit tests.
// This is NOT a fallback path: nothing in the package loads it; tests/test_host_lane_logic.py uses it to
// check the per-lane builder logic against the oracle without a GPU.
#include "vgx_pathsim.h"
#include "vgx_inst.h"
#include "vgx_pathset_host.h"
#include "vgx_thin.h"
#include <string.h>

namespace {
struct HostStack
{
	float s[VGX_CUBIC_MAX_PENDING][6];
	void push(int level, float ax, float ay, float bx, float by, float cx, float cy)
	{
		float* p = s[level];
		p[0] = ax; p[1] = ay; p[2] = bx; p[3] = by; p[4] = cx; p[5] = cy;
	}
	void pop(int level, float& ax, float& ay, float& bx, float& by, float& cx, float& cy)
	{
		const float* p = s[level];
		ax = p[0]; ay = p[1]; bx = p[2]; by = p[3]; cx = p[4]; cy = p[5];
	}
};
}

extern "C" {

// Runs the exact serial builder (the device's slow path) for ONE draw on the host.
// counts[4] = { num_poly_vertices, num_subpaths, num_fill_meshes, num_stroke_meshes }
int vgxt_serial_flatten(const vgx_pathset_desc* d, const vgx_draw* draw, int applyTransform, float* poly, vgx_subpath* subs, uint32_t* counts)
{
	VgxPathSetDev ps;
	memset(&ps, 0, sizeof(ps));
	ps.cmd_type = d->cmd_type; ps.cmd_arg_off = d->cmd_arg_off; ps.args = d->args; ps.path_cmd_begin = d->path_cmd_begin;
	ps.npaths = d->npaths; ps.ncmd = d->ncmd;
	HostStack st;
	const uint32_t c0 = d->path_cmd_begin[draw->path], c1 = d->path_cmd_begin[draw->path + 1];
	uint32_t limit = 0;
	if (poly) { // the emit pass knows the final vertex count from the count pass
		uint32_t tmp[4];
		vgxt_serial_flatten(d, draw, 0, nullptr, nullptr, tmp);
		limit = tmp[0];
	}
	if (poly && applyTransform) {
		PathSim<true, true> sim;
		sim.scale = draw->scale; sim.tol = draw->tess_tol; sim.mtx = draw->mtx; sim.poly = poly; sim.polyBase = 0;
		sim.subs = subs; sim.subBase = 0; sim.mdesc = nullptr; sim.mprep = nullptr; sim.mtab = nullptr; sim.draw = nullptr; sim.limit = limit; sim.meshBase = 0; sim.drawIndex = 0;
		sim.fillFlags = draw->fill_flags; sim.strokeFlags = draw->stroke_flags; sim.numFillTotal = 0;
		sim.init();
		sim.run(ps, c0, c1, st);
		counts[0] = sim.nverts; counts[1] = sim.nsubs; counts[2] = sim.nfill; counts[3] = sim.nstroke;
	} else if (poly) {
		PathSim<true, false> sim;
		sim.scale = draw->scale; sim.tol = draw->tess_tol; sim.mtx = draw->mtx; sim.poly = poly; sim.polyBase = 0;
		sim.subs = subs; sim.subBase = 0; sim.mdesc = nullptr; sim.mprep = nullptr; sim.mtab = nullptr; sim.draw = nullptr; sim.limit = limit; sim.meshBase = 0; sim.drawIndex = 0;
		sim.fillFlags = draw->fill_flags; sim.strokeFlags = draw->stroke_flags; sim.numFillTotal = 0;
		sim.init();
		sim.run(ps, c0, c1, st);
		counts[0] = sim.nverts; counts[1] = sim.nsubs; counts[2] = sim.nfill; counts[3] = sim.nstroke;
	} else {
		PathSim<false, false> sim;
		sim.scale = draw->scale; sim.tol = draw->tess_tol; sim.mtx = nullptr; sim.poly = nullptr; sim.polyBase = 0;
		sim.subs = nullptr; sim.subBase = 0; sim.mdesc = nullptr; sim.mprep = nullptr; sim.mtab = nullptr; sim.draw = nullptr; sim.limit = limit; sim.meshBase = 0; sim.drawIndex = 0;
		sim.fillFlags = draw->fill_flags; sim.strokeFlags = draw->stroke_flags; sim.numFillTotal = 0;
		sim.init();
		sim.run(ps, c0, c1, st);
		counts[0] = sim.nverts; counts[1] = sim.nsubs; counts[2] = sim.nfill; counts[3] = sim.nstroke;
	}
	return 0;
}

// One lane of the instanced flatten kernel (InstCore, vgx_inst.h) for ONE draw on the host: the command loop of
// k_flatten_inst with the generic cubic walk, a bump allocator over `heap` (cap vertices, lane blocks of `lb` vertices) in
// place of the wave-aggregated one. `cursor` carries the heap position from draw to draw (lane-private blocks persist in
// the kernel; here every call starts a fresh block). sub_rec[k] is written at the sub-path-ending commands (k relative to
// the path's first command); counts[5] = { poly vertices, sub-paths, fill meshes, stroke meshes, 1 if the heap ran out }.
namespace {
struct HostInstEnv
{
	float* poly; uint64_t cap; uint32_t lb; uint64_t* cursor; bool failed;
	bool alloc(uint64_t want, uint64_t* base)
	{
		if (*cursor + want > cap) { failed = true; return false; }
		*base = *cursor; *cursor += want;
		return true;
	}
	void emit(float* wp, float x, float y) { wp[0] = x; wp[1] = y; }
	void flushForMove(float*) {}
};
}
int vgxt_inst_flatten(const vgx_pathset_desc* d, const vgx_draw* draw, float* heap, uint64_t cap, uint32_t lb, uint64_t* cursor, VgxSubRec* sub_rec, uint32_t* counts)
{
	HostStack st;
	InstCore<HostInstEnv> L;
	L.env.poly = heap; L.env.cap = cap; L.env.lb = lb; L.env.cursor = cursor; L.env.failed = false;
	L.initLane();
	L.beginDraw(draw->mtx, draw->scale, draw->tess_tol, draw->fill_flags, draw->stroke_flags);
	const uint32_t c0 = d->path_cmd_begin[draw->path], c1 = d->path_cmd_begin[draw->path + 1];
	for (uint32_t c = c0; c < c1; ++c) {
		const float* a = d->args + d->cmd_arg_off[c];
		const uint32_t na = d->cmd_arg_off[c + 1] - d->cmd_arg_off[c];
		const uint32_t type = d->cmd_type[c];
		switch (type) {
		case VGX_CMD_MOVE_TO: L.moveTo(a[0], a[1]); break;
		case VGX_CMD_LINE_TO: L.lineTo(a[0], a[1]); break;
		case VGX_CMD_CUBIC_TO: L.cubicTo(a[0], a[1], a[2], a[3], a[4], a[5], st); break;
		case VGX_CMD_QUAD_TO: L.quadTo(a[0], a[1], a[2], a[3], st); break;
		case VGX_CMD_CLOSE: L.close(); break;
		case VGX_CMD_POLYLINE: L.polyline(a, na >> 1); break;
		default: return -1; // statically serial paths never reach the instanced lane
		}
		const bool lastInSub = (c + 1 == c1) || d->cmd_type[c + 1] == VGX_CMD_MOVE_TO;
		if (lastInSub) { L.endSub(sub_rec + (c - c0)); }
	}
	const vgx_draw_info di = L.drawInfo();
	counts[0] = di.num_poly_vertices; counts[1] = di.num_subpaths; counts[2] = di.flags >> 1; counts[3] = di.num_meshes - (di.flags >> 1);
	counts[4] = L.env.failed ? 1u : 0u;
	return 0;
}

// closed-form mesh sizes (vgx_lane.h) for one mesh of a draw; returns 1 when the size is closed-form
int vgxt_mesh_closed_form(const vgx_draw* dr, uint32_t kind, int closed, uint32_t n, uint32_t* nv, uint32_t* ni)
{
	if (kind >= VGX_MESH_STROKE) {
		const VgxStrokeParams sp = vgx_stroke_params(kind, closed != 0, dr->stroke_flags, dr->stroke_width, dr->fringe, dr->scale, dr->tess_tol);
		const uint32_t H = vgx_half_circle_points(vgx_step_angle(dr->scale, sp.hsw, dr->tess_tol));
		return vgx_mesh_closed_form(kind, closed != 0, sp.cap, sp.join, n, H, nv, ni) ? 1 : 0;
	}
	return vgx_mesh_closed_form(kind, closed != 0, 0, 0, n, 2, nv, ni) ? 1 : 0;
}

// the pinned transcendentals (csrc/vgmath.h), for tests that restate arithmetic in numpy
float vgxt_cos(float a) { return vgm_cos(a); }
float vgxt_sin(float a) { return vgm_sin(a); }
// vectors of them (tests/test_oracle_libm.py: ULP distance of every pinned transcendental from glibc's):
// fn 0 cos, 1 sin, 2 tan, 3 acos, 4 atan2(a, b), 5 rsqrt
void vgxt_math_vec(int fn, const float* a, const float* b, float* out, uint64_t n)
{
	for (uint64_t i = 0; i < n; ++i) {
		switch (fn) {
		case 0: out[i] = vgm_cos(a[i]); break;
		case 1: out[i] = vgm_sin(a[i]); break;
		case 2: out[i] = vgm_tan(a[i]); break;
		case 3: out[i] = vgm_acos(a[i]); break;
		case 4: out[i] = vgm_atan2(a[i], b[i]); break;
		default: out[i] = vgm_rsqrt(a[i]); break;
		}
	}
}

} // extern "C"

extern "C" {

// Path sets of MOVE_TO / LINE_TO / CLOSE paths (vgx_thin.h): the static layout tables as vgx_pathset_create builds them, then
// k_flatten_thin's lane function over every command instance of the batch, one after the other. Outputs as the kernel leaves
// them: poly [command instances][2] (vertex v of draw d at cmd_prefix[d] + v), sub_rec [static sub-paths of the batch] (record j of
// draw d at sub_prefix[d] + j), dinfo [ndraws], serial [ndraws] (1: the draw is listed for the exact builder).
// Returns 1, 0 when the set is not eligible, < 0 = -(validation error).
int vgxt_thin_flatten(const vgx_pathset_desc* d, const vgx_draw* draws, uint64_t ndraws, float* poly, VgxSubRec* subRec, vgx_draw_info* dinfo, uint8_t* serial)
{
	std::vector<uint8_t> cmdFlags, pathFlags;
	std::vector<uint32_t> spStart;
	uint32_t maxCmds = 0;
	const int st = vgx_pathset_validate_host(d, &cmdFlags, &spStart, &pathFlags, &maxCmds);
	if (st != VGX_OK) { return -st; }
	std::vector<uint32_t> pathSubBegin(d->npaths + 1, 0);
	uint32_t nsub = 0;
	for (uint32_t p = 0; p < d->npaths; ++p) {
		pathSubBegin[p] = nsub;
		for (uint32_t c = d->path_cmd_begin[p]; c < d->path_cmd_begin[p + 1]; ++c) { if (cmdFlags[c] & VGX_CF_LAST_IN_SUB) { ++nsub; } }
	}
	pathSubBegin[d->npaths] = nsub;
	std::vector<VgxCmdThin> thv(d->ncmd + 3);
	VgxCmdThin* th = thv.data() + 1;
	std::vector<VgxThinPath> tp(d->npaths + 1);
	std::vector<VgxThinSub> ts(nsub + 1);
	vgx_thin_fill(d, cmdFlags.data(), spStart.data(), pathFlags.data(), th);
	if (d->npaths == 0 || d->ncmd == 0 || !vgx_thin_build(d->npaths, d->path_cmd_begin, pathFlags.data(), pathSubBegin.data(), th, tp.data(), ts.data())) { return 0; }
	uint64_t cmdPrefix = 0, subPrefix = 0;
	for (uint64_t i = 0; i < ndraws; ++i) {
		const vgx_draw* dr = draws + i;
		const VgxThinPath q = tp[dr->path];
		const uint32_t ncmd = d->path_cmd_begin[dr->path + 1] - d->path_cmd_begin[dr->path];
		serial[i] = 0;
		for (uint32_t k = 0; k < ncmd; ++k) {
			if (vgx_thin_lane(q, th[q.pc0 + k], ts.data(), dr->mtx, dr->fill_flags, dr->stroke_flags, cmdPrefix, &subPrefix, poly, subRec, dinfo + i)) { serial[i] = 1; }
		}
		cmdPrefix += ncmd;
		subPrefix += pathSubBegin[dr->path + 1] - pathSubBegin[dr->path];
	}
	return 1;
}

}

extern "C" {

// The derived tables of a path set as the host loops build them (vgx_pathset_host.h, vgx_thin.h): the oracle of the device-side
// build of vgx_pathset_create (vgx_pathset.hip). `which` = VGX_PS_TABLE_* (include/vgx.h). Returns the table's size in bytes
// (dst may be NULL to ask), < 0 = -(validation status).
int64_t vgxt_pathset_table(const vgx_pathset_desc* d, int which, void* dst, uint64_t cap)
{
	std::vector<uint8_t> cmdFlags, pathFlags;
	std::vector<uint32_t> spStart, pathSubBegin, subLastCmd;
	uint32_t maxCmds = 0;
	const int st = vgx_pathset_validate_host(d, &cmdFlags, &spStart, &pathFlags, &maxCmds);
	if (st != VGX_OK) { return -(int64_t)st; }
	vgx_pathset_subs_host(d, cmdFlags.data(), &pathSubBegin, &subLastCmd);
	std::vector<VgxCmdThin> thv(d->ncmd + 3);
	memset(thv.data(), 0, thv.size() * sizeof(VgxCmdThin));
	VgxCmdThin* th = thv.data() + 1;
	std::vector<VgxThinPath> tp(d->npaths + 1);
	std::vector<VgxThinSub> ts(subLastCmd.size() + 1);
	vgx_thin_fill(d, cmdFlags.data(), spStart.data(), pathFlags.data(), th);
	const bool thinStatic = d->npaths != 0 && d->ncmd != 0 && vgx_thin_build(d->npaths, d->path_cmd_begin, pathFlags.data(), pathSubBegin.data(), th, tp.data(), ts.data());
	bool hasSerial = false, hasEmpty = false;
	for (uint32_t i = 0; i < d->npaths; ++i) {
		if (pathFlags[i] & VGX_PF_SERIAL) { hasSerial = true; }
		if (d->path_cmd_begin[i + 1] == d->path_cmd_begin[i]) { hasEmpty = true; }
	}
	std::vector<VgxCmdRec> rec;
	const void* src = nullptr; uint64_t n = 0;
	uint32_t scal[8] = { maxCmds, hasSerial ? 1u : 0u, hasEmpty ? 1u : 0u, thinStatic ? 1u : 0u, (uint32_t)subLastCmd.size(), d->npaths, d->ncmd, 0u };
	switch (which) {
	case VGX_PS_TABLE_CMD_FLAGS: src = cmdFlags.data(); n = d->ncmd; break;
	case VGX_PS_TABLE_SP_START: src = spStart.data(); n = (uint64_t)d->ncmd * 4; break;
	case VGX_PS_TABLE_PATH_FLAGS: src = pathFlags.data(); n = d->npaths; break;
	case VGX_PS_TABLE_CMDREC:
		rec.resize(d->ncmd + 1);
		vgx_pathset_records_host(d, cmdFlags.data(), spStart.data(), rec.data());
		src = rec.data(); n = (uint64_t)d->ncmd * sizeof(VgxCmdRec); break;
	case VGX_PS_TABLE_PATH_SUB_BEGIN: src = pathSubBegin.data(); n = ((uint64_t)d->npaths + 1) * 4; break;
	case VGX_PS_TABLE_SUB_LAST_CMD: src = subLastCmd.data(); n = (uint64_t)subLastCmd.size() * 4; break;
	case VGX_PS_TABLE_CMDTHIN: src = th; n = (uint64_t)d->ncmd * sizeof(VgxCmdThin); break;
	case VGX_PS_TABLE_THIN_PATH: src = tp.data(); n = thinStatic ? (uint64_t)d->npaths * sizeof(VgxThinPath) : 0; break;
	case VGX_PS_TABLE_THIN_SUB: src = ts.data(); n = thinStatic ? (uint64_t)subLastCmd.size() * sizeof(VgxThinSub) : 0; break;
	case VGX_PS_TABLE_SCALARS: src = scal; n = sizeof(scal); break;
	default: return -(int64_t)VGX_E_INVALID_ARG;
	}
	if (dst) {
		if (cap < n) { return -(int64_t)VGX_E_NOSPACE; }
		if (n) { memcpy(dst, src, n); }
	}
	return (int64_t)n;
}

}

#include "vgx_text.h"

extern "C" {

// the matrix vgx_text_quads hands to the per-quad transform for one run (vgx_text.h); returns 1 when it is finite
int vgxt_text_run_matrix(const vgx_text_run* run, float* m) { return vgx_text_run_matrix(*run, m) ? 1 : 0; }

// vgx_text_quads on the host: the functions of vgx_text.h (the ones the kernel of vgx_text.hip runs one quad per lane) run after run,
// quad after quad, with the call's contract -- places and capacities as given, nothing written for a run that is too large, not
// finite or out of place, one mesh record per run, the totals in `sizes` (may be NULL). Returns the status the device call leaves in
// dev_status (the first failing run's; the device reports one of the failing runs').
int vgxt_text_quads(const float* quads, uint64_t nquads, const vgx_text_run* runs, uint64_t nruns, uint64_t first_mesh,
                    const vgx_mesh_out* out, void* out_uv, uint32_t uv_bytes, vgx_sizes* sizes)
{
	int status = VGX_OK;
	uint64_t endV = 0, endI = 0, total = 0;
	for (uint64_t r = 0; r < nruns; ++r) {
		const vgx_text_run& run = runs[r];
		float m[6];
		int st = vgx_text_run_status(run, m);
		bool ordered = run.first_quad <= nquads && run.num_quads <= nquads - run.first_quad;
		if (r > 0) { ordered = ordered && runs[r - 1].first_quad <= run.first_quad && runs[r - 1].num_quads <= run.first_quad - runs[r - 1].first_quad; }
		if (st == VGX_OK && !ordered) { st = VGX_E_INVALID_ARG; }
		bool write = false;
		if (st == VGX_OK) {
			const uint64_t ev = run.first_vertex + 4ull * run.num_quads, ei = run.first_index + 6ull * run.num_quads;
			if (ev > endV) { endV = ev; }
			if (ei > endI) { endI = ei; }
			total += run.num_quads;
			write = vgx_text_run_fits(run, out->cap_vertices, out->cap_indices);
			if (!write) { st = VGX_E_NOSPACE; }
		}
		if (out->meshes) {
			if (first_mesh + r < out->cap_meshes) { out->meshes[first_mesh + r] = vgx_text_run_mesh(run, st == VGX_OK); }
			else if (st == VGX_OK) { st = VGX_E_NOSPACE; }
		}
		if (status == VGX_OK) { status = st; }
		if (!write) { continue; }
		for (uint32_t k = 0; k < run.num_quads; ++k) {
			const float* q = quads + 8 * (run.first_quad + k);
			const uint64_t v = run.first_vertex + 4ull * k;
			vgx_text_quad_pos(q, m, out->pos + 2 * v);
			for (int c = 0; c < 4; ++c) { out->color[v + c] = run.color; }
			if (out_uv && uv_bytes == 4) { vgx_text_quad_uv16(q, (uint32_t*)out_uv + v); }
			else if (out_uv && uv_bytes == 8) { vgx_text_quad_uvf(q, (float*)out_uv + 2 * v); }
			vgx_text_quad_idx(k, out->idx + run.first_index + 6ull * k);
		}
	}
	if (sizes) {
		memset(sizes, 0, sizeof(*sizes));
		sizes->num_meshes = first_mesh + nruns; sizes->num_vertices = endV; sizes->num_indices = endI; sizes->num_elements = total;
	}
	return status;
}

}

#include "vgx_dash.h"
#include <vector>

extern "C" {

// the closed-form interval range of one record on a list of length T fixed units (vgx_dash_intervals); ~0 for an invalid record
uint64_t vgxt_dash_intervals(const struct vgx_dash* d, const float* pattern, uint64_t npattern, uint64_t T, uint64_t* jlo)
{
	VgxDashPat p;
	if (!vgx_dash_pat_build(*d, pattern, npattern, &p)) { return ~0ull; }
	return vgx_dash_intervals(p, T, jlo);
}

// vgx_dash on the host: the functions of vgx_dash.h (the ones the kernels of vgx_dash.hip run one lane per segment / "on" interval /
// output vertex) list after list, interval after interval, vertex after vertex, with the call's contract: nothing written unless
// everything is valid, in range and fits; the totals in `sizes` (may be NULL; exact for VGX_OK and VGX_E_NOSPACE). Returns the status
// the device call leaves in dev_status. `out` may be NULL (the count alone).
int vgxt_dash(const float* poly, const vgx_subpath* subs, const uint32_t* sub_draw, uint64_t nsubs, const struct vgx_dash* dashes, uint64_t ndraws,
              const float* pattern, uint64_t npattern, const vgx_dash_out* out, vgx_sizes* sizes)
{
	if (sizes) { memset(sizes, 0, sizeof(*sizes)); }
	std::vector<VgxDashPat> pat(ndraws ? ndraws : 1);
	bool valid = true;
	for (uint64_t k = 0; k < npattern; ++k) { valid = valid && vgx_dash_entry_ok(pattern[k]); }
	for (uint64_t d = 0; d < ndraws; ++d) { valid = vgx_dash_pat_build(dashes[d], pattern, npattern, &pat[d]) && valid; }
	for (uint64_t l = 0; l < nsubs; ++l) { valid = valid && sub_draw[l] < ndraws; }
	if (!valid) { return VGX_E_INVALID_ARG; }
	// the prefix sums of every dashed list, back to back
	std::vector<uint64_t> G(1, 0), base(nsubs + 1, 0);
	for (uint64_t l = 0; l < nsubs; ++l) {
		base[l] = G.size() - 1;
		if (subs[l].num_vertices > 0x7FFFFFFFu) { return VGX_E_RANGE; }
		if (pat[sub_draw[l]].count == 0) { continue; }
		const uint32_t n = subs[l].num_vertices, m = vgx_dash_num_segments(n, subs[l].flags);
		const float* v = poly + 2 * subs[l].first_vertex;
		uint64_t hi = 0;
		for (uint32_t i = 0; i < m; ++i) {
			const uint32_t i1 = i + 1u == n ? 0u : i + 1u;
			uint64_t q;
			if (!vgx_dash_seg_q(v[2 * i], v[2 * i + 1], v[2 * i1], v[2 * i1 + 1], &q)) { return VGX_E_RANGE; }
			hi += q >> 31;
			G.push_back(G.back() + q);
		}
		if (hi > (1ull << 31) || G.back() - G[base[l]] > VGX_DASH_MAX_T) { return VGX_E_RANGE; }
	}
	base[nsubs] = G.size() - 1;
	// the call's "on" intervals (the scan OpDashCand), before any of them is walked
	{
		uint64_t nint = 0;
		for (uint64_t l = 0; l < nsubs; ++l) {
			const VgxDashPat& P = pat[sub_draw[l]];
			uint64_t nc = 1, jlo;
			if (P.count != 0) {
				const uint32_t m = vgx_dash_num_segments(subs[l].num_vertices, subs[l].flags);
				nc = m ? vgx_dash_intervals(P, G[base[l] + m] - G[base[l]], &jlo) : 0;
			}
			if (nc > VGX_DASH_MAX_INTERVALS || (nint += nc) > VGX_DASH_MAX_INTERVALS) { return VGX_E_RANGE; }
		}
	}
	// pass 0 counts (what k_dash_count does), pass 1 writes (k_dash_emit)
	for (int pass = 0; pass < 2; ++pass) {
		uint64_t np = 0, nv = 0;
		for (uint64_t l = 0; l < nsubs; ++l) {
			const VgxDashPat& P = pat[sub_draw[l]];
			const uint32_t n = subs[l].num_vertices;
			const float* v = poly + 2 * subs[l].first_vertex;
			if (P.count == 0) { // verbatim
				if (pass) {
					vgx_subpath rec; rec.first_vertex = nv; rec.num_vertices = n; rec.flags = subs[l].flags;
					out->subpaths[np] = rec; out->subpath_draw[np] = sub_draw[l];
					if (out->subpath_src) { out->subpath_src[np] = (uint32_t)l; }
					for (uint32_t k = 0; k < 2 * n; ++k) { out->poly[2 * nv + k] = v[k]; }
				}
				++np; nv += n;
				continue;
			}
			VgxDashList L;
			L.v = v; L.G = G.data() + base[l]; L.n = n; L.m = vgx_dash_num_segments(n, subs[l].flags);
			if (L.m == 0) { continue; }
			L.T = L.G[L.m] - L.G[0];
			uint64_t jlo;
			const uint64_t nc = vgx_dash_intervals(P, L.T, &jlo);
			for (uint64_t c = 0; c < nc; ++c) {
				VgxDashPiece p;
				if (!vgx_dash_piece(L, P, jlo + c, &p)) { continue; }
				const uint32_t k = vgx_dash_piece_vertices(p);
				if (pass) {
					vgx_subpath rec; rec.first_vertex = nv; rec.num_vertices = k; rec.flags = 0;
					out->subpaths[np] = rec; out->subpath_draw[np] = sub_draw[l];
					if (out->subpath_src) { out->subpath_src[np] = (uint32_t)l; }
					for (uint32_t i = 0; i < k; ++i) { const V2 x = vgx_dash_piece_vertex(L, p, i); out->poly[2 * (nv + i)] = x.x; out->poly[2 * (nv + i) + 1] = x.y; }
				}
				++np; nv += k;
			}
		}
		if (!pass) {
			if (sizes) { sizes->num_subpaths = np; sizes->num_poly_vertices = nv; }
			if (!out) { return VGX_OK; }
			if (np > out->cap_subpaths || nv > out->cap_poly_vertices) { return VGX_E_NOSPACE; }
		}
	}
	return VGX_OK;
}

}

#include "vgx_dashframe.h"

extern "C" {

// The slots of a frame with dashed strokes (vgx_dashframe.h), as k_dashframe_place finds them: dashed[m] != 0 marks the source meshes the
// dash pass cut, piece_src[p] the source mesh of every piece (non-decreasing). slot_kept[m] = the frame slot of source mesh m (~0 for a
// dashed one), slot_piece[p] = the slot of piece p. Returns the number of meshes of the frame.
uint64_t vgxt_dashframe_ranks(const uint8_t* dashed, uint64_t nsource, const uint32_t* piece_src, uint64_t npieces, uint64_t* slot_kept, uint64_t* slot_piece)
{
	std::vector<uint64_t> before(nsource + 1, 0); // D(m): the scan OpDashFrameLists
	for (uint64_t m = 0; m < nsource; ++m) { before[m + 1] = before[m] + (dashed[m] ? 1u : 0u); }
	for (uint64_t m = 0; m < nsource; ++m) {
		slot_kept[m] = dashed[m] ? ~0ull : vgx_df_slot_kept(m, before[m], before[m] ? vgx_df_pieces_before(piece_src, npieces, m) : 0ull);
	}
	for (uint64_t p = 0; p < npieces; ++p) { slot_piece[p] = vgx_df_slot_piece(piece_src[p], before[piece_src[p]], p); }
	return vgx_df_num_meshes(nsource, before[nsource], npieces);
}

}

#include "vgx_bounds.h"

extern "C" {

// vgx_mesh_bounds on the host: the order-preserving images of vgx_bounds.h (the ones the kernel of vgx_bounds.hip reduces and combines)
// vertex after vertex, decoded at the end as the call's last kernel does.
void vgxt_mesh_bounds(const float* pos, const vgx_mesh* meshes, uint64_t num_meshes, float* bounds)
{
	for (uint64_t m = 0; m < num_meshes; ++m) {
		uint32_t lox = VGX_ORD_POS_INF, loy = VGX_ORD_POS_INF, hix = VGX_ORD_NEG_INF, hiy = VGX_ORD_NEG_INF;
		const float* p = pos + 2 * meshes[m].first_vertex;
		for (uint32_t v = 0; v < meshes[m].num_vertices; ++v) {
			const uint32_t x = vgx_ord_from_float(p[2 * v]), y = vgx_ord_from_float(p[2 * v + 1]);
			if (x < lox) { lox = x; }
			if (y < loy) { loy = y; }
			if (x > hix) { hix = x; }
			if (y > hiy) { hiy = y; }
		}
		bounds[4 * m] = vgx_float_from_ord(lox); bounds[4 * m + 1] = vgx_float_from_ord(loy);
		bounds[4 * m + 2] = vgx_float_from_ord(hix); bounds[4 * m + 3] = vgx_float_from_ord(hiy);
	}
}

uint32_t vgxt_ord_from_float(float f) { return vgx_ord_from_float(f); }
float vgxt_float_from_ord(uint32_t o) { return vgx_float_from_ord(o); }

// vgx_cache_cull on the host: the functions of vgx_bounds.h instance after instance, with the call's contract (out->inst may be `inst`;
// bounds / kept / num_kept may be NULL). Returns the status the device call leaves in dev_status.
int vgxt_cache_cull(uint64_t cache_meshes, const float* mesh_bounds, const vgx_cache_instance* inst, uint64_t ninst,
                    const float* views, uint32_t nviews, const uint32_t* inst_view, const vgx_cull_out* out)
{
	int status = VGX_OK;
	uint64_t nk = 0;
	for (uint64_t i = 0; i < ninst; ++i) {
		vgx_cache_instance in = inst[i];
		const uint32_t view = inst_view ? inst_view[i] : 0u;
		VgxBox B = vgx_box_empty();
		bool keep = false;
		if (vgx_cull_valid(in, cache_meshes, view, nviews)) {
			keep = vgx_cull_decide(vgx_box_union_range(mesh_bounds, in.first_mesh, in.num_meshes), in.mtx, views + 4 * (uint64_t)view, &B);
		} else {
			status = VGX_E_INVALID_ARG;
		}
		if (!keep) { in.num_meshes = 0; }
		if (!keep || out->inst != inst) { out->inst[i] = in; }
		if (out->bounds) { vgx_box_store(out->bounds + 4 * i, B); }
		if (keep && out->kept) { out->kept[nk] = (uint32_t)i; }
		nk += keep ? 1u : 0u;
	}
	if (out->num_kept) { *out->num_kept = nk; }
	return status;
}

}

#include "vgx_pick.h"
#include <stdlib.h>

extern "C" {

// vgx_pick on the host: the functions of vgx_pick.h in a plain sequential loop over queries, meshes and triangles, with the call's
// contract (mesh_bounds may be NULL: the boxes are computed first, as the device call does). HOST pointers. Returns the status the
// device call returns for these arguments.
int vgxt_pick(const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_pick_query* queries, uint32_t nqueries, vgx_pick_hit* hits)
{
	if (!frame || (nqueries && (!queries || !hits))) { return VGX_E_INVALID_ARG; }
	if (nqueries > VGX_PICK_MAX_QUERIES || frame->num_meshes >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	const uint64_t nm = frame->num_meshes;
	float* own = nullptr;
	if (!mesh_bounds && nm) {
		own = (float*)malloc(nm * 4 * sizeof(float));
		if (!own) { return VGX_E_INTERNAL; }
		vgxt_mesh_bounds(frame->pos, frame->meshes, nm, own);
		mesh_bounds = own;
	}
	for (uint32_t q = 0; q < nqueries; ++q) {
		const vgx_pick_query Q = queries[q];
		uint64_t best = 0;
		for (uint64_t m = 0; m < nm && m < (uint64_t)Q.mesh_end; ++m) {
			const float* bx = mesh_bounds + 4 * m;
			if (!vgx_pick_in_box(Q.x, Q.y, bx[0], bx[1], bx[2], bx[3])) { continue; }
			const vgx_mesh me = frame->meshes[m];
			const uint16_t* ip = frame->idx + me.first_index;
			const float* pp = frame->pos + 2 * me.first_vertex;
			const uint32_t* cp = frame->color + me.first_vertex;
			for (uint32_t t = 0; t < vgx_pick_mesh_triangles(me); ++t) {
				const uint32_t i0 = ip[3 * t], i1 = ip[3 * t + 1], i2 = ip[3 * t + 2];
				if (!vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) { continue; }
				if ((Q.flags & VGX_PICK_SKIP_TRANSPARENT) && vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2])) { continue; }
				if (!vgx_pick_tri(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), v2(pp[2 * i2], pp[2 * i2 + 1]), Q.x, Q.y)) { continue; }
				const uint64_t key = vgx_pick_key((uint32_t)m, t);
				if (key > best) { best = key; }
			}
		}
		hits[q] = vgx_pick_decode(best, frame->meshes);
	}
	free(own);
	return VGX_OK;
}

// vgx_pick_frame on the host: the vgx_pickf_* functions of vgx_pick.h in a plain sequential loop over queries, the meshes of the range in
// ascending order (the stamp S walks with them) and their triangles or edges, with the call's whole contract (mesh_bounds may be NULL: the
// boxes are computed first). HOST pointers, the draw tables included. Returns the status the device call returns for these arguments;
// *status (may be NULL) receives what it leaves in dev_status
int vgxt_pick_frame(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                    const vgx_pick_query* queries, uint32_t nqueries, vgx_pick_hit* hits, uint32_t* status)
{
	const int rc = vgx_pickf_check_args(frame, mesh_bounds, state, queries, nqueries, hits, status);
	if (rc != VGX_OK) { return rc; }
	const uint64_t end = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
	bool invalid = false;
	for (uint64_t m = mesh_begin; m < end; ++m) { invalid = invalid || frame->meshes[m].draw >= state->num_draws; }
	if (status) { *status = invalid ? VGX_E_INVALID_ARG : VGX_OK; }
	float* own = nullptr;
	if (!mesh_bounds && mesh_begin < end && !invalid) {
		own = (float*)malloc(frame->num_meshes * 4 * sizeof(float));
		if (!own) { return VGX_E_INTERNAL; }
		vgxt_mesh_bounds(frame->pos, frame->meshes, frame->num_meshes, own);
		mesh_bounds = own;
	}
	for (uint32_t q = 0; q < nqueries; ++q) {
		const vgx_pick_query Q = queries[q];
		double px, py;
		int32_t X, Y;
		const bool point = vgx_pickf_point(Q.x, Q.y, &px, &py, &X, &Y);
		uint32_t S = VGX_RASTER_STAMP_NONE, best = VGX_PICK_NONE, bestT = VGX_PICK_NONE;
		// a mesh at or behind the query's mesh_end is no hit, and what it stamps is seen by meshes above it only
		for (uint64_t m = mesh_begin; m < end && m < (uint64_t)Q.mesh_end && point && !invalid; ++m) {
			const vgx_mesh me = frame->meshes[m];
			VgxPickfMesh st;
			vgx_pickf_mesh_state(me, state->draws[me.draw].state_key, state->draw_state[me.draw], &st);
			const float* box = mesh_bounds + 4 * m;
			if (!st.elems || !vgx_pickf_in_scissor(st.rect, X, Y) || !vgx_pickf_in_box(box, px, py)) { continue; }
			const uint16_t* ip = frame->idx + me.first_index;
			const float* pp = frame->pos + 2 * me.first_vertex;
			const uint32_t* cp = frame->color + me.first_vertex;
			const bool skips = vgx_pickf_skips(st.mode, Q.flags);
			bool covered = false;
			uint32_t top = VGX_PICK_NONE;
			if (vgx_raster_kind_is_contours(me.subpath_kind)) {
				if (skips && (cp[0] >> 24) == 0u) { continue; }
				int32_t W = 0;
				for (uint32_t k = 0; k < st.elems; ++k) {
					const uint32_t i0 = ip[2 * k], i1 = ip[2 * k + 1];
					if (i0 < me.num_vertices && i1 < me.num_vertices) { W += vgx_pickf_edge(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), px, py); }
				}
				covered = vgx_raster_contour_covered(W, me.subpath_kind, box, px, py);
			} else {
				for (uint32_t t = 0; t < st.elems; ++t) {
					const uint32_t i0 = ip[3 * t], i1 = ip[3 * t + 1], i2 = ip[3 * t + 2];
					if (!vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) { continue; }
					if (skips && vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2])) { continue; }
					if (vgx_pickf_tri(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), v2(pp[2 * i2], pp[2 * i2 + 1]), px, py)) { covered = true; top = t; }
				}
			}
			if (!covered) { continue; }
			if (st.mode == VGX_RF_STAMP) { S = st.f; }
			else if (vgx_pickf_hit(st.mode, st.f, st.n, S, m, Q.mesh_end)) { best = (uint32_t)m; bestT = top; }
		}
		hits[q] = vgx_pickf_record(best, bestT, frame->meshes);
	}
	free(own);
	return VGX_OK;
}

}

#include "vgx_pick_rect.h"

extern "C" {

// The predicate of vgx_pick_rect for one triangle (tri = ax, ay, bx, by, cx, cy) and one rectangle (rect = x0, y0, x1, y1): steps 1 to 4,
// step 4 in the header's four-corner form or in the one-corner form the kernels run
int vgxt_pick_rect_touch(const float* tri, const float* rect, int four_corners)
{
	vgx_pick_rect_query Q;
	Q.x0 = rect[0]; Q.y0 = rect[1]; Q.x1 = rect[2]; Q.y1 = rect[3]; Q.mesh_begin = 0u; Q.mesh_end = VGX_PICK_NONE; Q.flags = 0u; Q.reserved = 0u;
	VgxPickrTri T;
	vgx_pickr_setup(v2(tri[0], tri[1]), v2(tri[2], tri[3]), v2(tri[4], tri[5]), &T);
	return vgx_pickr_query_valid(Q) && vgx_pickr_touch(T, Q, four_corners != 0) ? 1 : 0;
}

// vgx_pick_rect on the host: the functions of vgx_pick_rect.h in a plain sequential loop over queries, the entries of the range in ascending
// order, their meshes and their triangles, with the call's contract (mesh_bounds may be NULL: the boxes are computed first). HOST pointers.
// Returns the status the device call returns for these arguments.
int vgxt_pick_rect(const vgx_cache_desc* frame, const float* mesh_bounds, const vgx_pick_rect_query* queries, uint32_t nqueries, const vgx_pick_rect_out* out)
{
	const int rc = vgx_pickr_check_args(frame, mesh_bounds, queries, nqueries, out);
	if (rc != VGX_OK) { return rc; }
	const uint64_t nm = frame->num_meshes;
	float* own = nullptr;
	if (!mesh_bounds && nm && nqueries) {
		own = (float*)malloc(nm * 4 * sizeof(float));
		if (!own) { return VGX_E_INTERNAL; }
		vgxt_mesh_bounds(frame->pos, frame->meshes, nm, own);
		mesh_bounds = own;
	}
	for (uint32_t q = 0; q < nqueries; ++q) {
		const vgx_pick_rect_query Q = queries[q];
		const bool window = (Q.flags & VGX_PICK_RECT_WINDOW) != 0u, byDraw = (Q.flags & VGX_PICK_RECT_BY_DRAW) != 0u;
		const uint64_t end = (uint64_t)Q.mesh_end < nm ? (uint64_t)Q.mesh_end : nm;
		uint32_t count = 0u, bestMesh = 0u, bestTri = 0u; // + 1, 0: none
		uint64_t m = vgx_pickr_query_valid(Q) ? (uint64_t)Q.mesh_begin : end;
		while (m < end) {
			uint64_t runEnd = m + 1;
			while (byDraw && runEnd < end && frame->meshes[runEnd].draw == frame->meshes[m].draw) { ++runEnd; }
			uint64_t touch = 0ull, inside = 1ull; // bit 0: this query
			uint32_t lastMesh = 0u, lastTri = 0u;
			for (uint64_t j = m; j < runEnd; ++j) {
				const float* bx = mesh_bounds + 4 * j;
				if (!vgx_pickr_box_inside(Q, bx[0], bx[1], bx[2], bx[3])) { inside = 0ull; }
				const vgx_mesh me = frame->meshes[j];
				if (!vgx_pickr_box_overlap(Q, bx[0], bx[1], bx[2], bx[3])) { continue; }
				const uint16_t* ip = frame->idx + me.first_index;
				const float* pp = frame->pos + 2 * me.first_vertex;
				const uint32_t* cp = frame->color + me.first_vertex;
				for (uint32_t t = 0; t < vgx_pick_mesh_triangles(me); ++t) {
					const uint32_t i0 = ip[3 * t], i1 = ip[3 * t + 1], i2 = ip[3 * t + 2];
					if (!vgx_pick_tri_valid(i0, i1, i2, me.num_vertices)) { continue; }
					if ((Q.flags & VGX_PICK_SKIP_TRANSPARENT) && vgx_pick_tri_transparent(cp[i0], cp[i1], cp[i2])) { continue; }
					VgxPickrTri T;
					vgx_pickr_setup(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), v2(pp[2 * i2], pp[2 * i2 + 1]), &T);
					if (vgx_pickr_touch(T, Q)) { touch = 1ull; lastMesh = (uint32_t)j + 1u; lastTri = t + 1u; }
				}
			}
			if (vgx_pickr_selected(touch, inside, window ? 1ull : 0ull) & 1ull) {
				if (count < out->list_cap) { out->list[(uint64_t)q * out->list_cap + count] = vgx_pickr_entry_value(Q, (uint32_t)m); }
				++count;
				bestMesh = lastMesh; bestTri = lastTri;
			}
			m = runEnd;
		}
		if (out->count) { out->count[q] = count; }
		if (out->top) { out->top[q] = vgx_pickr_record(bestMesh, bestTri, frame->meshes); }
	}
	free(own);
	return VGX_OK;
}

}

#include "vgx_raster.h"
#include "vgx_damage.h"
#include "vgx_concave_lane.h"
#include "vgx_triangulate_lane.h"

extern "C" {

// vgx_concave_contours on the host: the functions of vgx_concave_lane.h draw after draw and contour vertex after contour vertex. HOST
// pointers. Returns what the device call returns on the host; *status and *sizes (may be NULL) receive what it leaves in dev_status and
// dev_sizes. With a status other than VGX_OK no vertex and no index is written
int vgxt_concave_contours(const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                          const vgx_mesh_out* out, vgx_sizes* sizes, uint32_t* status)
{
	if (!out || !out->pos || !out->color || !out->idx || (ndraws && (!poly || !subpaths || !draw_info || !draws))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)out->pos & 7u) || ((uintptr_t)out->color & 3u) || ((uintptr_t)out->idx & 1u) || ((uintptr_t)out->meshes & 7u)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	uint32_t st = VGX_OK;
	uint64_t nc = 0, nv = 0, nm = 0;
	for (int pass = 0; pass < 2 && st == VGX_OK; ++pass) { // sizes and records, then -- the capacities hold -- the streams
		nc = nv = nm = 0;
		for (uint64_t i = 0; i < ndraws; ++i) {
			const vgx_draw& d = draws[i];
			uint64_t V;
			const int made = contours_draw_counts(d, draw_info[i], subpaths, &V);
			if (made < 0 && st == VGX_OK) { st = VGX_E_INVALID_ARG; }
			if (made <= 0) { continue; }
			const bool aa = (d.fill_flags & VGX_FILL_AA) != 0u;
			if ((aa ? 2 * V : V) > 65536u && st == VGX_OK) { st = VGX_E_MESH_TOO_LARGE; }
			const uint64_t fi = 2 * nc + 3 * (nv - nc);
			if (pass == 0) {
				vgx_mesh m[2];
				const uint32_t n = contours_draw_meshes(d, (uint32_t)i, V, nv, fi, m);
				for (uint32_t k = 0; k < n; ++k) { if (out->meshes && nm + k < out->cap_meshes) { out->meshes[nm + k] = m[k]; } }
			} else {
				for (uint64_t c = 0; c < V; ++c) {
					contours_emit_vertex(poly, subpaths + draw_info[i].first_subpath, draw_info[i].num_subpaths, d, c, V, nv, fi, out->pos, out->color, out->idx);
				}
			}
			nc += V; nv += aa ? 3 * V : V; nm += aa ? 2u : 1u;
		}
		const uint64_t ni = 2 * nc + 3 * (nv - nc);
		if (st == VGX_OK && (nv > out->cap_vertices || ni > out->cap_indices || (out->meshes && nm > out->cap_meshes))) { st = VGX_E_NOSPACE; }
		if (sizes) { memset(sizes, 0, sizeof(*sizes)); sizes->num_meshes = nm; sizes->num_vertices = nv; sizes->num_indices = ni; }
	}
	if (status) { *status = st; }
	return VGX_OK;
}

// vgx_concave_triangulate on the host: the rule of vgx_triangulate_lane.h ring after ring (tri_ring_route), then the draws one after the
// other as vgxt_concave_contours walks them. HOST pointers; draw_route (may be NULL) as the device call's. Returns what the device call
// returns on the host; *status and *sizes (may be NULL) receive what it leaves in dev_status and dev_sizes
int vgxt_concave_triangulate(const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                             const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* sizes, uint32_t* status)
{
	if (!out || !out->pos || !out->color || !out->idx || (ndraws && (!poly || !subpaths || !draw_info || !draws))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)out->pos & 7u) || ((uintptr_t)out->color & 3u) || ((uintptr_t)out->idx & 1u) || ((uintptr_t)out->meshes & 7u)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u) || ((uintptr_t)draw_route & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	const uint32_t cap = VGX_TRIANGULATE_MAX_VERTICES;
	V2* ring = (V2*)malloc(cap * sizeof(V2));
	uint16_t* links = (uint16_t*)malloc(2 * cap * sizeof(uint16_t));
	uint16_t* tri = (uint16_t*)malloc(3 * cap * sizeof(uint16_t));
	uint32_t* routes = (uint32_t*)malloc((ndraws + 1) * sizeof(uint32_t));
	if (!ring || !links || !tri || !routes) { free(ring); free(links); free(tri); free(routes); return VGX_E_INTERNAL; }
	uint32_t st = VGX_OK;
	uint64_t nv = 0, ni = 0, nm = 0;
	for (int pass = 0; pass < 2 && st == VGX_OK; ++pass) { // routes, sizes and records, then -- the capacities hold -- the streams
		nv = ni = nm = 0;
		for (uint64_t i = 0; i < ndraws; ++i) {
			const vgx_draw& d = draws[i];
			uint64_t V;
			int made;
			uint32_t route = tri_draw_class(d, draw_info[i], subpaths, &V, &made);
			if (made < 0 && st == VGX_OK) { st = VGX_E_INVALID_ARG; }
			const vgx_subpath* sp = subpaths + draw_info[i].first_subpath;
			if (route == VGX_TRI_ROUTE_TRIANGLES && (pass == 0 || routes[i] == VGX_TRI_ROUTE_TRIANGLES)) { // a refusal is known from pass 0
				for (uint32_t j = 0; j < (uint32_t)V; ++j) { ring[j] = tri_ring_vertex(poly + 2 * sp[0].first_vertex, (uint32_t)V, d, j); }
				route = tri_ring_route(ring, (uint32_t)V, links, links + cap, tri);
			} else if (pass == 1) {
				route = routes[i];
			}
			if (pass == 0) {
				routes[i] = route;
				if (draw_route) { draw_route[i] = route; }
			}
			if (route == 0u) { continue; }
			uint64_t dv, dn; uint32_t dm; bool big;
			tri_draw_sizes(d, route, V, &dv, &dn, &dm, &big);
			if (big && st == VGX_OK) { st = VGX_E_MESH_TOO_LARGE; }
			if (pass == 0) {
				vgx_mesh m[2];
				const uint32_t n = tri_draw_meshes(d, (uint32_t)i, route, V, nv, ni, m);
				for (uint32_t k = 0; k < n; ++k) { if (out->meshes && nm + k < out->cap_meshes) { out->meshes[nm + k] = m[k]; } }
			} else if (route == VGX_TRI_ROUTE_TRIANGLES) {
				for (uint64_t c = 0; c < V; ++c) { tri_emit_vertex(poly, sp, d, c, V, nv, ni, out->pos, out->color, out->idx); }
				for (uint64_t k = 0; k < 3 * (V - 2); ++k) { tri_emit_index(d, tri, k, V, ni, out->idx); }
			} else {
				for (uint64_t c = 0; c < V; ++c) { contours_emit_vertex(poly, sp, draw_info[i].num_subpaths, d, c, V, nv, ni, out->pos, out->color, out->idx); }
			}
			nv += dv; ni += dn; nm += dm;
		}
		if (st == VGX_OK && (nv > out->cap_vertices || ni > out->cap_indices || (out->meshes && nm > out->cap_meshes))) { st = VGX_E_NOSPACE; }
		if (sizes) { memset(sizes, 0, sizeof(*sizes)); sizes->num_meshes = nm; sizes->num_vertices = nv; sizes->num_indices = ni; }
	}
	free(ring); free(links); free(tri); free(routes);
	if (status) { *status = st; }
	return VGX_OK;
}

// vgx_concave_triangulate_rings on the host: vgxt_concave_triangulate with tri_rings_route in tri_ring_route's place and the sizes of
// a draw with holes. trips (may be NULL, [ndraws]): per draw the largest number of candidates one of its bridge searches tried
int vgxt_concave_triangulate_rings(const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                   const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* sizes, uint32_t* status, uint32_t* trips)
{
	if (!out || !out->pos || !out->color || !out->idx || (ndraws && (!poly || !subpaths || !draw_info || !draws))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)out->pos & 7u) || ((uintptr_t)out->color & 3u) || ((uintptr_t)out->idx & 1u) || ((uintptr_t)out->meshes & 7u)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u) || ((uintptr_t)draw_route & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	const uint32_t cap = VGX_TRIANGULATE_MAX_VERTICES;
	V2* ring = (V2*)malloc(cap * sizeof(V2));
	uint16_t* links = (uint16_t*)malloc((3 * cap + VGX_TRI_MAX_RINGS) * sizeof(uint16_t)); // vert, prev, next, mh
	uint16_t* tri = (uint16_t*)malloc(3 * cap * sizeof(uint16_t));
	uint32_t* routes = (uint32_t*)malloc((ndraws + 1) * sizeof(uint32_t));
	uint32_t* tried = (uint32_t*)malloc(VGX_TRI_MAX_RINGS * sizeof(uint32_t));
	int8_t* sgn = (int8_t*)malloc(VGX_TRI_MAX_RINGS);
	if (!ring || !links || !tri || !routes || !tried || !sgn) { free(ring); free(links); free(tri); free(routes); free(tried); free(sgn); return VGX_E_INTERNAL; }
	uint32_t st = VGX_OK;
	uint64_t nv = 0, ni = 0, nm = 0;
	for (int pass = 0; pass < 2 && st == VGX_OK; ++pass) { // routes, sizes and records, then -- the capacities hold -- the streams
		nv = ni = nm = 0;
		for (uint64_t i = 0; i < ndraws; ++i) {
			const vgx_draw& d = draws[i];
			uint64_t V;
			uint32_t H;
			int made;
			uint32_t route = tri_rings_draw_class(d, draw_info[i], subpaths, &V, &H, &made);
			if (made < 0 && st == VGX_OK) { st = VGX_E_INVALID_ARG; }
			const vgx_subpath* sp = subpaths + draw_info[i].first_subpath;
			if (pass == 0 && trips) { trips[i] = 0; }
			if (route == VGX_TRI_ROUTE_TRIANGLES && (pass == 0 || routes[i] == VGX_TRI_ROUTE_TRIANGLES)) { // a refusal is known from pass 0
				for (uint32_t j = 0; j < (uint32_t)V; ++j) { ring[j] = tri_rings_vertex(poly, sp, H + 1u, d, j); }
				for (uint32_t j = 0; j < H; ++j) { tried[j] = 0; }
				route = tri_rings_route(ring, (uint32_t)V, sp, H + 1u, (d.fill_flags & VGX_FILL_EVEN_ODD) != 0u, links, links + cap, links + 2 * cap, sgn, links + 3 * cap, tri, tried);
				if (pass == 0 && trips) { for (uint32_t j = 0; j < H; ++j) { if (tried[j] > trips[i]) { trips[i] = tried[j]; } } }
			} else if (pass == 1) {
				route = routes[i];
			}
			if (pass == 0) {
				routes[i] = route;
				if (draw_route) { draw_route[i] = route; }
			}
			if (route == 0u) { continue; }
			uint64_t dv, dn; uint32_t dm; bool big;
			tri_rings_draw_sizes(d, route, V, H, &dv, &dn, &dm, &big);
			if (big && st == VGX_OK) { st = VGX_E_MESH_TOO_LARGE; }
			if (pass == 0) {
				vgx_mesh m[2];
				const uint32_t n = tri_rings_draw_meshes(d, (uint32_t)i, route, V, H, nv, ni, m);
				for (uint32_t k = 0; k < n; ++k) { if (out->meshes && nm + k < out->cap_meshes) { out->meshes[nm + k] = m[k]; } }
			} else if (route == VGX_TRI_ROUTE_TRIANGLES) {
				for (uint64_t c = 0; c < V; ++c) { (void)contours_emit_vertex_data(poly, sp, H + 1u, d, c, V, nv, ni, out->pos, out->color, out->idx); }
				for (uint64_t k = 0; k < 3 * (V + 2 * H - 2); ++k) { tri_emit_index(d, tri, k, V, ni, out->idx); }
			} else {
				for (uint64_t c = 0; c < V; ++c) { contours_emit_vertex(poly, sp, H + 1u, d, c, V, nv, ni, out->pos, out->color, out->idx); }
			}
			nv += dv; ni += dn; nm += dm;
		}
		if (st == VGX_OK && (nv > out->cap_vertices || ni > out->cap_indices || (out->meshes && nm > out->cap_meshes))) { st = VGX_E_NOSPACE; }
		if (sizes) { memset(sizes, 0, sizeof(*sizes)); sizes->num_meshes = nm; sizes->num_vertices = nv; sizes->num_indices = ni; }
	}
	free(ring); free(links); free(tri); free(routes); free(tried); free(sgn);
	if (status) { *status = st; }
	return VGX_OK;
}

// vgx_concave_triangulate_nested on the host: vgxt_concave_triangulate_rings with tri_nested_route and the sizes of a draw of G groups.
// trips as there
int vgxt_concave_triangulate_nested(const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                    const vgx_mesh_out* out, uint32_t* draw_route, vgx_sizes* sizes, uint32_t* status, uint32_t* trips)
{
	if (!out || !out->pos || !out->color || !out->idx || (ndraws && (!poly || !subpaths || !draw_info || !draws))) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)out->pos & 7u) || ((uintptr_t)out->color & 3u) || ((uintptr_t)out->idx & 1u) || ((uintptr_t)out->meshes & 7u)) { return VGX_E_INVALID_ARG; }
	if (((uintptr_t)poly & 7u) || ((uintptr_t)subpaths & 7u) || ((uintptr_t)draw_info & 7u) || ((uintptr_t)draws & 3u) || ((uintptr_t)draw_route & 3u)) { return VGX_E_INVALID_ARG; }
	if (ndraws >= 0xFFFFFFFFull) { return VGX_E_RANGE; }
	const uint32_t cap = VGX_TRIANGULATE_MAX_VERTICES;
	V2* ring = (V2*)malloc(cap * sizeof(V2));
	uint16_t* links = (uint16_t*)malloc((3 * cap + 7 * VGX_TRI_MAX_RINGS) * sizeof(uint16_t)); // vert, prev, next, mh, tri_nested_route's six tables
	uint16_t* tri = (uint16_t*)malloc(3 * cap * sizeof(uint16_t));
	uint32_t* routes = (uint32_t*)malloc(2 * (ndraws + 1) * sizeof(uint32_t)); // and G per draw
	uint32_t* tried = (uint32_t*)malloc(VGX_TRI_MAX_RINGS * sizeof(uint32_t));
	int8_t* sgn = (int8_t*)malloc(VGX_TRI_MAX_RINGS);
	if (!ring || !links || !tri || !routes || !tried || !sgn) { free(ring); free(links); free(tri); free(routes); free(tried); free(sgn); return VGX_E_INTERNAL; }
	uint32_t* groups = routes + (ndraws + 1);
	uint32_t st = VGX_OK;
	uint64_t nv = 0, ni = 0, nm = 0;
	for (int pass = 0; pass < 2 && st == VGX_OK; ++pass) { // routes, sizes and records, then -- the capacities hold -- the streams
		nv = ni = nm = 0;
		for (uint64_t i = 0; i < ndraws; ++i) {
			const vgx_draw& d = draws[i];
			uint64_t V;
			uint32_t H;
			int made;
			uint32_t route = tri_rings_draw_class(d, draw_info[i], subpaths, &V, &H, &made);
			if (made < 0 && st == VGX_OK) { st = VGX_E_INVALID_ARG; }
			const vgx_subpath* sp = subpaths + draw_info[i].first_subpath;
			const uint32_t S = H + 1u;
			if (pass == 0) { groups[i] = 0; if (trips) { trips[i] = 0; } }
			if (route == VGX_TRI_ROUTE_TRIANGLES && (pass == 0 || routes[i] == VGX_TRI_ROUTE_TRIANGLES)) { // a refusal is known from pass 0
				for (uint32_t j = 0; j < (uint32_t)V; ++j) { ring[j] = tri_rings_vertex(poly, sp, S, d, j); }
				for (uint32_t j = 0; j < H; ++j) { tried[j] = 0; }
				route = tri_nested_route(ring, (uint32_t)V, sp, S, (d.fill_flags & VGX_FILL_EVEN_ODD) != 0u, links, links + cap, links + 2 * cap, sgn, links + 3 * cap,
				                         links + 3 * cap + VGX_TRI_MAX_RINGS, tri, &groups[i], tried);
				if (pass == 0 && trips) { for (uint32_t j = 0; j < H; ++j) { if (tried[j] > trips[i]) { trips[i] = tried[j]; } } }
			} else if (pass == 1) {
				route = routes[i];
			}
			if (pass == 0) {
				routes[i] = route;
				if (draw_route) { draw_route[i] = route; }
			}
			if (route == 0u) { continue; }
			uint64_t dv, dn; uint32_t dm; bool big;
			tri_nested_draw_sizes(d, route, V, S, groups[i], &dv, &dn, &dm, &big);
			if (big && st == VGX_OK) { st = VGX_E_MESH_TOO_LARGE; }
			if (pass == 0) {
				vgx_mesh m[2];
				const uint32_t n = tri_nested_draw_meshes(d, (uint32_t)i, route, V, S, groups[i], nv, ni, m);
				for (uint32_t k = 0; k < n; ++k) { if (out->meshes && nm + k < out->cap_meshes) { out->meshes[nm + k] = m[k]; } }
			} else if (route == VGX_TRI_ROUTE_TRIANGLES) {
				for (uint64_t c = 0; c < V; ++c) { (void)contours_emit_vertex_data(poly, sp, S, d, c, V, nv, ni, out->pos, out->color, out->idx); }
				for (uint64_t k = 0; k < 3 * (V + 2ull * S - 4ull * groups[i]); ++k) { tri_emit_index(d, tri, k, V, ni, out->idx); }
			} else {
				for (uint64_t c = 0; c < V; ++c) { contours_emit_vertex(poly, sp, S, d, c, V, nv, ni, out->pos, out->color, out->idx); }
			}
			nv += dv; ni += dn; nm += dm;
		}
		if (st == VGX_OK && (nv > out->cap_vertices || ni > out->cap_indices || (out->meshes && nm > out->cap_meshes))) { st = VGX_E_NOSPACE; }
		if (sizes) { memset(sizes, 0, sizeof(*sizes)); sizes->num_meshes = nm; sizes->num_vertices = nv; sizes->num_indices = ni; }
	}
	free(ring); free(links); free(tri); free(routes); free(tried); free(sgn);
	if (status) { *status = st; }
	return VGX_OK;
}

// vgx_raster on the host: the functions of vgx_raster.h in a plain loop over the meshes of the range, their triangles and the pixels
// of each triangle's box inside the scissor; with the call's contract (mesh_bounds may be NULL: the boxes are computed first; given,
// they are the prefilter they are on the device). HOST pointers, the target's pixels included. Returns the status the device call
// returns for these arguments; *status (may be NULL) receives what it leaves in dev_status. There is no scratch to outgrow here.
int vgxt_raster(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_target* target,
                uint32_t* status)
{
	const int rc = vgx_raster_check_args(VGX_RL_PLAIN, frame, mesh_bounds, mesh_begin, mesh_end, nullptr, nullptr, nullptr, target, status);
	if (rc != VGX_OK) { return rc; }
	const vgx_raster_target& t = *target;
	if (status) { *status = VGX_OK; }
	if (t.scissor[0] == t.scissor[2] || t.scissor[1] == t.scissor[3]) { return VGX_OK; }
	const uint64_t end = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
	float* own = nullptr;
	if (!mesh_bounds && mesh_begin < end) {
		own = (float*)malloc(frame->num_meshes * 4 * sizeof(float));
		if (!own) { return VGX_E_INTERNAL; }
		vgxt_mesh_bounds(frame->pos, frame->meshes, frame->num_meshes, own);
	}
	if (t.flags & VGX_RASTER_CLEAR) {
		for (uint32_t j = t.scissor[1]; j < t.scissor[3]; ++j) {
			for (uint32_t i = t.scissor[0]; i < t.scissor[2]; ++i) { t.pixels[(uint64_t)j * t.stride + i] = t.clear_color; }
		}
	}
	for (uint64_t m = mesh_begin; m < end; ++m) {
		const vgx_mesh me = frame->meshes[m];
		VgxRasterRect r;
		if (!vgx_raster_mesh_tiles(me, (mesh_bounds ? mesh_bounds : own) + 4 * m, t.x0, t.y0, t.scissor, VGX_RL_PLAIN, &r)) { continue; }
		const uint16_t* ip = frame->idx + me.first_index;
		const float* pp = frame->pos + 2 * me.first_vertex;
		const uint32_t* cp = frame->color + me.first_vertex;
		for (uint32_t k = 0; k < me.num_indices / 3u; ++k) {
			const uint32_t i0 = ip[3 * k], i1 = ip[3 * k + 1], i2 = ip[3 * k + 2];
			if (i0 >= me.num_vertices || i1 >= me.num_vertices || i2 >= me.num_vertices) { continue; }
			VgxRasterTri T;
			if (!vgx_raster_setup(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), v2(pp[2 * i2], pp[2 * i2 + 1]), cp[i0], cp[i1], cp[i2], &T)) { continue; }
			uint32_t a0, a1, b0, b1;
			if (!vgx_raster_span(T.minx, T.maxx, t.x0, t.scissor[0], t.scissor[2], &a0, &a1) || !vgx_raster_span(T.miny, T.maxy, t.y0, t.scissor[1], t.scissor[3], &b0, &b1)) { continue; }
			for (uint32_t j = b0; j <= b1; ++j) {
				for (uint32_t i = a0; i <= a1; ++i) {
					uint32_t* const p = t.pixels + (uint64_t)j * t.stride + i;
					const uint32_t d = vgx_raster_pixel(T, (double)(t.x0 + (int32_t)i) + 0.5, (double)(t.y0 + (int32_t)j) + 0.5, *p);
					if (d != *p) { *p = d; }
				}
			}
		}
	}
	free(own);
	return VGX_OK;
}

}

// The frame-level calls on the host: vgxt_raster's loop with the per-draw state of vgx_raster.h, a stamp image of its own and, as far as
// the level (VGX_RL_*) goes, the sampling and the paint functions. HOST pointers throughout, the images' pixels, the UV stream and the
// paint tables included. The meshes are looked at twice: first for an invalid one (nothing may be written then), then drawn.
// `damage` (vgxt_raster_damaged, else null = every tile): a pixel outside the marked tiles is neither cleared nor drawn to
static bool raster_pixel_damaged(const uint32_t* damage, const vgx_raster_target& t, uint32_t i, uint32_t j)
{
	return !damage || vgx_damage_bit(damage, (j / VGX_RASTER_TILE) * vgx_damage_tiles_w(t.width) + i / VGX_RASTER_TILE);
}

// One contour mesh of vgx_raster_concave: per pixel of the box inside the mesh's rectangle, W over the valid edges, then the flush
static void raster_contour_mesh(const vgx_cache_desc* frame, const vgx_mesh& me, const float* box, const VgxRasterMeshState& ms, const VgxRasterPaint& pr,
                                const vgx_raster_target& t, uint32_t* stamp, const uint32_t* damage)
{
	uint32_t a0, a1, b0, b1;
	if (!vgx_raster_span(box[0], box[2], t.x0, ms.rect[0], ms.rect[2], &a0, &a1) || !vgx_raster_span(box[1], box[3], t.y0, ms.rect[1], ms.rect[3], &b0, &b1)) { return; }
	const uint16_t* ip = frame->idx + me.first_index;
	const float* pp = frame->pos + 2 * me.first_vertex;
	const uint32_t c = frame->color[me.first_vertex];
	const auto pfetch = [&pr](uint32_t x, uint32_t y) { return pr.im.pixels[(uint64_t)y * pr.im.stride + x]; };
	for (uint32_t j = b0; j <= b1; ++j) {
		for (uint32_t i = a0; i <= a1; ++i) {
			if (!raster_pixel_damaged(damage, t, i, j)) { continue; }
			const double px = (double)(t.x0 + (int32_t)i) + 0.5, py = (double)(t.y0 + (int32_t)j) + 0.5;
			int32_t W = 0;
			for (uint32_t k = 0; k < me.num_indices / 2u; ++k) {
				const uint32_t i0 = ip[2 * k], i1 = ip[2 * k + 1];
				VgxRasterTri T;
				if (i0 < me.num_vertices && i1 < me.num_vertices && vgx_raster_contour_edge(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), &T)) {
					W += vgx_raster_contour_winding(T, px, py);
				}
			}
			if (!vgx_raster_contour_covered(W, me.subpath_kind, box, px, py)) { continue; }
			uint32_t* const p = t.pixels + (uint64_t)j * t.stride + i;
			const uint32_t d = vgx_raster_contour_pixel(c, ms.pad, pr, ms.mode, ms.f, ms.n, px, py, stamp + (size_t)j * t.width + i, *p, pfetch);
			if (d != *p) { *p = d; }
		}
	}
}

static int raster_frame_loop(int level, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                             const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* status,
                             const vgx_raster_damage* dmg = nullptr)
{
	const int rc = vgx_raster_check_args(level, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, status);
	if (rc != VGX_OK) { return rc; }
	if (dmg && vgx_damage_record_check(dmg) != VGX_OK) { return VGX_E_INVALID_ARG; }
	const uint32_t* const damage = dmg ? dmg->tile_bits : nullptr; // (max_entries: there is no sort here, and no window to outgrow)
	const vgx_raster_target& t = *target;
	if (status) { *status = VGX_OK; }
	if (t.scissor[0] == t.scissor[2] || t.scissor[1] == t.scissor[3]) { return VGX_OK; }
	// the tables of the level: the others are not there
	const vgx_raster_image* const images = level >= VGX_RL_TEXTURED ? tex->images : nullptr;
	const uint32_t numImages = level >= VGX_RL_TEXTURED ? tex->num_images : 0u;
	const vgx_paint* const gradients = level >= VGX_RL_PAINTED ? paints->gradients : nullptr;
	const vgx_paint* const patterns = level >= VGX_RL_PAINTED ? paints->patterns : nullptr;
	const uint32_t numGradients = level >= VGX_RL_PAINTED ? paints->num_gradients : 0u, numPatterns = level >= VGX_RL_PAINTED ? paints->num_patterns : 0u;
	const uint64_t end = mesh_end < frame->num_meshes ? mesh_end : frame->num_meshes;
	for (uint64_t m = mesh_begin; m < end; ++m) {
		const vgx_mesh me = frame->meshes[m];
		VgxRasterMeshState ms;
		ms.mode = VGX_RF_INVALID;
		if (me.draw < state->num_draws) {
			vgx_raster_mesh_state(level, me, state->draws[me.draw].state_key, state->draw_state[me.draw], t.x0, t.y0, t.scissor, images, numImages,
			                      gradients, numGradients, patterns, numPatterns, &ms);
		}
		if (ms.mode == VGX_RF_INVALID) {
			if (status) { *status = VGX_E_INVALID_ARG; }
			return VGX_OK;
		}
	}
	float* own = nullptr;
	if (!mesh_bounds && mesh_begin < end) {
		own = (float*)malloc(frame->num_meshes * 4 * sizeof(float));
		if (!own) { return VGX_E_INTERNAL; }
		vgxt_mesh_bounds(frame->pos, frame->meshes, frame->num_meshes, own);
	}
	uint32_t* stamp = (uint32_t*)malloc((size_t)t.width * t.height * sizeof(uint32_t));
	if (!stamp) { free(own); return VGX_E_INTERNAL; }
	for (size_t k = 0; k < (size_t)t.width * t.height; ++k) { stamp[k] = VGX_RASTER_STAMP_NONE; }
	if (t.flags & VGX_RASTER_CLEAR) {
		for (uint32_t j = t.scissor[1]; j < t.scissor[3]; ++j) {
			for (uint32_t i = t.scissor[0]; i < t.scissor[2]; ++i) {
				if (raster_pixel_damaged(damage, t, i, j)) { t.pixels[(uint64_t)j * t.stride + i] = t.clear_color; }
			}
		}
	}
	for (uint64_t m = mesh_begin; m < end; ++m) {
		const vgx_mesh me = frame->meshes[m];
		VgxRasterMeshState ms;
		vgx_raster_mesh_state(level, me, state->draws[me.draw].state_key, state->draw_state[me.draw], t.x0, t.y0, t.scissor, images, numImages,
		                      gradients, numGradients, patterns, numPatterns, &ms);
		const bool sampled = (ms.pad & VGX_RT_SAMPLED) != 0u;
		const vgx_raster_image im = sampled ? images[ms.pad & 0xFFFFu] : vgx_raster_image();
		const auto fetch = [&im](uint32_t x, uint32_t y) { return im.pixels[(uint64_t)y * im.stride + x]; };
		VgxRasterPaint pr;
		memset(&pr, 0, sizeof(pr));
		if (ms.pad & VGX_RT_PAINTED) { vgx_raster_paint_record(((ms.pad & VGX_RT_GRADIENT) ? gradients : patterns)[ms.pad & 0xFFFFu], images, &pr); }
		const auto pfetch = [&pr](uint32_t x, uint32_t y) { return pr.im.pixels[(uint64_t)y * pr.im.stride + x]; };
		VgxRasterRect r;
		if (ms.mode == VGX_RF_NOTHING || !vgx_raster_mesh_tiles(me, (mesh_bounds ? mesh_bounds : own) + 4 * m, t.x0, t.y0, ms.rect, level, &r)) { continue; }
		if (ms.pad & VGX_RT_CONTOUR) { // the winding number of every sample the box can hold, over all the mesh's edges, then rule and colour
			raster_contour_mesh(frame, me, (mesh_bounds ? mesh_bounds : own) + 4 * m, ms, pr, t, stamp, damage);
			continue;
		}
		const uint16_t* ip = frame->idx + me.first_index;
		const float* pp = frame->pos + 2 * me.first_vertex;
		const uint32_t* cp = frame->color + me.first_vertex;
		for (uint32_t k = 0; k < me.num_indices / 3u; ++k) {
			const uint32_t i0 = ip[3 * k], i1 = ip[3 * k + 1], i2 = ip[3 * k + 2];
			if (i0 >= me.num_vertices || i1 >= me.num_vertices || i2 >= me.num_vertices) { continue; }
			VgxRasterTri T;
			if (!vgx_raster_setup(v2(pp[2 * i0], pp[2 * i0 + 1]), v2(pp[2 * i1], pp[2 * i1 + 1]), v2(pp[2 * i2], pp[2 * i2 + 1]), cp[i0], cp[i1], cp[i2], &T)) { continue; }
			double uv[6];
			if (sampled) {
				vgx_raster_uv_widen(tex->uv, tex->uv_bytes, me.first_vertex + i0, uv);
				vgx_raster_uv_widen(tex->uv, tex->uv_bytes, me.first_vertex + i1, uv + 2);
				vgx_raster_uv_widen(tex->uv, tex->uv_bytes, me.first_vertex + i2, uv + 4);
			}
			uint32_t a0, a1, b0, b1;
			if (!vgx_raster_span(T.minx, T.maxx, t.x0, ms.rect[0], ms.rect[2], &a0, &a1) || !vgx_raster_span(T.miny, T.maxy, t.y0, ms.rect[1], ms.rect[3], &b0, &b1)) { continue; }
			for (uint32_t j = b0; j <= b1; ++j) {
				for (uint32_t i = a0; i <= a1; ++i) {
					if (!raster_pixel_damaged(damage, t, i, j)) { continue; }
					uint32_t* const p = t.pixels + (uint64_t)j * t.stride + i;
					const double px = (double)(t.x0 + (int32_t)i) + 0.5, py = (double)(t.y0 + (int32_t)j) + 0.5;
					uint32_t* const sp = stamp + (size_t)j * t.width + i;
					const uint32_t d = sampled ? vgx_raster_textured_pixel(T, uv, im, ms.mode, ms.f, ms.n, px, py, *sp, *p, fetch)
					                 : (ms.pad & VGX_RT_GRADIENT) ? vgx_raster_gradient_pixel(T, pr, ms.mode, ms.f, ms.n, px, py, *sp, *p)
					                 : (ms.pad & VGX_RT_PATTERN) ? vgx_raster_pattern_pixel(T, pr, ms.mode, ms.f, ms.n, px, py, *sp, *p, pfetch)
					                                             : vgx_raster_frame_pixel(T, ms.mode, ms.f, ms.n, px, py, sp, *p);
					if (d != *p) { *p = d; }
				}
			}
		}
	}
	free(stamp);
	free(own);
	return VGX_OK;
}

extern "C" {

int vgxt_raster_frame(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                      const vgx_raster_target* target, uint32_t* status)
{
	return raster_frame_loop(VGX_RL_FRAME, frame, mesh_bounds, mesh_begin, mesh_end, state, nullptr, nullptr, target, status);
}

int vgxt_raster_textured(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                         const vgx_raster_textures* tex, const vgx_raster_target* target, uint32_t* status)
{
	return raster_frame_loop(VGX_RL_TEXTURED, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, nullptr, target, status);
}

int vgxt_raster_concave(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                        const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* status)
{
	return raster_frame_loop(VGX_RL_CONCAVE, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, status);
}

// the winding number of the sample (px, py) over the n directed edges u[k] -> v[k] (2 floats each), for the tests of the predicate
int32_t vgxt_raster_winding(const float* u, const float* v, uint64_t n, double px, double py)
{
	int32_t W = 0;
	for (uint64_t k = 0; k < n; ++k) {
		VgxRasterTri T;
		if (vgx_raster_contour_edge(v2(u[2 * k], u[2 * k + 1]), v2(v[2 * k], v[2 * k + 1]), &T)) { W += vgx_raster_contour_winding(T, px, py); }
	}
	return W;
}

int vgxt_raster_painted(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                        const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* status)
{
	return raster_frame_loop(VGX_RL_PAINTED, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, status);
}

// the pieces of the paint rule, for the tests: t of a gradient at a paint coordinate, an end's channel as 8 bits, the square root
double vgxt_raster_gradient_t(const float* params, double qx, double qy) { return vgx_raster_gradient_t(params, qx, qy); }
uint32_t vgxt_raster_q8(float c) { return vgx_raster_q8(c); }
double vgxt_raster_sqrt(double x) { return vgx_raster_sqrt(x); }

// the pieces, for the tests of the predicate: the two canonical values of one directed edge u->v in a triangle of orientation
// `positive`, at (px, py), and whether the edge takes a tie
double vgxt_raster_edge(const float* u, const float* v, int positive, double px, double py, int* tie)
{
	VgxRasterEdge e;
	const uint32_t f = vgx_raster_edge(v2(u[0], u[1]), v2(v[0], v[1]), positive != 0, 0, &e);
	*tie = (f & VGX_RT_TIE(0)) != 0;
	return vgx_raster_edge_value(e, f, 0, px, py);
}

// coverage of one sample by one triangle (a, b, c: 2 floats each)
int vgxt_raster_cover(const float* a, const float* b, const float* c, double px, double py)
{
	VgxRasterTri T;
	double E[3], S;
	return vgx_raster_setup(v2(a[0], a[1]), v2(b[0], b[1]), v2(c[0], c[1]), 0, 0, 0, &T) && vgx_raster_cover(T, px, py, E, &S);
}

}

#include "vgx_update.h"

extern "C" {

// vgx_cache_layout on the host: the per-instance function of vgx_update.h summed instance after instance. HOST pointers. Returns the
// status the device call leaves in dev_status.
int vgxt_cache_layout(const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst, vgx_cache_slot* slots)
{
	int status = VGX_OK;
	vgx_cache_slot s;
	s.first_mesh = 0; s.first_vertex = 0; s.first_index = 0; s.cache_first_mesh = 0;
	for (uint64_t i = 0; i < ninst; ++i) {
		VgxRangeCounts n = { 0, 0, 0 };
		if (!vgx_cache_range_counts(*cache, inst[i], &n)) { status = VGX_E_INVALID_ARG; }
		s.cache_first_mesh = inst[i].first_mesh;
		slots[i] = s;
		s.first_mesh += n.meshes; s.first_vertex += n.vertices; s.first_index += n.indices;
	}
	s.cache_first_mesh = 0;
	slots[ninst] = s;
	return status;
}

// vgx_cache_update on the host: the listed entries one after the other in the order given (duplicates included), each through the
// functions the kernels of vgx_update.hip call. HOST pointers, `ndirty_limit` included (NULL: the whole list). Returns the status the
// device call leaves in dev_status.
int vgxt_cache_update(const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst, const vgx_cache_slot* slots,
                      const uint32_t* dirty, uint64_t ndirty, const uint64_t* ndirty_limit, const vgx_update_frame* frame)
{
	uint32_t flags = 0;
	const uint64_t nlist = (ndirty_limit && *ndirty_limit < ndirty) ? *ndirty_limit : ndirty;
	for (uint64_t j = 0; j < nlist; ++j) {
		const uint64_t d = dirty[j];
		VgxRangeCounts n;
		const uint32_t bad = vgx_update_classify(*cache, inst, ninst, slots, d, frame->num_vertices, frame->num_meshes, &n);
		flags |= bad;
		if (bad) { continue; }
		const vgx_cache_instance in = inst[d];
		const vgx_cache_slot s0 = slots[d];
		const uint64_t rangeFirst = vgx_cache_first_vertex(*cache, in.first_mesh);
		for (uint64_t v = 0; v < n.vertices; ++v) { // k_update_pos
			const float* c = cache->pos + 2 * (rangeFirst + v);
			const V2 r = v2xform(v2(c[0], c[1]), in.mtx);
			frame->pos[2 * (s0.first_vertex + v)] = r.x; frame->pos[2 * (s0.first_vertex + v) + 1] = r.y;
		}
		for (uint64_t k = 0; k < n.meshes; ++k) { // k_update_meshes
			const vgx_mesh src = cache->meshes[in.first_mesh + k];
			uint64_t off;
			const uint32_t nv = vgx_update_mesh_span(src, rangeFirst, n.vertices, &off);
			if (vgx_mesh_takes_instance_colour(src.subpath_kind)) {
				for (uint32_t v = 0; v < nv; ++v) { frame->color[s0.first_vertex + off + v] = in.color; }
			}
			if (frame->mesh_bounds) {
				uint32_t lox = VGX_ORD_POS_INF, loy = VGX_ORD_POS_INF, hix = VGX_ORD_NEG_INF, hiy = VGX_ORD_NEG_INF;
				for (uint32_t v = 0; v < nv; ++v) {
					const float* c = cache->pos + 2 * (rangeFirst + off + v);
					const V2 r = v2xform(v2(c[0], c[1]), in.mtx);
					const uint32_t x = vgx_ord_from_float(r.x), y = vgx_ord_from_float(r.y);
					if (x < lox) { lox = x; }
					if (y < loy) { loy = y; }
					if (x > hix) { hix = x; }
					if (y > hiy) { hiy = y; }
				}
				float* b = frame->mesh_bounds + 4 * (s0.first_mesh + k);
				b[0] = vgx_float_from_ord(lox); b[1] = vgx_float_from_ord(loy); b[2] = vgx_float_from_ord(hix); b[3] = vgx_float_from_ord(hiy);
			}
		}
	}
	return vgx_update_status(flags);
}

// The damage marks on the host: the functions of vgx_damage.h box after box, ORing plainly. HOST pointers. vgxt_damage_instances walks
// the list in the order given and returns the status the device call leaves in dev_status; vgxt_damage_meshes returns VGX_OK.
static void damage_mark_host(const float* box, const vgx_raster_target* t, uint32_t* bits)
{
	VgxRasterRect r;
	if (!vgx_damage_box_tiles(box, t->x0, t->y0, t->width, t->height, &r)) { return; }
	vgx_tile_rect_words(r, vgx_damage_tiles_w(t->width), [bits](uint32_t w, uint32_t mask) { bits[w] |= mask; });
}

int vgxt_damage_meshes(const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, uint64_t num_meshes, const vgx_raster_target* target, uint32_t* tile_bits)
{
	const uint64_t end = mesh_end < num_meshes ? mesh_end : num_meshes;
	for (uint64_t m = mesh_begin; m < end; ++m) { damage_mark_host(mesh_bounds + 4 * m, target, tile_bits); }
	return VGX_OK;
}

int vgxt_damage_instances(const float* mesh_bounds, uint64_t num_meshes, const vgx_cache_slot* slots, uint64_t ninst, const uint32_t* dirty, uint64_t ndirty,
                          const uint64_t* ndirty_limit, const vgx_raster_target* target, uint32_t* tile_bits)
{
	int status = VGX_OK;
	const uint64_t nlist = (ndirty_limit && *ndirty_limit < ndirty) ? *ndirty_limit : ndirty;
	for (uint64_t j = 0; j < nlist; ++j) {
		uint64_t first, count;
		if (!vgx_damage_entry(slots, ninst, num_meshes, dirty[j], &first, &count)) { status = VGX_E_INVALID_ARG; continue; }
		for (uint64_t k = 0; k < count; ++k) { damage_mark_host(mesh_bounds + 4 * (first + k), target, tile_bits); }
	}
	return status;
}

// vgx_raster_damaged on the host: the frame-level loop at the concave level, writing inside the marked tiles alone
int vgxt_raster_damaged(const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                        const vgx_raster_textures* tex, const vgx_raster_paints* paints, const vgx_raster_target* target, const vgx_raster_damage* damage,
                        uint32_t* status)
{
	if (!damage) { return VGX_E_INVALID_ARG; }
	return raster_frame_loop(VGX_RL_CONCAVE, frame, mesh_bounds, mesh_begin, mesh_end, state, tex, paints, target, status, damage);
}

uint64_t vgxt_damage_words(uint32_t width, uint32_t height) { return ((uint64_t)vgx_damage_tiles_w(width) * vgx_damage_tiles_w(height) + 31u) / 32u; }

}

#include "vgx_raster_cmds.h"
#include "vgx_cmd_bounds.h"

// vgx_raster_commands on the host, in the kernels' own decomposition (vgx_raster_cmds.h): the state of every command, the rectangle of
// tiles of every chunk of 64 triangles, then tile after tile the chunks whose rectangle holds the tile, in ascending order, their
// triangles tested against the tile cut by both scissors as the tile kernel tests them. HOST pointers, the table, the real count
// (real_cmds, may be NULL), the images' pixels and the paint tables included. totals (may be NULL) receives the chunks and the bin
// entries the device call counts. There is no scratch to outgrow here: *status is VGX_OK, VGX_E_INVALID_ARG or VGX_E_RANGE.
// `dmg` (vgxt_raster_commands_damaged, else null = every tile) with cmd_bounds (may be NULL): a command whose box reaches no marked tile
// has no chunks, a bin entry is a pair of a chunk and a MARKED tile, and an unmarked tile is neither cleared nor drawn to (max_entries:
// there is no sort here, and no window to outgrow)
static int raster_commands_loop(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const float* cmd_bounds,
                                const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target,
                                const vgx_raster_damage* dmg, uint32_t* status, uint64_t* totals)
{
	const int rc = vgx_rasterc_check_args(streams, cmds, num_cmds, real_cmds, images, num_images, paints, target, status);
	if (rc != VGX_OK) { return rc; }
	if (dmg && (vgx_damage_record_check(dmg) != VGX_OK || ((uintptr_t)cmd_bounds & 15u))) { return VGX_E_INVALID_ARG; }
	const uint32_t* const damage = dmg ? dmg->tile_bits : nullptr;
	const vgx_raster_target& t = *target;
	if (status) { *status = VGX_OK; }
	if (totals) { totals[0] = totals[1] = 0; }
	if (t.scissor[0] == t.scissor[2] || t.scissor[1] == t.scissor[3]) { return VGX_OK; }
	const uint32_t n = real_cmds && *real_cmds < num_cmds ? *real_cmds : num_cmds;
	VgxRastercTables tb;
	tb.num_vertices = streams->num_vertices; tb.num_indices = streams->num_indices; tb.real_cmds = n; tb.has_uv = streams->uv ? 1u : 0u;
	tb.images = images; tb.num_images = num_images;
	tb.gradients = paints ? paints->gradients : nullptr; tb.num_gradients = paints ? paints->num_gradients : 0u;
	tb.patterns = paints ? paints->patterns : nullptr; tb.num_patterns = paints ? paints->num_patterns : 0u;
	std::vector<VgxRasterMeshState> state(n);
	std::vector<VgxRasterRect> rect;   // per chunk
	std::vector<uint32_t> chunkCmd, chunkTri;
	bool invalid = false;
	uint64_t entries = 0;
	for (uint32_t c = 0; c < n; ++c) {
		vgx_rasterc_cmd_state(cmds[c], c, tb, t.x0, t.y0, t.scissor, &state[c]);
		invalid = invalid || state[c].mode == VGX_RF_INVALID;
		if (damage && cmd_bounds && state[c].mode != VGX_RF_INVALID && state[c].mode != VGX_RF_NOTHING
		 && !vgx_cmdb_damaged(cmd_bounds + 4ull * c, damage, t.x0, t.y0, t.width, t.height)) { state[c].mode = VGX_RF_NOTHING; }
		const uint32_t chunks = vgx_rasterc_state_chunks(cmds[c], state[c]);
		for (uint32_t k = 0; k < chunks; ++k) {
			VgxRasterRect r = vgx_rasterc_rect_empty();
			for (uint32_t q = 0; q < VGX_RASTERC_CHUNK; ++q) {
				uint64_t v[3];
				if (!vgx_rasterc_triangle(cmds[c], streams->idx, k * VGX_RASTERC_CHUNK + q, v)) { continue; }
				const float* pp = streams->pos;
				r = vgx_rasterc_rect_union(r, vgx_rasterc_triangle_tiles(v2(pp[2 * v[0]], pp[2 * v[0] + 1]), v2(pp[2 * v[1]], pp[2 * v[1] + 1]), v2(pp[2 * v[2]], pp[2 * v[2] + 1]),
				                                                         t.x0, t.y0, state[c].rect));
			}
			rect.push_back(r); chunkCmd.push_back(c); chunkTri.push_back(k * VGX_RASTERC_CHUNK);
			entries += damage ? vgx_damage_rect_count(damage, r, vgx_damage_tiles_w(t.width)) : vgx_rasterc_rect_entries(r);
		}
	}
	if (totals) { totals[0] = rect.size(); totals[1] = entries; }
	const uint32_t st = vgx_rasterc_status(rect.size(), entries, invalid, ~0ull, ~0ull);
	if (status) { *status = st; }
	if (st != VGX_OK) { return VGX_OK; }
	const uint32_t tilesX0 = t.scissor[0] / VGX_RASTER_TILE, tilesY0 = t.scissor[1] / VGX_RASTER_TILE;
	const uint32_t tilesX1 = (t.scissor[2] - 1u) / VGX_RASTER_TILE, tilesY1 = (t.scissor[3] - 1u) / VGX_RASTER_TILE;
	for (uint32_t ty = tilesY0; ty <= tilesY1; ++ty) {
		for (uint32_t tx = tilesX0; tx <= tilesX1; ++tx) {
			const uint32_t ox = tx * VGX_RASTER_TILE, oy = ty * VGX_RASTER_TILE;
			if (damage && !vgx_damage_bit(damage, ty * vgx_damage_tiles_w(t.width) + tx)) { continue; } // ahead of the clear: the tile is not redrawn
			uint32_t S[VGX_RASTER_TILE * VGX_RASTER_TILE];
			for (uint32_t q = 0; q < VGX_RASTER_TILE * VGX_RASTER_TILE; ++q) { S[q] = VGX_RASTER_STAMP_NONE; }
			if (t.flags & VGX_RASTER_CLEAR) {
				for (uint32_t j = oy > t.scissor[1] ? oy : t.scissor[1]; j < oy + VGX_RASTER_TILE && j < t.scissor[3]; ++j) {
					for (uint32_t i = ox > t.scissor[0] ? ox : t.scissor[0]; i < ox + VGX_RASTER_TILE && i < t.scissor[2]; ++i) { t.pixels[(uint64_t)j * t.stride + i] = t.clear_color; }
				}
			}
			for (size_t k = 0; k < rect.size(); ++k) { // the tile's run of entries: ascending chunk ordinal
				const VgxRasterRect& r = rect[k];
				if (vgx_rasterc_rect_is_empty(r) || tx < r.tx0 || tx > r.tx1 || ty < r.ty0 || ty > r.ty1) { continue; }
				const vgx_raster_cmd& cmd = cmds[chunkCmd[k]];
				const VgxRasterMeshState& ms = state[chunkCmd[k]];
				// the command's rectangle cut to this tile
				const uint32_t cx0 = ox > ms.rect[0] ? ox : ms.rect[0], cx1 = ox + VGX_RASTER_TILE < ms.rect[2] ? ox + VGX_RASTER_TILE : ms.rect[2];
				const uint32_t cy0 = oy > ms.rect[1] ? oy : ms.rect[1], cy1 = oy + VGX_RASTER_TILE < ms.rect[3] ? oy + VGX_RASTER_TILE : ms.rect[3];
				if (cx0 >= cx1 || cy0 >= cy1) { continue; }
				const bool sampled = (ms.pad & VGX_RT_SAMPLED) != 0u;
				const vgx_raster_image im = sampled ? images[ms.pad & 0xFFFFu] : vgx_raster_image();
				const auto fetch = [&im](uint32_t x, uint32_t y) { return im.pixels[(uint64_t)y * im.stride + x]; };
				VgxRasterPaint pr;
				memset(&pr, 0, sizeof(pr));
				if (ms.pad & VGX_RT_PAINTED) { vgx_raster_paint_record(((ms.pad & VGX_RT_GRADIENT) ? tb.gradients : tb.patterns)[ms.pad & 0xFFFFu], images, &pr); }
				const auto pfetch = [&pr](uint32_t x, uint32_t y) { return pr.im.pixels[(uint64_t)y * pr.im.stride + x]; };
				for (uint32_t q = 0; q < VGX_RASTERC_CHUNK; ++q) {
					uint64_t v[3];
					if (!vgx_rasterc_triangle(cmd, streams->idx, chunkTri[k] + q, v)) { continue; }
					const float* pp = streams->pos;
					const bool stamp = ms.mode == VGX_RF_STAMP; // a clip command's colours are not read
					VgxRasterTri T;
					if (!vgx_raster_setup(v2(pp[2 * v[0]], pp[2 * v[0] + 1]), v2(pp[2 * v[1]], pp[2 * v[1] + 1]), v2(pp[2 * v[2]], pp[2 * v[2] + 1]),
					                      stamp ? 0u : streams->color[v[0]], stamp ? 0u : streams->color[v[1]], stamp ? 0u : streams->color[v[2]], &T)) { continue; }
					uint32_t a0, a1, b0, b1;
					if (!vgx_raster_span(T.minx, T.maxx, t.x0, cx0, cx1, &a0, &a1) || !vgx_raster_span(T.miny, T.maxy, t.y0, cy0, cy1, &b0, &b1)) { continue; }
					double uv[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
					if (sampled) {
						vgx_raster_uv_widen(streams->uv, streams->uv_bytes, v[0], uv);
						vgx_raster_uv_widen(streams->uv, streams->uv_bytes, v[1], uv + 2);
						vgx_raster_uv_widen(streams->uv, streams->uv_bytes, v[2], uv + 4);
					}
					for (uint32_t j = b0; j <= b1; ++j) {
						for (uint32_t i = a0; i <= a1; ++i) {
							uint32_t* const p = t.pixels + (uint64_t)j * t.stride + i;
							const double px = (double)(t.x0 + (int32_t)i) + 0.5, py = (double)(t.y0 + (int32_t)j) + 0.5;
							uint32_t* const sp = S + (j - oy) * VGX_RASTER_TILE + (i - ox);
							const uint32_t d = sampled ? vgx_raster_textured_pixel(T, uv, im, ms.mode, ms.f, ms.n, px, py, *sp, *p, fetch)
							                 : (ms.pad & VGX_RT_GRADIENT) ? vgx_raster_gradient_pixel(T, pr, ms.mode, ms.f, ms.n, px, py, *sp, *p)
							                 : (ms.pad & VGX_RT_PATTERN) ? vgx_raster_pattern_pixel(T, pr, ms.mode, ms.f, ms.n, px, py, *sp, *p, pfetch)
							                                             : vgx_raster_frame_pixel(T, ms.mode, ms.f, ms.n, px, py, sp, *p);
							if (d != *p) { *p = d; }
						}
					}
				}
			}
		}
	}
	return VGX_OK;
}

extern "C" {

int vgxt_raster_commands(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const vgx_raster_image* images,
                         uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* status, uint64_t* totals)
{
	return raster_commands_loop(streams, cmds, num_cmds, real_cmds, nullptr, images, num_images, paints, target, nullptr, status, totals);
}

// vgx_raster_commands_damaged on the host: the same loop inside the marked tiles alone, the commands their boxes let out skipped
int vgxt_raster_commands_damaged(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const float* cmd_bounds,
                                 const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints, const vgx_raster_target* target,
                                 const vgx_raster_damage* damage, uint32_t* status, uint64_t* totals)
{
	if (!damage) { return VGX_E_INVALID_ARG; }
	return raster_commands_loop(streams, cmds, num_cmds, real_cmds, cmd_bounds, images, num_images, paints, target, damage, status, totals);
}

// vgx_raster_cmds_from_assembly on the host: one record per draw command, the clip region mapped from draws to commands by two searches
int vgxt_raster_cmds_from_assembly(const vgx_drawcmd* drawcmds, uint64_t num_drawcmds, const vgx_mesh* meshes, uint64_t num_meshes, const vgx_raster_draws* state,
                                   vgx_raster_cmd* out, uint32_t* num_cmds, uint32_t* status)
{
	if (!state || !num_cmds || (num_drawcmds && (!drawcmds || !out)) || (num_meshes && !meshes) || state->reserved != 0u || (state->num_draws && !state->draw_state)) {
		return VGX_E_INVALID_ARG;
	}
	if (num_drawcmds > 0xFFFFFFFFull) { return VGX_E_RANGE; }
	bool bad = false;
	for (uint64_t m = 0; m < num_meshes; ++m) { bad = bad || vgx_raster_kind_is_contours(meshes[m].subpath_kind); }
	const auto draw_of = [&](uint64_t k) { const uint64_t m = drawcmds[k].first_mesh; return m < num_meshes ? meshes[m].draw : 0xFFFFFFFFu; };
	const auto first_of = [&](uint64_t d) {
		uint64_t lo = 0, hi = num_drawcmds;
		while (lo < hi) {
			const uint64_t mid = lo + ((hi - lo) >> 1);
			if ((uint64_t)draw_of(mid) < d) { lo = mid + 1u; } else { hi = mid; }
		}
		return lo;
	};
	for (uint64_t k = 0; k < num_drawcmds; ++k) {
		const vgx_drawcmd& dc = drawcmds[k];
		vgx_raster_cmd c;
		memset(&c, 0, sizeof(c));
		c.first_vertex = dc.first_vertex; c.first_index = dc.first_index; c.num_vertices = dc.num_vertices; c.num_indices = dc.num_indices;
		c.type = vgx_raster_draw_type(dc.state_key); c.handle = dc.state_key & 0xFFFFu;
		c.clip_first_cmd = VGX_RASTERC_NONE;
		const uint32_t d = draw_of(k);
		if (dc.first_mesh >= num_meshes || d >= state->num_draws) {
			bad = true;
		} else {
			const vgx_draw_state& ds = state->draw_state[d];
			for (int q = 0; q < 4; ++q) { c.scissor[q] = ds.scissor[q]; }
			c.clip_rule = ds.clip_rule;
			if (ds.clip_first_draw != VGX_RASTER_STAMP_NONE && ds.clip_num_draws != 0u) {
				const uint64_t first = first_of(ds.clip_first_draw), end = first_of((uint64_t)ds.clip_first_draw + ds.clip_num_draws);
				c.clip_first_cmd = (uint32_t)first; c.clip_num_cmds = (uint32_t)(end - first);
			}
		}
		out[k] = c;
	}
	*num_cmds = (uint32_t)num_drawcmds;
	if (status) { *status = bad ? VGX_E_INVALID_ARG : VGX_OK; }
	return VGX_OK;
}

}

#include "vgx_pick_cmds.h"

// vgx_pick_commands on the host: the functions of vgx_pick_cmds.h in a plain sequential loop over queries, the commands in ascending
// order (the stamp S walks with them) and their triangles, with the call's whole contract. HOST pointers, the owners' table included;
// real_cmds (may be NULL) plays dev_num_cmds. Returns the status the device call returns for these arguments; *status (may be NULL)
// receives what it leaves in dev_status
// cmd_bounds (may be NULL) is the one clause vgx_pick_commands_boxed adds (vgx_cmd_bounds.h: vgx_cmdb_holds)
static int pick_commands_loop(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const float* cmd_bounds,
                              const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits, uint32_t* status)
{
	const int rc = vgx_pickc_check_args(streams, cmds, num_cmds, real_cmds, owners, queries, nqueries, hits, status);
	if (rc != VGX_OK) { return rc; }
	if ((uintptr_t)cmd_bounds & 15u) { return VGX_E_INVALID_ARG; }
	const uint32_t n = real_cmds && *real_cmds < num_cmds ? *real_cmds : num_cmds;
	std::vector<VgxPickfMesh> state(n);
	bool invalid = false;
	for (uint32_t c = 0; c < n; ++c) {
		vgx_pickc_cmd_state(cmds[c], c, streams->num_vertices, streams->num_indices, n, &state[c]);
		invalid = invalid || state[c].mode == VGX_RF_INVALID;
	}
	if (status) { *status = invalid ? VGX_E_INVALID_ARG : VGX_OK; }
	for (uint32_t q = 0; q < nqueries; ++q) {
		const vgx_pick_cmd_query Q = queries[q];
		double px, py;
		int32_t X, Y;
		const bool point = vgx_pickc_point(Q, &px, &py, &X, &Y);
		uint32_t S = VGX_RASTER_STAMP_NONE, best = VGX_PICK_NONE, bestT = VGX_PICK_NONE;
		for (uint32_t c = 0; c < n && point && !invalid; ++c) {
			const VgxPickfMesh& st = state[c];
			if (!st.elems || !vgx_pickf_in_scissor(st.rect, X, Y) || (cmd_bounds && !vgx_cmdb_holds(cmd_bounds + 4ull * c, Q.x, Q.y))) { continue; }
			bool counted = false;
			uint32_t top = VGX_PICK_NONE;
			for (uint32_t t = 0; t < st.elems; ++t) {
				uint64_t v[3];
				if (!vgx_rasterc_triangle(cmds[c], streams->idx, t, v)) { continue; }
				const float* pp = streams->pos;
				if (!vgx_pickf_tri(v2(pp[2 * v[0]], pp[2 * v[0] + 1]), v2(pp[2 * v[1]], pp[2 * v[1] + 1]), v2(pp[2 * v[2]], pp[2 * v[2] + 1]), px, py)) { continue; }
				// a clip command's colours are not read
				const bool transparent = st.mode != VGX_RF_STAMP && vgx_pick_tri_transparent(streams->color[v[0]], streams->color[v[1]], streams->color[v[2]]);
				if (vgx_pickc_counts(st.mode, c, t, transparent, Q.cmd_end, Q.tri_end, Q.flags)) { counted = true; top = t; }
			}
			if (!counted) { continue; }
			if (st.mode == VGX_RF_STAMP) { S = c; }
			else if (vgx_pickc_hit(st.mode, st.f, st.n, S)) { best = c; bestT = top; }
		}
		hits[q] = vgx_pickc_record(best, bestT, cmds, owners ? owners->meshes : nullptr, owners ? owners->num_meshes : 0);
	}
	return VGX_OK;
}

extern "C" {

// vgx_pick_commands on the host: the loop above without boxes
int vgxt_pick_commands(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const vgx_pick_owners* owners,
                       const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits, uint32_t* status)
{
	return pick_commands_loop(streams, cmds, num_cmds, real_cmds, nullptr, owners, queries, nqueries, hits, status);
}

// vgx_pick_commands_boxed on the host: the same loop with the box clause of vgx_cmd_bounds.h (vgx_cmdb_holds); cmd_bounds may be NULL
int vgxt_pick_commands_boxed(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, const float* cmd_bounds,
                             const vgx_pick_owners* owners, const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits, uint32_t* status)
{
	return pick_commands_loop(streams, cmds, num_cmds, real_cmds, cmd_bounds, owners, queries, nqueries, hits, status);
}

// the owner search alone: the mesh that owns position p of the index stream, 0xFFFFFFFF: none
uint32_t vgxt_pick_owner(const vgx_mesh* meshes, uint64_t num_meshes, uint64_t p) { return vgx_pickc_owner(meshes, num_meshes, p); }

// vgx_command_bounds on the host: the functions of vgx_cmd_bounds.h command after command and triangle after triangle over the range,
// the order-preserving images decoded at the end as the call's last kernel does. HOST pointers; real_cmds (may be NULL) plays
// dev_num_cmds. Returns the status the device call returns for these arguments; *status (may be NULL) receives what it leaves in
// dev_status. Entries outside the range are not written
int vgxt_command_bounds(const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds, const uint32_t* real_cmds, uint32_t cmd_begin, uint32_t cmd_end,
                        float* bounds, uint32_t* status)
{
	const int rc = vgx_cmdb_check_args(streams, cmds, num_cmds, real_cmds, cmd_begin, cmd_end, bounds, status);
	if (rc != VGX_OK) { return rc; }
	const uint32_t n = vgx_cmdb_range(real_cmds && *real_cmds < num_cmds ? *real_cmds : num_cmds, cmd_begin, cmd_end);
	bool invalid = false;
	for (uint32_t i = 0; i < n; ++i) {
		const vgx_raster_cmd& c = cmds[cmd_begin + i];
		const uint32_t chunks = vgx_cmdb_chunks(c, streams->num_vertices, streams->num_indices);
		invalid = invalid || !vgx_cmdb_valid(c, streams->num_vertices, streams->num_indices);
		VgxOrdBox b = vgx_ordbox_empty();
		for (uint64_t t = 0; t < (uint64_t)chunks * VGX_RASTERC_CHUNK; ++t) { b = vgx_ordbox_union(b, vgx_cmdb_triangle(c, streams->idx, streams->pos, (uint32_t)t)); }
		float* e = bounds + 4ull * (cmd_begin + i);
		e[0] = vgx_float_from_ord(b.minx); e[1] = vgx_float_from_ord(b.miny); e[2] = vgx_float_from_ord(b.maxx); e[3] = vgx_float_from_ord(b.maxy);
	}
	if (status) { *status = invalid ? VGX_E_INVALID_ARG : VGX_OK; }
	return VGX_OK;
}

}
