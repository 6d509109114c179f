// vgx_chunk.h -- the chunk step of the command-parallel flatten kernels: k_flatten<EMIT, XFORM> and k_flatten_build
// (vgx_flatten.hip) and k_flat1<CAP> (vgx_flat1.hip). A wave walks its segment 64 command instances at a time, one lane
// per path command, and every such chunk takes the same three steps around the kernel's own walk and stores:
//   chunk_decode   the lane's draw (from the lane-resident draw window), its command record and the draw's fields
//   chunk_book     the polyline's bookkeeping segmented by draw and by sub-path: two scans, pathClose, per-draw totals
//   ChunkCarry     what the draw / sub-path that continues into the next chunk hands over
// Everything is force-inlined into its kernel; where the kernels differ the difference is a named template switch.
// Device only.
#ifndef VGX_CHUNK_H
#define VGX_CHUNK_H

#include "vgx_internal.h"
#include "vgx_wave.h"
#include "vgx_walk.h"

namespace {

// ---- decode --------------------------------------------------------------------------------------------------------
struct ChunkCmd // what a lane knows about its command instance before the walk (an invalid lane: a CLOSE of draw d0 without flags)
{
	uint64_t d;            // draw
	const vgx_draw* dr;
	uint64_t ownerBase;    // cmd_prefix[d]
	uint32_t recIndex;     // index of the command in the path set
	VgxCmdRec rec;         // type, flags, start point, arguments 0..7 (a[6..7]: the sub-path's first point)
	bool drawHead, drawLast; // first / last command of its draw
	uint32_t serialStatic; // the path takes the serial lane path (ARC / ARC_TO / shapes)
	float scale, tol;
	uint32_t fillFlags, strokeFlags;
};

// Valid lanes of the chunk (the last chunk of a segment is partly empty).
__device__ __forceinline__ int chunk_valid_lanes(uint64_t C1, uint64_t chunk)
{
	return (int)((C1 - chunk) < (uint64_t)VGX_WAVE ? (C1 - chunk) : (uint64_t)VGX_WAVE);
}

// The owner draw of every lane from the draw window (refilled at `dcur`, the draw of the previous chunk's last command,
// when it does not reach the chunk's end), then the command record and the draw's fields.
//   REFILL_BEHIND  also refill when the window starts behind dcur. Set by k_flatten_build and k_flat1, not by k_flatten;
//                  no kernel moves dcur below wbase today (NOTEBOOK.md), the switch keeps each kernel's test as it was.
//   THIN           VGX_PF_THIN paths read the 16-byte thin records. Set by k_flatten_build only: the only reader of ps.cmdthin.
// `extra(D)`: the kernel's own loads for a valid lane, requested together with the draw's fields (a load issued behind the
// call waits for the records first).
template<bool REFILL_BEHIND, bool THIN, class EXTRA>
__device__ __forceinline__ ChunkCmd chunk_decode(const VgxFlattenArgs& A, DrawWindow& W, uint64_t& wbase, uint64_t d0, uint64_t d1, uint64_t C1, uint64_t chunk, uint64_t dcur, int lane, EXTRA extra)
{
	const VgxPathSetDev& ps = A.ps;
	const uint64_t ci = chunk + lane;
	const bool valid = ci < C1;
	const uint64_t lastKey = chunk + (VGX_WAVE - 1);
	if (!(wave_bcast_u64(W.prefix, VGX_WAVE - 1) > lastKey) || (REFILL_BEHIND && dcur < wbase)) {
		wbase = dcur;
		W = draw_window_load(A, wbase, lane);
	}
	const bool windowCovers = wave_bcast_u64(W.prefix, VGX_WAVE - 1) > lastKey;
	// owner = last window entry <= my key, searched on 32-bit offsets relative to the chunk start
	const uint32_t wrel = window_rel(W.prefix, chunk);
	const int ownerOfs = window_owner_rel(wrel, valid ? (uint32_t)lane : 0u);
	const uint32_t orel = (uint32_t)__shfl((int)wrel, ownerOfs);
	const int firstOwner = __popcll(wave_ballot(W.prefix <= chunk)) - 1; // draw that owns the chunk's first command
	ChunkCmd D;
	D.ownerBase = orel > 0 ? chunk + orel : wave_bcast_u64(W.prefix, firstOwner < 0 ? 0 : firstOwner);
	uint32_t pc0 = (uint32_t)__shfl((int)(W.pc0 | ((W.serial & 1u) << 31)), ownerOfs);
	D.serialStatic = pc0 >> 31;
	pc0 &= 0x7FFFFFFFu;
	uint32_t thinPath = THIN ? ((uint32_t)__shfl((int)W.serial, ownerOfs) >> 1) & 1u : 0u;
	D.d = d0; D.dr = A.draws; D.recIndex = 0; D.drawHead = false; D.drawLast = false; D.scale = 1.0f; D.tol = 0.25f; D.fillFlags = 0; D.strokeFlags = 0;
	D.rec.type = VGX_CMD_CLOSE; D.rec.flags = 0; D.rec.na = 0; D.rec.arg_off = 0; D.rec.start[0] = 0.0f; D.rec.start[1] = 0.0f;
	for (int i = 0; i < 8; ++i) { D.rec.a[i] = 0.0f; }
	if (valid) {
		if (windowCovers) {
			D.d = wbase + (uint64_t)ownerOfs;
		} else { // more than 63 draws begin inside this chunk (1-command or empty paths)
			D.d = find_owner_u64(A.cmd_prefix, d0, d1, ci);
			D.ownerBase = A.cmd_prefix[D.d];
			const uint32_t path = A.draws[D.d].path;
			pc0 = ps.path_cmd_begin[path];
			D.serialStatic = ps.path_flags[path] & VGX_PF_SERIAL;
			if (THIN) { thinPath = (ps.path_flags[path] >> 1) & 1u; }
		}
		D.dr = A.draws + D.d;
		const uint32_t k = (uint32_t)(ci - D.ownerBase);
		D.recIndex = pc0 + k;
		if (THIN && thinPath) {
			// my record, the one in front (its point = my start point) and, in front of a CLOSE, the one behind (the
			// sub-path's first point): neighbours of a 1 KB run the wave reads anyway
			const VgxCmdThin t0 = ps.cmdthin[pc0 + k];
			const VgxCmdThin tp = ps.cmdthin[(long long)(pc0 + k) - 1]; // (command 0 of the set reads the padding record; a path's first command never uses it)
			D.rec.type = t0.meta & 0xFFu; D.rec.flags = (t0.meta >> 8) & 0xFFu;
			D.rec.na = D.rec.type == VGX_CMD_CLOSE ? 0u : 2u;
			D.rec.start[0] = tp.x; D.rec.start[1] = tp.y;
			if (D.rec.type == VGX_CMD_CLOSE) { D.rec.a[6] = t0.x; D.rec.a[7] = t0.y; }
			else {
				D.rec.a[0] = t0.x; D.rec.a[1] = t0.y;
				if (D.rec.flags & VGX_CF_NEXT_IS_CLOSE) { const VgxCmdThin tn = ps.cmdthin[pc0 + k + 1]; D.rec.a[6] = tn.x; D.rec.a[7] = tn.y; }
			}
		} else {
			D.rec = ps.cmdrec[pc0 + k]; // one 64-byte record
		}
		D.drawHead = (k == 0);
		D.drawLast = (D.rec.flags & VGX_CF_LAST_IN_PATH) != 0;
		D.scale = D.dr->scale; D.tol = D.dr->tess_tol;
		D.fillFlags = D.dr->fill_flags; D.strokeFlags = D.dr->stroke_flags;
		extra(D);
	}
	return D;
}

// ---- per-command counts ----------------------------------------------------------------------------------------------
// The cubic of a CUBIC_TO / QUAD_TO command (the cubic walks themselves differ per kernel on purpose and stay there).
__device__ __forceinline__ void cubic_setup(bool quad, V2 start, const float* a, float* c1x, float* c1y, float* c2x, float* c2y, float* ex, float* ey)
{
	*c1x = a[0]; *c1y = a[1]; *c2x = a[2]; *c2y = a[3]; *ex = a[4]; *ey = a[5];
	if (quad) {
		*ex = a[2]; *ey = a[3];
		vgx_quad_to_cubic(start.x, start.y, a[0], a[1], *ex, *ey, c1x, c1y, c2x, c2y);
	}
}

// Nominal end point of a command that adds vertices (the vertex a following CLOSE may pop).
//   GUARD_EMPTY  an argument-less POLYLINE reads nothing. Set by k_flat1, which evaluates this for every valid lane;
//                k_flatten_build only behind limit > 0.
template<bool GUARD_EMPTY>
__device__ __forceinline__ V2 cmd_end_point(uint32_t type, const float* a, const float* pa, uint32_t na)
{
	return (type == VGX_CMD_POLYLINE) ? ((!GUARD_EMPTY || na >= 2) ? v2(pa[na - 2], pa[na - 1]) : v2(0.0f, 0.0f)) : (type == VGX_CMD_CUBIC_TO ? v2(a[4], a[5]) : (type == VGX_CMD_QUAD_TO ? v2(a[2], a[3]) : v2(a[0], a[1])));
}

struct ChunkCount { int cnt; bool slow, exists; };

// Vertices of a MOVE_TO / LINE_TO (point `pt`) / POLYLINE command; `slow`: pathAddVertex's epsilon test dropped one, so the
// last vertex is not the command's nominal end point. Cubics are counted by the kernel's walk, CLOSE by chunk_book.
__device__ __forceinline__ ChunkCount chunk_count_plain(uint32_t type, V2 start, V2 pt, const float* pa, uint32_t na)
{
	ChunkCount r;
	r.cnt = 0; r.slow = false; r.exists = false;
	switch (type) {
	case VGX_CMD_MOVE_TO: r.cnt = 1; r.exists = true; break;
	case VGX_CMD_LINE_TO: r.cnt = 1; r.slow = v2near(start, pt); break;
	case VGX_CMD_POLYLINE: {
		const uint32_t npts = na >> 1;
		r.cnt = (int)npts - ((npts > 0 && v2near(start, v2(pa[0], pa[1]))) ? 1 : 0);
		r.slow = r.cnt == 0; // a fully de-duplicated polyline leaves the last vertex unchanged: not its nominal end point
	} break;
	default: break; // shapes / arcs only occur in serial paths (k_flatten_serial)
	}
	return r;
}

// ---- segmented bookkeeping + carries ------------------------------------------------------------------------------------
struct ChunkBook
{
	int cnt;             // my vertices; -1: a CLOSE that pops the previous vertex
	int cntAll;          // cnt, or a whole serial draw's vertices at its last command (SERIAL_TAILS)
	bool closedHere, pop, serialTail;
	int incl, excl;      // scan of cntAll over the chunk
	int inDrawBefore, spBefore, spTotal; // vertices of my draw / sub-path in front of me, of my sub-path including me
	int subsIncl, fillIncl, strokeIncl;  // sub-paths / fill meshes / stroke meshes of my draw up to and including me
	int headExists;      // my sub-path began with a MOVE_TO of a lane-parallel draw
	bool lastInSub, fillHere, strokeHere, slowDraw;
};

struct ChunkCarry // of the draw / sub-path that continues across 64-command chunks (wave-uniform)
{
	int drawVerts = 0, spVerts = 0, subs = 0, fill = 0, stroke = 0, slow = 0, spExists = 0;

	// Taken from the last valid lane; a draw end resets all, a sub-path end the sub-path's two. `dcur`: see chunk_decode.
	//   GUARD_EMPTY  a chunk without valid lanes leaves everything as it is. Set by k_flat1 only: it runs one chunk for
	//                a segment without commands; the other two never enter an empty chunk.
	template<bool GUARD_EMPTY>
	__device__ __forceinline__ void advance(const ChunkBook& B, const ChunkCmd& C, int nvalid, uint64_t* dcur)
	{
		if (GUARD_EMPTY && !(nvalid > 0)) { return; }
		const int L = nvalid - 1;
		const int lastIsDrawLast = wave_bcast((int)C.drawLast, L);
		const int lastIsSubLast = wave_bcast((int)((C.rec.flags & VGX_CF_LAST_IN_SUB) != 0), L);
		const int nDraw = wave_bcast(B.inDrawBefore + B.cntAll, L);
		const int nSp = wave_bcast(B.spTotal, L);
		const int nSubs = wave_bcast(B.subsIncl, L);
		const int nFill = wave_bcast(B.fillIncl, L);
		const int nStroke = wave_bcast(B.strokeIncl, L);
		const int nSlow = wave_bcast((int)B.slowDraw, L);
		const int nHeadExists = wave_bcast(B.headExists, L);
		drawVerts = lastIsDrawLast ? 0 : nDraw;
		subs = lastIsDrawLast ? 0 : nSubs;
		fill = lastIsDrawLast ? 0 : nFill;
		stroke = lastIsDrawLast ? 0 : nStroke;
		slow = lastIsDrawLast ? 0 : nSlow;
		spVerts = (lastIsDrawLast || lastIsSubLast) ? 0 : nSp;
		spExists = (lastIsDrawLast || lastIsSubLast) ? 0 : nHeadExists;
		*dcur = wave_bcast_u64(C.d, L); // draw of the last command: the next window (if needed) starts here
	}
};

// Both scans and everything they decide. `cnt / slow / exists`: the lane's count (0 / false for invalid lanes and lanes
// of serial draws); `closeNear`: a CLOSE's start point is its sub-path's first point within epsilon.
//   DECIDE_CLOSE  the first scan decides pathClose (path.cpp:707-726: closes a sub-path of more than 2 vertices, pops its
//                 last vertex when that repeats the first). Off in k_flatten<EMIT = true> only, which reads the count
//                 pass's decision back from cmd_cnt (`closedIn / popIn`, cnt = -1 for a pop).
//   HEAD_EXISTS   a sub-path counts only when its head lane exists (a MOVE_TO that was not part of a serial draw). Off in
//                 k_flatten_build only, which has no such term and no carry for it (NOTEBOOK.md).
//   SKIP_SERIAL   lanes of serial draws end no sub-path. Off in k_flatten only, whose lastInSub has no such term
//                 (its serial lanes never have an existing head: NOTEBOOK.md).
//   SERIAL_TAILS  the last command of a serial draw stands for the draw's `serialVerts` vertices in the scan. Set by k_flat1
//                 only: it places serial draws as opaque blocks inside the ordered output.
template<bool DECIDE_CLOSE, bool HEAD_EXISTS, bool SKIP_SERIAL, bool SERIAL_TAILS>
__device__ __forceinline__ ChunkBook chunk_book(const ChunkCarry& K, const ChunkCmd& C, bool valid, bool serialDraw, int cnt, bool slow, bool exists, bool closeNear, int lane,
	bool closedIn = false, bool popIn = false, int serialVerts = 0)
{
	ChunkBook B;
	const uint32_t cflags = C.rec.flags;
	B.closedHere = closedIn; B.pop = popIn;
	const uint64_t drawHeads = wave_ballot(valid && C.drawHead);
	const uint64_t subHeads = wave_ballot(valid && (cflags & VGX_CF_STARTS_SUB));
	const int dh = seg_head(drawHeads, lane);
	const int sh = seg_head(subHeads, lane);
	if (DECIDE_CLOSE) {
		// pathClose needs the vertex count of its sub-path so far
		const int incl1 = wave_incl_scan(cnt, lane);
		const int spBefore1 = seg_rel(incl1 - cnt, sh, K.spVerts);
		if (valid && !serialDraw && C.rec.type == VGX_CMD_CLOSE && spBefore1 > 2) {
			B.closedHere = true;
			if (closeNear) { B.pop = true; cnt = -1; } // the previous vertex is removed
		}
	}
	B.cnt = cnt;
	B.serialTail = SERIAL_TAILS && valid && serialDraw && C.drawLast;
	B.cntAll = B.serialTail ? serialVerts : cnt;
	B.incl = wave_incl_scan(B.cntAll, lane);
	B.excl = B.incl - B.cntAll;
	B.inDrawBefore = seg_rel(B.excl, dh, K.drawVerts);
	B.spBefore = seg_rel(B.excl, sh, K.spVerts);
	B.spTotal = B.spBefore + cnt; // vertices of my sub-path up to and including me

	const uint64_t existMask = wave_ballot(valid && exists);
	const uint64_t mine = seg_mask_upto(dh, lane);
	B.subsIncl = __popcll(existMask & mine) + (dh < 0 ? K.subs : 0);
	B.headExists = HEAD_EXISTS ? ((sh < 0) ? K.spExists : (int)((existMask >> sh) & 1ull)) : 1;
	B.lastInSub = valid && !(SKIP_SERIAL && serialDraw) && (cflags & VGX_CF_LAST_IN_SUB) && B.headExists;
	B.fillHere = B.lastInSub && (C.fillFlags & VGX_FILL_ENABLE) && B.spTotal >= 3;
	B.strokeHere = B.lastInSub && (C.strokeFlags & VGX_STROKE_ENABLE) && B.spTotal >= 2;
	const uint64_t fillMask = wave_ballot(B.fillHere);
	const uint64_t strokeMask = wave_ballot(B.strokeHere);
	B.fillIncl = __popcll(fillMask & mine) + (dh < 0 ? K.fill : 0);
	B.strokeIncl = __popcll(strokeMask & mine) + (dh < 0 ? K.stroke : 0);
	const uint64_t slowMask = wave_ballot(valid && slow);
	B.slowDraw = ((slowMask & mine) != 0) || (dh < 0 && K.slow);
	return B;
}

// ---- records ---------------------------------------------------------------------------------------------------------------
// Per-draw record written at the draw's last command. Slow form: a degenerate draw (epsilon de-dup hit / dropped piece),
// which k_flatten_serial redoes exactly. Places other than the first vertex are the caller's (0 here).
__device__ __forceinline__ vgx_draw_info draw_info_for(bool slowDraw, uint64_t firstVertex, int numVertices, int subsIncl, int fillIncl, int strokeIncl)
{
	vgx_draw_info di;
	di.first_poly_vertex = firstVertex; di.first_subpath = 0; di.first_mesh = 0;
	if (slowDraw) {
		di.num_poly_vertices = 0; di.num_subpaths = 0; di.num_meshes = 0;
		di.flags = 1u;
	} else {
		di.num_poly_vertices = (uint32_t)numVertices;
		di.num_subpaths = (uint32_t)subsIncl;
		di.num_meshes = (uint32_t)(fillIncl + strokeIncl);
		di.flags = ((uint32_t)fillIncl << 1);
	}
	return di;
}

// Draws k_flatten_serial has to (re)do: wave-aggregated append to serial_list. Returns whether any lane appended.
//   MARK_REDO  also raises flat_redo. Set by k_flat1 only: its second run is for batches in which the first listed a draw.
template<bool MARK_REDO>
__device__ __forceinline__ bool serial_list_append(VgxTotals* T, uint32_t* serialList, bool toSerial, uint64_t d, int lane)
{
	const uint64_t sm = wave_ballot(toSerial);
	if (sm) {
		unsigned long long sbase = 0;
		if (lane == 0) {
			sbase = atomicAdd(&T->num_serial_list, (unsigned long long)__popcll(sm));
			if (MARK_REDO) { T->flat_redo = 1u; }
		}
		sbase = wave_bcast_u64(sbase, 0);
		if (toSerial) { serialList[sbase + (uint64_t)__popcll(sm & lanemask_lt(lane))] = (uint32_t)d; }
	}
	return sm != 0;
}

} // namespace

#endif
