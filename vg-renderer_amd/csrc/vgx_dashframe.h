// vgx_dashframe.h -- where every mesh of a frame with dashed strokes lies (vgx_tessellate_dashed, include/vgx.h). Host + device, so
// that the arithmetic is unit-tested on the CPU (csrc/vgx_hosttest.cpp: vgxt_dashframe_ranks); vgx_dashframe.hip distributes it.
//
// Two inputs, each sorted by draw:
//   the SOURCE meshes m = 0 .. M-1 the flatten stage describes, in frame order (per draw: fills by sub-path, strokes by sub-path);
//     some of them are "dashed": stroke meshes of a draw whose dash record has count > 0. They produce no mesh themselves;
//   the PIECES p = 0 .. Np-1 the dash pass cut from the dashed source meshes, in source order: src[p] = the source mesh, non-decreasing.
// Frame order: every source mesh that is kept stays where it was among the kept ones, and the pieces of a dashed source mesh take that
// mesh's place, by increasing start. With
//   D(m) = dashed source meshes in front of m     (an exclusive scan over the source meshes)
//   B(m) = pieces cut from source meshes < m      (a search in src[]: the pieces are sorted by source)
// the slots are closed-form:
//   kept source mesh m          -> m - D(m) + B(m)
//   piece p of source mesh m    -> m - D(m) + p          (B(m) + its number among m's pieces = p)
//   meshes of the frame          = M - D(M) + Np
// A dashed mesh without pieces (no "on" length, a pattern coarser than the list) simply takes no slot.
#ifndef VGX_DASHFRAME_H
#define VGX_DASHFRAME_H

#include <stdint.h>
#include "vgx_lane.h"

// pieces whose source mesh is < m: the first p with src[p] >= m
VGX_HD uint64_t vgx_df_pieces_before(const uint32_t* src, uint64_t npieces, uint64_t m)
{
	uint64_t lo = 0, hi = npieces;
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);
		if (src[mid] < m) { lo = mid + 1; } else { hi = mid; }
	}
	return lo;
}

VGX_HD uint64_t vgx_df_slot_kept(uint64_t m, uint64_t dashedBefore, uint64_t piecesBefore) { return m - dashedBefore + piecesBefore; }
VGX_HD uint64_t vgx_df_slot_piece(uint64_t m, uint64_t dashedBefore, uint64_t p) { return m - dashedBefore + p; }
VGX_HD uint64_t vgx_df_num_meshes(uint64_t nsource, uint64_t ndashed, uint64_t npieces) { return nsource - ndashed + npieces; }

#endif
