// vgx_dashframe.hip -- a frame with dashed strokes in one asynchronous call (vgx_tessellate_dashed, include/vgx.h): what runs between
// the flatten stage and the stroker's size pass, with no host in between. The slots are the arithmetic of vgx_dashframe.h.
//
//   scan over the source meshes  which of the flatten stage's mesh descriptors are stroke meshes of a dashed draw -> D(m), and the vertex
//                                list the dash pass cuts for each of them: the descriptor's own polyline, where the flatten route left it
//                                (every other mesh: an empty list, so list number = mesh number)                     (OpDashFrameLists)
//   vgx_launch_dash              the dash pass in its frame form (vgx_dash.hip): pieces into context scratch, BEHIND the flatten stage's
//                                heap in the same allocation, so that the size pass and the emit kernels read one polyline
//   k_dashframe_join             one thread: the two verdicts become the call's, the frame's mesh count, the need for the host's mirror
//   k_dashframe_place            one lane per OUTPUT mesh, whatever a draw owns: lanes [0, M) take the source meshes (a kept one is copied
//                                to its slot -- descriptor, constants, closed-form size: nothing is recomputed, its polyline stays where it
//                                is), lanes [0, Np) the pieces (descriptor of an open list with the draw's stroke fields, as the stroker-level
//                                entry writes it). No lane loops over a draw's pieces: a 100 000-piece draw is 100 000 lanes.
// The exact serial builder's draws (ARC / shape paths, degenerate input) need nothing of their own: k_flatten_serial has written their
// descriptors into the same ordered table before any of this runs, and a dashed one is cut from the polyline that descriptor names.
#include "vgx_internal.h"
#include "vgx_scan.h"
#include "vgx_pathsim.h"
#include "vgx_dashframe.h"

namespace {

__device__ __forceinline__ uint32_t df_status(const VgxTotals* t) { return __hip_atomic_load(&t->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool df_is_dashed(const VgxDashFrameArgs& A, const VgxMeshDesc& md)
{
	return VGX_MD_KIND(md.kind) >= VGX_MESH_STROKE && A.dashes[md.draw].count != 0u;
}

struct OpDashFrameLists // dashed stroke meshes in front of every source mesh -> D(m); the lists of the dash pass
{
	VgxDashFrameArgs A;
	__device__ uint64_t size() const { return A.totals->status == VGX_OK ? A.totals->sizes.num_meshes : 0ull; }
	__device__ Sum3 load(uint64_t m) const
	{
		Sum3 r = sum3_zero();
		r.a = df_is_dashed(A, A.mdesc[m]) ? 1u : 0u;
		return r;
	}
	__device__ void store(uint64_t m, Sum3 e) const
	{
		const VgxMeshDesc md = A.mdesc[m];
		vgx_subpath sp;
		sp.first_vertex = 0; sp.num_vertices = 0; sp.flags = 0;
		if (df_is_dashed(A, md)) { sp.first_vertex = md.poly_first; sp.num_vertices = md.poly_n; sp.flags = VGX_MD_CLOSED(md.kind); }
		A.lists[m] = sp;
		A.list_draw[m] = md.draw;
		A.dashed_before[m] = e.a;
	}
	__device__ void finish(Sum3 t) const
	{
		const uint64_t n = size();
		A.dashed_before[n] = t.a;
		*A.nlists = n;
	}
};

// One thread, behind the dash pass. Verdicts: a broken dash record / pattern entry (VGX_E_INVALID_ARG) or a list out of range (VGX_E_RANGE)
// ends the call whatever the flatten stage said -- calling again would not help; a flatten stage that outgrew the context keeps its own
// verdict (k_imm_publish makes it VGX_E_GROWN); pieces or frame meshes that outgrew the context: VGX_E_GROWN, the need to the mirror.
__global__ void k_dashframe_join(VgxDashFrameArgs A)
{
	VgxTotals* T = A.totals;
	const VgxTotals* D = A.dash_totals;
	const uint32_t st = df_status(T), ds = df_status(D);
	const bool counted = ds == (uint32_t)VGX_OK || ds == (uint32_t)VGX_E_NOSPACE; // (k_dash_ranges wrote the totals)
	const uint64_t pieces = counted ? D->sizes.num_subpaths : 0ull, verts = counted ? D->sizes.num_poly_vertices : 0ull;
	const uint64_t M = *A.nlists;
	A.need[0] = pieces; A.need[1] = verts; A.need[2] = M; A.need[3] = (st == (uint32_t)VGX_OK && counted) ? 1ull : 0ull;
	if (ds != (uint32_t)VGX_OK && ds != (uint32_t)VGX_E_NOSPACE && ds != (uint32_t)VGX_E_GROWN) {
		T->status = ds;
		T->scratch_short = 0u;
	} else if (st == (uint32_t)VGX_OK) {
		const uint64_t frame = vgx_df_num_meshes(M, A.dashed_before[M], pieces);
		if (ds != (uint32_t)VGX_OK || frame > A.cap_meshes) { T->status = VGX_E_GROWN; }
		else { T->sizes.num_meshes = frame; }
	}
	if (A.dev_dash_sizes) {
		vgx_sizes z;
		z.num_poly_vertices = verts; z.num_subpaths = pieces;
		z.num_meshes = 0; z.num_vertices = 0; z.num_indices = 0; z.num_serial_draws = 0; z.num_cmd_instances = 0; z.num_elements = 0; z.num_fill_elements = 0; z.num_drawcmds = 0;
		*A.dev_dash_sizes = z;
	}
}

__global__ __launch_bounds__(256) void k_dashframe_place(VgxDashFrameArgs A)
{
	if (A.totals->status != VGX_OK) { return; } // (the last writer, k_dashframe_join, ran before this launch)
	const uint64_t M = *A.nlists, np = A.dash_totals->sizes.num_subpaths;
	const uint64_t n = M > np ? M : np, stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		if (i < M) { // source mesh i: kept ones move to their slot as they are
			const VgxMeshDesc md = A.mdesc[i];
			if (!df_is_dashed(A, md)) {
				const uint64_t db = A.dashed_before[i];
				const uint64_t slot = vgx_df_slot_kept(i, db, db ? vgx_df_pieces_before(A.piece_src, np, i) : 0ull);
				A.mdesc2[slot] = md; A.mtab2[slot] = A.mtab[i]; A.mprep2[slot] = A.mprep[i];
			}
		}
		if (i < np) { // piece i: an open list stroked with its draw's fields; the sub-path index is the source's
			const uint32_t m = A.piece_src[i];
			const vgx_subpath sp = A.piece_subs[i];
			const VgxMeshDesc md = A.mdesc[m];
			const uint64_t slot = vgx_df_slot_piece(m, A.dashed_before[m], i);
			if (vgx_write_mesh(A.mdesc2, A.mtab2, slot, A.draws + md.draw, md.draw, md.subpath, VGX_MD_KIND(md.kind), false, A.piece_base + sp.first_vertex, sp.num_vertices, A.mprep2, nullptr)) {
				atomicAdd(&A.totals->num_round_meshes, 1u);
			}
		}
	}
}

} // namespace

void vgx_launch_dashframe_lists(const VgxDashFrameArgs& a, hipStream_t s)
{
	OpDashFrameLists op; op.A = a;
	vgx_device_scan(op, a.partial, s, a.cap_meshes);
}

void vgx_launch_dashframe_place(const VgxDashFrameArgs& a, hipStream_t s)
{
	hipLaunchKernelGGL(k_dashframe_join, dim3(1), dim3(1), 0, s, a);
	hipLaunchKernelGGL(k_dashframe_place, dim3(2048), dim3(256), 0, s, a);
}
