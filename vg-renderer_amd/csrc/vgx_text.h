// vgx_text.h -- the arithmetic of renderTextQuads (reference src/vg.cpp:5541-5621) for ONE run and ONE quad: host + device.
// The kernel of vgx_text.hip runs it one quad per lane; libvgx_hosttest.so (vgx_hosttest.cpp) runs the same functions quad after
// quad so that the CPU suite pins the arithmetic against the reference's own loops without a GPU.
//
// What the reference does with the glyph quads FontStash produced (ctxText, vg.cpp:4177-4232):
//   pushState; transformTranslate(x + dx / scale, y + dy / scale)   (:4228-4229, 4055-4062)
//   renderTextQuads: mtx[0..3] = m[0..3] * (1.0f / scale), mtx[4..5] = m[4..5]   (:5545-5558)
//     vgutil::batchTransformTextQuads: corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) through transformPos2D  (vg_util.cpp:332-445, vg_util.h:24-28)
//     the colour four times per quad (memset32, :5575), UVs (s0,t0) (s1,t0) (s1,t1) (s0,t1) as int16 or float (:5577-5613),
//     vgutil::genQuadIndices_unaligned: b, b+1, b+2, b, b+2, b+3 with b = 4 * quad (vg_util.cpp:275-330)
//   popState
#ifndef VGX_TEXT_H
#define VGX_TEXT_H

#include "vgx_lane.h"

#define VGX_TEXT_MAX_QUADS 16384u // 4 * 16384 = 65536 vertices: the most a draw command holds (vg.cpp:5323), uint16 indices

VGX_HD bool vgx_text_finite(float v)
{
	union { float f; uint32_t u; } c; c.f = v;
	return (c.u & 0x7F800000u) != 0x7F800000u;
}

// The matrix batchTransformTextQuads gets for a run. Returns false when the scale or a resulting term is not finite (scale 0 included).
VGX_HD bool vgx_text_run_matrix(const vgx_text_run& r, float* m)
{
	const float tx = r.x + r.dx / r.scale;
	const float ty = r.y + r.dy / r.scale;
	const float m4 = r.mtx[4] + (r.mtx[0] * tx + r.mtx[2] * ty); // m[4] += m[0] * x + m[2] * y
	const float m5 = r.mtx[5] + (r.mtx[1] * tx + r.mtx[3] * ty);
	const float inv = 1.0f / r.scale;
	m[0] = r.mtx[0] * inv;
	m[1] = r.mtx[1] * inv;
	m[2] = r.mtx[2] * inv;
	m[3] = r.mtx[3] * inv;
	m[4] = m4;
	m[5] = m5;
	return vgx_text_finite(r.scale) && vgx_text_finite(m[0]) && vgx_text_finite(m[1]) && vgx_text_finite(m[2]) && vgx_text_finite(m[3])
		&& vgx_text_finite(m[4]) && vgx_text_finite(m[5]);
}

// VGX_OK, or why the run writes nothing: more quads than a draw command holds / a non-finite matrix
VGX_HD int vgx_text_run_status(const vgx_text_run& r, float* m)
{
	const bool finite = vgx_text_run_matrix(r, m);
	if (r.num_quads > VGX_TEXT_MAX_QUADS) { return VGX_E_MESH_TOO_LARGE; }
	return finite ? VGX_OK : VGX_E_NONFINITE;
}

// the run's places against the capacities (overflow-safe; num_quads <= VGX_TEXT_MAX_QUADS)
VGX_HD bool vgx_text_run_fits(const vgx_text_run& r, uint64_t capVertices, uint64_t capIndices)
{
	const uint64_t nv = 4ull * r.num_quads, ni = 6ull * r.num_quads;
	return r.first_vertex <= capVertices && nv <= capVertices - r.first_vertex && r.first_index <= capIndices && ni <= capIndices - r.first_index;
}

VGX_HD vgx_mesh vgx_text_run_mesh(const vgx_text_run& r, bool ok)
{
	vgx_mesh m;
	m.first_vertex = r.first_vertex; m.first_index = r.first_index;
	m.num_vertices = ok ? 4u * r.num_quads : 0u; m.num_indices = ok ? 6u * r.num_quads : 0u;
	m.draw = r.draw; m.subpath_kind = (uint32_t)VGX_MESH_TEXT << 28;
	return m;
}

// transformPos2D (vg_util.h:24-28) of the four corners of q = {x0, y0, x1, y1, ...}
VGX_HD void vgx_text_quad_pos(const float* q, const float* m, float* p)
{
	const float x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3];
	p[0] = m[0] * x0 + m[2] * y0 + m[4]; p[1] = m[1] * x0 + m[3] * y0 + m[5];
	p[2] = m[0] * x1 + m[2] * y0 + m[4]; p[3] = m[1] * x1 + m[3] * y0 + m[5];
	p[4] = m[0] * x1 + m[2] * y1 + m[4]; p[5] = m[1] * x1 + m[3] * y1 + m[5];
	p[6] = m[0] * x0 + m[2] * y1 + m[4]; p[7] = m[1] * x0 + m[3] * y1 + m[5];
}

// (int16_t)(s * INT16_MAX), (int16_t)(t * INT16_MAX) packed as the vertex's UV word (vg.cpp:5587-5590); truncation towards zero
VGX_HD uint32_t vgx_text_uv16(float s, float t)
{
	const uint32_t us = (uint32_t)(uint16_t)(int16_t)(int32_t)(s * 32767.0f);
	const uint32_t ut = (uint32_t)(uint16_t)(int16_t)(int32_t)(t * 32767.0f);
	return us | (ut << 16);
}
// the four UV words of q = {..., s0, t0, s1, t1}: (s0,t0) (s1,t0) (s1,t1) (s0,t1)
VGX_HD void vgx_text_quad_uv16(const float* q, uint32_t* uv)
{
	uv[0] = vgx_text_uv16(q[4], q[5]); uv[1] = vgx_text_uv16(q[6], q[5]);
	uv[2] = vgx_text_uv16(q[6], q[7]); uv[3] = vgx_text_uv16(q[4], q[7]);
}
VGX_HD void vgx_text_quad_uvf(const float* q, float* uv)
{
	uv[0] = q[4]; uv[1] = q[5]; uv[2] = q[6]; uv[3] = q[5];
	uv[4] = q[6]; uv[5] = q[7]; uv[6] = q[4]; uv[7] = q[7];
}

// genQuadIndices_unaligned for quad `local` of its run (firstVertexID 0: indices are mesh-local)
VGX_HD void vgx_text_quad_idx(uint32_t local, uint16_t* idx)
{
	const uint16_t b = (uint16_t)(4u * local);
	idx[0] = b; idx[1] = (uint16_t)(b + 1); idx[2] = (uint16_t)(b + 2);
	idx[3] = b; idx[4] = (uint16_t)(b + 2); idx[5] = (uint16_t)(b + 3);
}

#endif
