/*
 * vgx.h -- C-ABI of the MI355X-native batch geometry path (libvgx.so).
 *
 * This is the drop-in boundary for vg-renderer's CPU geometry hot path:
 *   vg::Path     bezier flattener        (reference include/vg/path.h:19-38,    src/path.cpp)
 *   vg::Stroker  stroke/fill/AA mesher   (reference include/vg/stroker.h:11-85, src/stroker.cpp)
 * The reference calls those once per path per frame (src/vg.cpp:2969-3059, 3061-3179, 3401-3492);
 * this ABI takes MANY path instances ("draws") at once so that one launch sequence on a gfx950
 * device does the work of millions of pathXXX/strokerXXX calls. Everything is plain pointers and
 * sizes; no C++ or torch types cross the boundary. The C++ header include/vgx_compat.hpp layers the
 * reference's own vg::pathXXX / vg::strokerXXX names on top of this ABI.
 *
 * Conventions
 *   - "host" pointers are ordinary CPU memory, "device" pointers are HIP device memory on the
 *     context's device. Each parameter says which one it is.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). Calls are asynchronous
 *     unless they return data to the host (documented per function).
 *   - All functions return a vgx_status; they never abort and never print.
 *   - Numeric contract: IEEE binary32, no FMA contraction, transcendentals from csrc/vgmath.h.
 *     Indices are mesh-local uint16 (reference vg::Mesh, include/vg/vg.h:353-360), colours are
 *     uint32 0xAABBGGRR (include/vg/vg.h:80-86).
 */
#ifndef VGX_H
#define VGX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGX_VERSION 1

typedef enum vgx_status {
	VGX_OK = 0,
	VGX_E_INVALID_ARG = 1,   /* null pointer, bad enum, count out of range */
	VGX_E_INVALID_PATH = 2,  /* command stream violates the path grammar (see vgx_pathset_create) */
	VGX_E_NONFINITE = 3,     /* NaN/Inf in path arguments (would hang the reference, path.cpp:109), or a draw whose
	                          * scale / tess_tol / fringe / stroke_width / mtx is NaN, Inf, negative, or scale, tess_tol <= 0,
	                          * or tess_tol / scale^2 < 1e-12 (checked on the device, reported in the status word) */
	VGX_E_NOSPACE = 4,       /* caller-provided output capacity too small; vgx_sizes holds the need */
	VGX_E_MESH_TOO_LARGE = 5,/* a mesh needs > 65536 vertices (uint16 indices, vg.cpp:734) */
	VGX_E_HIP = 6,           /* a HIP runtime call failed; vgx_last_hip_error() has the code */
	VGX_E_NO_DEVICE = 7,     /* no gfx950 device / HIP runtime unavailable */
	VGX_E_RANGE = 8,         /* batch exceeds 2^32-1 polyline vertices or commands; split the batch */
	VGX_E_INTERNAL = 9,      /* device-side protocol error (a wait inside the single-pass kernel timed out): a bug, report it */
	VGX_E_STALE = 10,        /* vgx_tessellate: the draws no longer have the structure the last vgx_tessellate_count found (template
	                          * mode, see vgx_tessellate): a field other than mtx / colours / state_key of some draw differs from the
	                          * counted batch. Outputs are undefined; call vgx_tessellate_count on the new draws */
	VGX_E_GROWN = 11         /* vgx_tessellate_immediate (dev_status): the batch outgrew a scratch table of the context. Nothing was written past
	                          * any table; the need went to the context, the next immediate call grows its scratch first: call again */
} vgx_status;

/* Path commands. One opcode per vg::pathXXX builder call (reference include/vg/path.h:24-35).
 * Arguments are float32, in the order of the reference's function parameters. */
typedef enum vgx_cmd {
	VGX_CMD_MOVE_TO = 0,   /* x, y                     pathMoveTo       path.cpp:62-78   */
	VGX_CMD_LINE_TO = 1,   /* x, y                     pathLineTo       path.cpp:80-84   */
	VGX_CMD_CUBIC_TO = 2,  /* c1x,c1y,c2x,c2y,x,y      pathCubicTo      path.cpp:86-182  */
	VGX_CMD_QUAD_TO = 3,   /* cx,cy,x,y                pathQuadraticTo  path.cpp:184-201 */
	VGX_CMD_CLOSE = 4,     /* -                        pathClose        path.cpp:707-726 */
	VGX_CMD_ARC_TO = 5,    /* x1,y1,x2,y2,r            pathArcTo        path.cpp:203-273 */
	VGX_CMD_ARC = 6,       /* cx,cy,r,a0,a1,dir(0|1)   pathArc          path.cpp:633-682 */
	VGX_CMD_RECT = 7,      /* x,y,w,h                  pathRect         path.cpp:275-286 */
	VGX_CMD_ROUNDED_RECT = 8,         /* x,y,w,h,r     pathRoundedRect  path.cpp:288-409 */
	VGX_CMD_ROUNDED_RECT_VARYING = 9, /* x,y,w,h,rtl,rtr,rbr,rbl        path.cpp:411-559 */
	VGX_CMD_CIRCLE = 10,   /* cx,cy,r                  pathCircle       path.cpp:561-597 */
	VGX_CMD_ELLIPSE = 11,  /* cx,cy,rx,ry              pathEllipse      path.cpp:599-631 */
	VGX_CMD_POLYLINE = 12, /* x0,y0,...,xn-1,yn-1      pathPolyline     path.cpp:684-705 */
	VGX_CMD_COUNT_ = 13
} vgx_cmd;

/* Values are the reference's vg::LineCap / vg::LineJoin (include/vg/vg.h:156-174); they are ABI. */
enum { VGX_CAP_BUTT = 0, VGX_CAP_ROUND = 1, VGX_CAP_SQUARE = 2 };
enum { VGX_JOIN_MITER = 0, VGX_JOIN_ROUND = 1, VGX_JOIN_BEVEL = 2 };

/* vgx_draw.fill_flags */
#define VGX_FILL_ENABLE 0x1u /* strokerConvexFill / strokerConvexFillAA per sub-path (vg.cpp:3099-3131) */
#define VGX_FILL_AA 0x2u
/* Index ORDER of strokerConvexFillAA meshes as the reference's default x86 build writes it (the SSE2 variant,
 * stroker.cpp:610-701: first fringe quad, then per fan triangle the triangle followed by the next edge's fringe quad, last
 * quad) instead of the scalar variant's (all fan triangles, then all fringe quads, stroker.cpp:769-795). Same triangles,
 * same counts, same vertices; for callers that compare index streams with an SSE build of the reference. Positions stay
 * the scalar build's (the SSE variant computes them with rcpps / rsqrtps approximations). */
#define VGX_FILL_INDEX_ORDER_SSE 0x100u
/* PathType::Concave fills (VG_FILL_FLAGS, include/vg/vg.h:229; ctxFillPath* src/vg.cpp:3133-3178): a draw with VGX_FILL_CONCAVE and
 * WITHOUT VGX_FILL_ENABLE produces no mesh in vgx_tessellate. Two routes build it and vgx_merge puts it at the draw's place in the
 * frame: triangles, as the reference makes them -- vgx_flatten_* (contours) + libtess2 on the CPU side of the caller + vgx_concave_move
 * / vgx_concave_emit --, or, for a frame that goes to vgx_raster_concave, contour meshes without libtess2 and without leaving the
 * device -- vgx_flatten + vgx_concave_contours; vgx_concave_triangulate is that call with triangles, made on the device, for the draws
 * that are one simple ring. vgx_cmdlist_decode emits concave FillPath* commands as such draws (VGX_FILL_AA / VGX_FILL_EVEN_ODD say
 * which strokerConcaveFillEnd[AA] call and FillRule the reference would use). */
#define VGX_FILL_CONCAVE 0x10u
#define VGX_FILL_EVEN_ODD 0x20u
/* A user mesh (vg::indexedTriList, src/vg.cpp:4129-4175): the draw has no path and no GPU mesh; vgx_cmdlist_decode hands the mesh
 * itself over in vgx_cmdlist_out::tri_* (positions already through the state transform, as ctxIndexedTriList does with
 * batchTransformPositions) and vgx_merge puts it at the draw's place in the frame. */
#define VGX_FILL_TRILIST 0x40u
/* A Text / TextBox command (vg::text, vg::textBox; ctxText src/vg.cpp:4177-4232): the draw has no path and no mesh from
 * vgx_tessellate; vgx_cmdlist_decode_text hands the command over as a vgx_text_cmd, the caller's FontStash makes the glyph quads,
 * vgx_text_quads makes the mesh(es) and vgx_merge_uv puts them at the draw's place in the frame. */
#define VGX_FILL_TEXT 0x80u
/* vgx_draw.stroke_flags */
#define VGX_STROKE_ENABLE 0x1u
#define VGX_STROKE_AA 0x2u
#define VGX_STROKE_THIN 0x4u /* strokerPolylineStrokeAAThin (vg.cpp:3417, 3464-3466); needs AA */
#define VGX_STROKE_CAP(flags) (((flags) >> 4) & 0x3u)
#define VGX_STROKE_JOIN(flags) (((flags) >> 6) & 0x3u)
#define VGX_STROKE_FLAGS(cap, join, aa, thin) \
	(VGX_STROKE_ENABLE | ((aa) ? VGX_STROKE_AA : 0u) | ((thin) ? VGX_STROKE_THIN : 0u) | ((uint32_t)(cap) << 4) | ((uint32_t)(join) << 6))

/* One path instance: what the reference does between vg::beginPath and vg::fillPath/strokePath for
 * one path under one state transform (vg.cpp:2969-2981 pathReset+strokerReset, vg.cpp:4957-4975
 * transformPath, vg.cpp:3061-3179 / 3401-3492 the stroker calls). 64 bytes, 16 dwords. */
typedef struct vgx_draw {
	uint32_t path;         /* index into the path set */
	uint32_t fill_flags;   /* VGX_FILL_* */
	uint32_t fill_color;   /* colour handed to strokerConvexFillAA */
	uint32_t stroke_flags; /* VGX_STROKE_* */
	uint32_t stroke_color; /* colour handed to strokerPolylineStrokeAA[Thin] */
	float stroke_width;    /* strokeWidth handed to strokerPolylineStroke[AA] (already scaled/clamped) */
	float scale;           /* pathReset/strokerReset scale (State::m_AvgScale) */
	float tess_tol;        /* tesselationTolerance (Context::m_TesselationTolerance) */
	float fringe;          /* fringeWidth (Context::m_FringeWidth) */
	float mtx[6];          /* 2x3 state transform [m0 m2 m4; m1 m3 m5] used by transformPath */
	uint32_t state_key;    /* draw-command assembly only (VGX_ASM_SPLIT_STATE): what allocDrawCommand / allocClipCommand compare
	                        * before merging a mesh into the previous command (vg.cpp:5376-5379, 5418-5428), folded by the host
	                        * into one word: DrawCommand::m_Type << 16 | m_HandleID in the low 20 bits, and above them a
	                        * generation the host bumps whenever it would set m_ForceNewDrawCommand / m_ForceNewClipCommand
	                        * (beginClip / endClip / resetClip / scissor changes, vg.cpp:3682-4026). 0 everywhere = one draw state */
} vgx_draw;

/* Path definitions ("path set"), host-side description handed to vgx_pathset_create.
 * cmd_arg_off has ncmd+1 entries: command k owns args[cmd_arg_off[k] .. cmd_arg_off[k+1]).
 * path p owns commands [path_cmd_begin[p], path_cmd_begin[p+1]). */
typedef struct vgx_pathset_desc {
	const uint8_t* cmd_type;        /* [ncmd]   vgx_cmd */
	const uint32_t* cmd_arg_off;    /* [ncmd+1] */
	const float* args;              /* [cmd_arg_off[ncmd]] */
	const uint32_t* path_cmd_begin; /* [npaths+1] */
	uint32_t npaths;
	uint32_t ncmd;
} vgx_pathset_desc;

/* vg::SubPath (include/vg/path.h:11-16) with batch-global addressing. 16 bytes. */
typedef struct vgx_subpath {
	uint64_t first_vertex; /* index into the batch's polyline vertex array */
	uint32_t num_vertices;
	uint32_t flags;        /* bit0 = isClosed */
} vgx_subpath;

/* Where one draw's data lives in the flatten output. 40 bytes. */
typedef struct vgx_draw_info {
	uint64_t first_poly_vertex;
	uint64_t first_subpath;
	uint64_t first_mesh;
	uint32_t num_poly_vertices; /* pathGetNumVertices */
	uint32_t num_subpaths;      /* pathGetNumSubPaths */
	uint32_t num_meshes;
	uint32_t flags;             /* bit0: went through the serial (exact, slow) lane path */
} vgx_draw_info;

/* vg::Mesh (include/vg/vg.h:353-360) with batch-global addressing. 32 bytes.
 * Meshes of a draw appear in the reference's call order: fill meshes by sub-path, then stroke
 * meshes by sub-path. Indices are mesh-local. */
typedef struct vgx_mesh {
	uint64_t first_vertex; /* into pos / color streams */
	uint64_t first_index;  /* into idx stream */
	uint32_t num_vertices;
	uint32_t num_indices;
	uint32_t draw;
	uint32_t subpath_kind; /* bits 0-27 sub-path index within the draw, bits 28-31 VGX_MESH_* */
} vgx_mesh;
enum { VGX_MESH_FILL = 0, VGX_MESH_FILL_AA = 1, VGX_MESH_STROKE = 2, VGX_MESH_STROKE_AA = 3, VGX_MESH_STROKE_AA_THIN = 4,
       VGX_MESH_CONCAVE_FILL_AA = 5 /* vgx_concave_emit */, VGX_MESH_TRILIST = 6 /* vgx_cmdlist_out::tri_meshes */,
       VGX_MESH_TEXT = 7 /* vgx_text_quads */, VGX_MESH_CONTOURS = 8 /* vgx_concave_contours: directed edges, below */ };
/* A mesh of kind VGX_MESH_CONTOURS holds the contours of a concave fill as an edge soup, for a consumer that fills by winding number
 * (vgx_raster_concave draws it, vgx_pick_frame hit-tests it by the same rule). Vertices are contour points in pos, colours in color. idx holds one directed edge per PAIR of mesh-local
 * indices: edge e is idx[first_index + 2e] -> idx[first_index + 2e + 1], e < num_indices / 2; a trailing odd index is ignored and an
 * edge with an index >= num_vertices is skipped. Bit 0 of the low 28 bits of subpath_kind is the fill rule: 0 = NonZero, 1 = EvenOdd.
 * No contour structure is stored: winding needs none. Everything that treats meshes as vertex and index ranges (vgx_mesh_bounds,
 * vgx_merge*, vgx_cache_localize / _submit / _update) handles the kind like any other; the consumers of TRIANGLES -- vgx_pick,
 * vgx_raster, vgx_raster_frame, vgx_raster_textured, vgx_raster_painted -- skip such a mesh whole. */
#define VGX_CONTOUR_EVEN_ODD 0x1u

/* Totals of a batch. Filled by the *_count calls (host struct). */
typedef struct vgx_sizes {
	uint64_t num_poly_vertices;
	uint64_t num_subpaths;
	uint64_t num_meshes;
	uint64_t num_vertices;
	uint64_t num_indices;
	uint64_t num_serial_draws; /* draws that needed the exact serial lane path (degenerate input) */
	uint64_t num_cmd_instances;/* path commands summed over draws (flatten work items) */
	uint64_t num_elements;     /* polyline vertices summed over meshes (stroker work items) */
	uint64_t num_fill_elements;/* ... of which belong to convex-fill meshes (the rest to polyline strokes) */
	uint64_t num_drawcmds;     /* draw commands / vertex buffers of the assembly step (0 unless vgx_set_assembly armed it) */
} vgx_sizes;

/* Flatten output (pathGetVertices / pathGetSubPaths for every draw). NULL members are skipped. */
typedef struct vgx_flat_out {
	float* poly;              /* [cap_poly_vertices][2] */
	vgx_subpath* subpaths;    /* [cap_subpaths] */
	vgx_draw_info* draw_info; /* [ndraws] */
	uint64_t cap_poly_vertices;
	uint64_t cap_subpaths;
} vgx_flat_out;

/* Tessellation output: the three vg::Mesh streams concatenated mesh after mesh + a mesh table.
 * Alignment: that of the element types and no more -- pos 8 bytes, color 4, idx 2, meshes 8 (its records hold uint64_t). The streams
 * may start anywhere such a pointer can: in the middle of a 16-byte word, at the last element of a cache line. Every entry that
 * writes one of these -- vgx_tessellate, vgx_tessellate_emit, vgx_tessellate_immediate, vgx_tessellate_dashed, vgx_stroke,
 * vgx_stroke_emit, vgx_cache_submit, vgx_merge / vgx_merge_uv / vgx_merge_uv_stream, vgx_concave_emit, vgx_concave_contours, vgx_concave_triangulate, vgx_text_quads -- returns
 * VGX_E_INVALID_ARG on the host, with nothing enqueued, for a pointer below that alignment.
 * Range: nothing outside [0, cap_vertices) of pos and color, [0, cap_indices) of idx and [0, cap_meshes) of meshes is read or
 * written, whatever the status the call ends with. */
typedef struct vgx_mesh_out {
	float* pos;       /* [cap_vertices][2] */
	uint32_t* color;  /* [cap_vertices]; non-AA meshes get the draw's colour on every vertex */
	uint16_t* idx;    /* [cap_indices] */
	vgx_mesh* meshes; /* [cap_meshes] */
	uint64_t cap_vertices;
	uint64_t cap_indices;
	uint64_t cap_meshes;
} vgx_mesh_out;

/* ---- draw-command assembly (optional next step of the frame) ------------------
 * What createDrawCommand_VertexColor / _Clip do after every stroker call (src/vg.cpp:5207-5244, 5297-5317): vertices go to
 * the current vertex buffer until it would exceed m_MaxVBVertices (allocVertices, :5321-5342), a new vertex buffer
 * forces a new draw command, meshes otherwise merge into the previous command when type and handle agree
 * (allocDrawCommand, :5359-5407), and indices are rebased by the vertices already in the COMMAND
 * (vgutil::batchTransformDrawIndices, vg_util.cpp:447-520). One vgx_drawcmd per draw command; 48 bytes. */
typedef struct vgx_drawcmd {
	uint64_t first_vertex;  /* where the command's vertices start in the pos / color / uv streams */
	uint64_t first_index;   /* DrawCommand::m_FirstIndexID: into the idx stream = the frame's single index buffer */
	uint64_t first_mesh;    /* first mesh merged into the command */
	uint32_t num_vertices;  /* DrawCommand::m_NumVertices */
	uint32_t num_indices;   /* DrawCommand::m_NumIndices */
	uint32_t num_meshes;
	uint32_t vertex_buffer; /* DrawCommand::m_VertexBufferID, counted from 0 for the batch */
	uint32_t first_vertex_in_vb; /* DrawCommand::m_FirstVertexID: offset inside its vertex buffer (0 for the buffer's first command) */
	uint32_t state_key;     /* the vgx_draw::state_key its meshes share (type / handle / generation); 0 without VGX_ASM_SPLIT_STATE */
} vgx_drawcmd;

enum { VGX_ASM_SPLIT_STATE = 1u }; /* vgx_assembly::flags: a change of vgx_draw::state_key between consecutive meshes starts a new
                                    * draw command inside the same vertex buffer (otherwise: one command per vertex buffer) */

typedef struct vgx_assembly {
	vgx_drawcmd* drawcmds;       /* DEVICE [cap_drawcmds]; 2 * vertices / max_vb_vertices + 2 (+ number of state changes) entries always suffice */
	uint64_t cap_drawcmds;
	uint64_t* dev_num_drawcmds;  /* DEVICE, may be NULL: receives the number of draw commands */
	uint32_t max_vb_vertices;    /* Config::m_MaxVBVertices (vg.cpp:726, <= 65536); 0 = 65536 */
	uint32_t flags;              /* VGX_ASM_* */
	/* the third vertex stream of createDrawCommand_VertexColor: every vertex gets the white-pixel UV (vg.cpp:5218-5225,
	 * vgutil::memset32 / memset64 of getWhitePixelUV): uv_bytes = 4 (VG_CONFIG_UV_INT16: int16 x 2) or 8 (float x 2) */
	void* uv;                    /* DEVICE [cap_vertices][uv_bytes], may be NULL */
	uint32_t uv_bytes;           /* 0 (no UV stream), 4 or 8 */
	uint32_t uv_value[2];        /* the constant, as raw bits (uv_value[1] unused for uv_bytes = 4) */
	uint32_t reserved;
} vgx_assembly;

typedef struct vgx_ctx vgx_ctx;         /* per-device context: scratch, scan storage, error state */
typedef struct vgx_pathset vgx_pathset; /* validated path definitions resident in device memory */

/* ---- context ------------------------------------------------------------------------------ */
/* Replaces createPath/createStroker (path.cpp:23-32, stroker.cpp:194-203): owns all scratch. */
int vgx_create(int device, vgx_ctx** out_ctx);
int vgx_destroy(vgx_ctx* ctx);
int vgx_last_hip_error(const vgx_ctx* ctx);
const char* vgx_status_string(int status);
uint32_t vgx_version(void);
/* Bytes of device scratch currently held by the context: every buffer it has grown (polyline staging, tables, scan temp).
   Path-set blobs waiting to be recycled are not scratch and not counted. */
uint64_t vgx_scratch_bytes(const vgx_ctx* ctx);

/* ---- path definitions --------------------------------------------------------------------- */
/* Validates and uploads a path set (round 6: on the DEVICE -- the four arrays go up as they are, the grammar checks are a
 * flagged reduction and every derived table is built by kernels, csrc/vgx_pathset.hip; what the reference does per command
 * while a path is recorded, path.cpp:62-84, 684-726, 761-784. The host reads one 32-byte record at the end; an invalid set
 * is handed to vgx_pathset_validate, which names the status). Grammar per path: first command must start a sub-path
 * (MOVE_TO, ARC, or a closed shape RECT, ROUNDED_RECT[_VARYING], CIRCLE, ELLIPSE); after CLOSE or a closed
 * shape the next command must start a sub-path again (the reference only VG_CHECKs this in debug
 * builds, path.cpp:82,88,764-765). Non-finite arguments are rejected. Synchronous.
 * A set whose paths are ALL made of MOVE_TO / LINE_TO / CLOSE only (polylines and polygons: pathMoveTo / pathLineTo /
 * pathClose, path.cpp:64-85, 707-726) also gets the polyline layout of every path here -- which commands add a vertex,
 * the vertex pathClose pops, the sub-path table: none of it depends on a draw -- and vgx_tessellate then moves such a
 * set's vertices through the draws' transforms without deciding anything again (csrc/vgx_thin.h; same output). */
int vgx_pathset_create(vgx_ctx* ctx, const vgx_pathset_desc* desc, vgx_pathset** out_ps);
/* Inspection (tests): one of the set's device tables copied to host memory; *bytes = its size (dst may be NULL to ask).
 * VGX_PS_TABLE_SCALARS: uint32[8] = longest path in commands, has serial paths, has empty paths, static thin layout, sub-paths,
 * npaths, ncmd, 0. */
enum { VGX_PS_TABLE_CMD_FLAGS = 0, VGX_PS_TABLE_SP_START = 1, VGX_PS_TABLE_PATH_FLAGS = 2, VGX_PS_TABLE_CMDREC = 3, VGX_PS_TABLE_PATH_SUB_BEGIN = 4,
       VGX_PS_TABLE_SUB_LAST_CMD = 5, VGX_PS_TABLE_CMDTHIN = 6, VGX_PS_TABLE_THIN_PATH = 7, VGX_PS_TABLE_THIN_SUB = 8, VGX_PS_TABLE_SCALARS = 9 };
int vgx_pathset_read_table(vgx_ctx* ctx, const vgx_pathset* ps, int which, void* dst, uint64_t cap_bytes, uint64_t* bytes);
/* The validation step of vgx_pathset_create alone (host only, needs no device). */
int vgx_pathset_validate(const vgx_pathset_desc* desc);
int vgx_pathset_destroy(vgx_ctx* ctx, vgx_pathset* ps);

/* ---- flatten: pathReset + path commands (+ optional transformPath) ------------------------- */
/* `draws` is a DEVICE pointer to ndraws vgx_draw records, 16-byte aligned (the kernels read a record as four 16-byte
 * words; hipMalloc memory and any offset that is a multiple of the 64-byte record are). apply_transform != 0 writes the
 * transformed polyline (what the stroker consumes); 0 writes pathGetVertices as-is.
 * _count runs count+scan and returns totals (synchronises the stream once to read them back);
 * _emit must follow with the same arguments and DEVICE output buffers of at least those sizes. */
int vgx_flatten_count(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream);
int vgx_flatten_emit(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int apply_transform, const vgx_flat_out* out, void* stream);
/* Single asynchronous call, the form for steady state (like vgx_tessellate): the same ordered output as _count + _emit from ONE
 * walk over every cubic, no host round trip. `out` carries the caller's capacities (out->poly and out->subpaths must be given;
 * out->draw_info may be NULL); `dev_sizes` (DEVICE vgx_sizes, may be NULL) receives the totals -- num_poly_vertices,
 * num_subpaths, num_meshes, num_cmd_instances, num_serial_draws -- and `dev_status` (DEVICE uint32, may be NULL) VGX_OK /
 * VGX_E_NOSPACE (a capacity was too small: the totals say what is needed, the buffers' contents are undefined) / ... .
 * Replaces pathReset + the path commands + pathGetVertices / pathGetSubPaths (+ transformPath) for every draw, reference
 * src/path.cpp:44-78, 86-201, 684-726, src/vg.cpp:4957-4975. */
int vgx_flatten(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, int apply_transform, const vgx_flat_out* out,
                vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- tessellate: flatten + transformPath + one strokerXXX call per sub-path per op --------- */
/* _count: flatten into context scratch, size every mesh, scan; returns totals (one stream sync).
 * _emit: writes pos/color/idx/meshes (DEVICE buffers). Must follow _count with the same batch. */
int vgx_tessellate_count(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream);
int vgx_tessellate_emit(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* stream);
/* Single asynchronous call for steady state: count + scan + emit with NO host round trip. Output
 * capacities are checked on the device; `dev_sizes` (DEVICE vgx_sizes, may be NULL) receives the
 * totals and `dev_status` (DEVICE uint32, may be NULL) receives VGX_OK / VGX_E_NOSPACE / ... .
 * Template mode: when the last vgx_tessellate_count found that the draws repeat their first P draws (>= 32 times, > 2048 draws)
 * in everything but mtx, fill_color, stroke_color and state_key, it flattened the period ONCE in local space (the reference flattens before it transforms,
 * vg.cpp:4957-4975) and vgx_tessellate on this path set with any whole number of periods is one kernel: per instance the
 * template's vertices through the instance's transform, the stroker's per-element arithmetic, stores. Every call re-checks all
 * draw records against the counted period on the device; a draw that differs in another field ends the call with
 * VGX_E_STALE in dev_status (outputs undefined): count again. VGX_TMPL=0 in the environment at vgx_create turns the mode off.
 * The period may also come in a FEW flavours ("classes", at most 64: the same drawing at a handful of scales, say): every
 * instance then equals one class representative in the fields above, each class gets its own template, instances of different
 * classes have different sizes. Such a template belongs to the counted batch: vgx_tessellate takes it for the same number of
 * draws, with every instance still of the class it had at the count (else VGX_E_STALE). VGX_TMPL_CLASSES=0 turns this off.
 * Round joins (round 5): their arc points are counted on the TRANSFORMED polyline (stroker.cpp:1146, 1592), so a template batch with Round
 * joins has no fixed size -- every call counts them for the transforms it is given (two small kernels in front of the emit), dev_sizes holds
 * THIS call's totals, and a call whose output outgrows the caller's buffers ends with VGX_E_NOSPACE in dev_status (the need in dev_sizes,
 * nothing written) although the counted batch fitted. Templates of one class only; VGX_TMPL_ROUND=0 keeps such batches on the ordinary path. */
int vgx_tessellate(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- immediate mode: batches that were never counted -----------------------------------------
 * The reference works in immediate mode: every frame is new content, appended into arrays that grow when they fill up (Path
 * src/path.cpp:748-759, Stroker src/stroker.cpp:2316-2347, vg::Mesh src/vg.cpp:5344-5357). vgx_tessellate_immediate is the batch
 * form of that: flatten + transformPath + the stroker calls for a batch the context may never have seen -- the same output, in the
 * same order, with the same draw-command assembly (vgx_set_assembly) as vgx_tessellate_count + vgx_tessellate_emit -- with no count.
 *   - No prior count is needed: it works on a fresh context and after counts, tessellations or flattens of other batches.
 *   - It fits: VGX_OK in dev_status, dev_sizes holds this batch's totals. Asynchronous: nothing on the host waits for the stream.
 *   - The caller's buffers are too small: VGX_E_NOSPACE; num_vertices, num_indices and num_meshes in dev_sizes are exact. While assembly
 *     is armed, num_drawcmds is exact when those fit and only the draw-command table is too small (the partition runs once the streams
 *     fit: 0 otherwise). Nothing is written past a capacity (as vgx_tessellate).
 *   - The context's scratch is too small: VGX_E_GROWN. Nothing is written past any scratch table. dev_sizes holds the exact flatten
 *     totals (num_cmd_instances, num_poly_vertices, num_subpaths, num_meshes); output totals that were not reached are 0. The need
 *     (with the long sub-paths the heap of the single-pass flatten is sized for) goes to a pinned host mirror of the context by an
 *     asynchronous copy; the NEXT immediate call on the context grows its scratch from it before it launches anything, with the
 *     formulas of vgx_tessellate_count. It reads the mirror only once the copy has completed (an event query): it never blocks on it.
 *   - Convergence: calling again with the same arguments -- reading dev_status in between and, after VGX_E_NOSPACE, growing the
 *     output buffers to dev_sizes -- reaches VGX_OK within three calls (one more when an armed assembly's draw-command table is too small
 *     as well); within one when vgx_reserve was big enough. A batch beyond 2^32 - 16 polyline vertices or command instances ends with
 *     VGX_E_RANGE instead of VGX_E_GROWN: split it.
 *   - Routes: frame-sized batches (<= 2048 draws) take the frame-sized pipeline; larger ones k_flatten_build first, and from the second
 *     call on the same (path set, number of draws) -- once the last call's totals have reached the mirror -- the instanced flatten
 *     when the draws repeat a sequence of paths (checked on the device every call) or the one-walk flatten for long curves, chosen
 *     with vgx_tessellate_count's rules. Template and static-batch modes stay with the counted calls.
 *   - Ends any counted state of the context, as vgx_flatten does: the template, the static batch and the _count / _emit pairing
 *     (count again before the next vgx_tessellate_emit or template-mode vgx_tessellate).
 * Host return values: VGX_OK once the work is enqueued, VGX_E_INVALID_ARG for null ctx / ps / out / stream pointers, VGX_E_HIP when
 * growing the scratch fails; the batch's own verdict is in dev_status. */
int vgx_tessellate_immediate(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out,
                             vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);
/* Size the context's scratch for batches up to these totals without counting anything (host; allocates, may block): ndraws draws
 * and, of `totals`, num_cmd_instances, num_poly_vertices, num_subpaths and num_meshes (the other fields are ignored). A batch within
 * them takes one vgx_tessellate_immediate call (the caller's buffers permitting). */
int vgx_reserve(vgx_ctx* ctx, uint64_t ndraws, const vgx_sizes* totals);

/* ---- stroker level: polylines in, meshes out ----------------------------------------------------- */
/* What the reference hands to strokerConvexFill[AA] / strokerPolylineStroke[AA|AAThin] (include/vg/stroker.h:29-72):
 * vertex lists that are ALREADY flattened and transformed. `poly` (DEVICE, [.][2]) holds the vertices, `subpaths`
 * (DEVICE) one record per vertex list {first_vertex, num_vertices, flags bit0 = isClosed}, `subpath_draw` (DEVICE)
 * the index of the vgx_draw whose fill_* / stroke_* / fringe / scale / tess_tol fields parameterise the calls for that
 * list (path and mtx are ignored). Mesh order: list after list, fill mesh (>= 3 vertices) before stroke mesh (>= 2).
 * vgx_mesh.subpath_kind carries the list index. _count sizes the output (one stream sync), _emit must follow. */
int vgx_stroke_count(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws, vgx_sizes* out_sizes, void* stream);
int vgx_stroke_emit(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* stream);

/* The same in ONE asynchronous call, like vgx_tessellate: the bytes and the mesh order of vgx_stroke_count + vgx_stroke_emit with no host round
 * trip (scratch needs at most two meshes per list, which the host knows). Capacities of `out` are checked on the device: dev_sizes (DEVICE,
 * may be NULL) receives the totals, dev_status (DEVICE uint32, may be NULL) VGX_OK / VGX_E_NOSPACE (exact totals, nothing written past a
 * capacity) / VGX_E_INVALID_ARG (a subpath_draw entry >= ndraws, a cap / join above 2). With it the chain vgx_flatten -> vgx_subpath_draws ->
 * vgx_dash -> vgx_stroke never visits the host. Ends any counted state of the context. */
int vgx_stroke(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths, const vgx_draw* draws, uint64_t ndraws,
               const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- dashed strokes (beyond the reference): vgx_flatten -> vgx_subpath_draws -> vgx_dash -> vgx_stroke_* ----------
 * SVG stroke-dasharray / stroke-dashoffset for the stroker-level boundary: vgx_dash cuts every vertex list of a dashed draw into
 * its "on" pieces, on the device; the pieces are ordinary open vertex lists for vgx_stroke_count / vgx_stroke_emit. The reference
 * has no dashes, so the pass is pinned to the specification below (tests/dash_model.py is its sequential model).
 * Units: the lists are the TRANSFORMED polylines, so pattern and phase are device units: multiply user-space lengths by
 * vgx_draw::scale, as ctxStrokePath* does for the stroke width (vg.cpp:3416).
 * Fills: dashing concerns the stroke only. vgx_stroke_* fills any list of >= 3 vertices whose draw has VGX_FILL_ENABLE, so stroke
 * the dashed lists with draws whose fill_flags are 0 and fill from the undashed lists.
 *
 * Specification, for a source list V_0 .. V_{n-1} with closed flag c whose draw has count > 0:
 *   Segments       m = n when closed, else n - 1; segment i runs from V_i to V_{(i+1) mod n}. n < 2: no output.
 *   Segment length dx = bx - ax, dy = by - ay, len_i = sqrtf(dx*dx + dy*dy): every operation rounded to float32, no FMA.
 *   Fixed point    q(x) = (uint64)((double)x * 65536.0 + 0.5). S_0 = 0, S_{i+1} = S_i + q(len_i), T = S_m, in uint64: integer
 *                  prefix sums, any scan order gives the same values.
 *   Pattern        p_k = q(pattern[first + k]), A_k = sum of p_j for j < k, P = A_count, f = q(phase) mod P.
 *   Validation     entries finite, >= 0 and below 2^40; P > 0; count even and <= VGX_DASH_MAX; first + count <= npattern; phase finite,
 *                  >= 0 and below 2^40; reserved == 0 (records with count == 0 obey all rules but P > 0). Every entry of pattern[],
 *                  referenced or not, must be finite, >= 0 and below 2^40.
 *   "On" intervals for integer r and even k: [r P + A_k - f, r P + A_{k+1} - f) intersected with [0, T].
 *   Snapping       each of the two ends c, with D = 256 (2^-8 units) and i the largest index < m with S_i <= c:
 *                  c - S_i <= D: c := S_i; otherwise S_{i+1} - c <= D: c := S_{i+1}. An interval with e <= s after snapping produces
 *                  nothing. Cuts stay off the vertices: no piece starts or ends with a segment below the reference's VG_EPSILON.
 *   Pieces         X(s), then every V_{j mod n} with s < S_j < e for j = 1 .. m in order, then X(e): an open list, flags = 0.
 *   X(c)           c equals some S_j: the vertex itself, bit for bit (several such j, from zero-length segments: the largest for a
 *                  start, the smallest for an end). Otherwise, inside segment i: t = (float)((double)(c - S_i) / (double)(S_{i+1} - S_i)),
 *                  X = (ax + (bx - ax)*t, ay + (by - ay)*t) in float32 without FMA.
 *   Output order   source lists in input order, pieces by increasing s, vertices contiguous; subpath_draw = the source list's draw,
 *                  subpath_src = its index.
 *   Undashed draws a list whose draw has count == 0 is copied verbatim, with its closed flag and any n.
 *   Closed lists   the last piece is not merged with the first.
 * Example: the closed square (0,0)(10,0)(10,10)(0,10), pattern [4,2], phase 1: (0,0)(3,0) | (5,0)(9,0) | (10,1)(10,5) |
 * (10,7)(10,10)(9,10) | (7,10)(3,10) | (1,10)(0,10)(0,7) | (0,5)(0,1). */
#define VGX_DASH_MAX 32
struct vgx_dash {           /* one per draw, 16 bytes. No typedef: the name vgx_dash is the call's; write `struct vgx_dash` */
	uint32_t first;         /* into pattern[] */
	uint32_t count;         /* 0: the draw is not dashed (its lists pass through); else even, 2..VGX_DASH_MAX */
	float    phase;         /* >= 0, finite; same units as pattern */
	uint32_t reserved;      /* 0 */
};
typedef struct vgx_dash_out {
	float*       poly;          /* DEVICE [cap_poly_vertices][2] */
	vgx_subpath* subpaths;      /* DEVICE [cap_subpaths] */
	uint32_t*    subpath_draw;  /* DEVICE [cap_subpaths]: draw of the source list */
	uint32_t*    subpath_src;   /* DEVICE [cap_subpaths], may be NULL: index of the source list */
	uint64_t cap_poly_vertices, cap_subpaths;
} vgx_dash_out;
/* The validation rules above for HOST arrays (needs no device): VGX_OK or VGX_E_INVALID_ARG. */
int vgx_dash_validate(const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern);
/* poly / subpaths / subpath_draw: the triple vgx_stroke_* takes; dashes [ndraws] and pattern [npattern]: all DEVICE pointers.
 * _count fills num_poly_vertices and num_subpaths of a host vgx_sizes, with one stream sync, and returns the batch's verdict
 * (VGX_E_INVALID_ARG / VGX_E_RANGE as below). It also sizes the context's scratch for the batch.
 * vgx_dash is the asynchronous steady-state form, like vgx_flatten: capacities are checked on the device, dev_sizes (DEVICE, may be
 * NULL) receives the totals and dev_status (DEVICE uint32, may be NULL)
 *   VGX_OK;
 *   VGX_E_NOSPACE      a capacity of `out` is too small: dev_sizes is exact, nothing is written past a capacity (nothing at all);
 *   VGX_E_INVALID_ARG  a dash record or pattern entry breaks the rules, or a subpath_draw entry is >= ndraws: found by a flagged
 *                      reduction, as the path-set grammar check is; nothing is written;
 *   VGX_E_RANGE        a non-finite segment length, a list longer than 2^62 fixed units (or of 2^31 vertices), or more than 2^32 - 1 "on"
 *                      intervals in the call -- counted as the pairs (r, k) with r P + A_k - f < T and r P + A_{k+1} - f > 0 over the dashed
 *                      lists, plus one per undashed list; a pattern far finer than the lists are long: split the batch; nothing is written;
 *   VGX_E_GROWN        the lists have more segments than the context's scratch holds (8 + 8 bytes per segment: S and an overflow guard).
 *                      The scratch is sized by vgx_dash_count, else from out->cap_poly_vertices; as with vgx_tessellate_immediate nothing is
 *                      written, the need goes to the context and the next vgx_dash grows the scratch first: call again. A
 *                      vgx_dash_count of the same batch on the context beforehand rules this out.
 * Work is distributed by OUTPUT: one lane per "on" interval, then one lane per output vertex, whatever the lengths of the segments.
 * Counted state: both calls end any counted state of the context, as vgx_flatten does (count again before the next
 * vgx_tessellate_emit, vgx_stroke_emit or template-mode vgx_tessellate). */
int vgx_dash_count(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths,
                   const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern, vgx_sizes* out_sizes, void* stream);
int vgx_dash(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const uint32_t* subpath_draw, uint64_t nsubpaths,
             const struct vgx_dash* dashes, uint64_t ndraws, const float* pattern, uint64_t npattern,
             const vgx_dash_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);
/* vgx_flat_out::draw_info -> the subpath_draw array vgx_stroke_* and vgx_dash take: subpath_draw[i] = the draw whose sub-paths
 * [first_subpath, first_subpath + num_subpaths) hold i, for i < nsubpaths. All DEVICE pointers; asynchronous. */
int vgx_subpath_draws(vgx_ctx* ctx, const vgx_draw_info* draw_info, uint64_t ndraws, uint32_t* subpath_draw, uint64_t nsubpaths, void* stream);

/* ---- dashed strokes in frames: draws in, the frame's meshes out, one asynchronous call ----------------------------------------
 * The batch form of vgx_tessellate_immediate with one `struct vgx_dash` per draw (dashes: DEVICE [ndraws], may be NULL = no draw is dashed;
 * pattern: DEVICE [npattern]). The record, the rules of vgx_dash_validate and the units are those of vgx_dash: device units, the caller
 * multiplies user lengths by vgx_draw::scale. Output, per draw d in order:
 *   1. the fill meshes of d, exactly as vgx_tessellate_immediate writes them (fills always come from the undashed sub-paths);
 *   2. stroke enabled and dashes[d].count == 0: the stroke meshes of d, exactly as today;
 *   3. stroke enabled and count > 0: for every sub-path s of d in order, the pieces the specification above gives for the transformed
 *      vertex list of s, by increasing start, one mesh per piece: what vgx_stroke writes for that open list with d's stroke fields (caps on
 *      both ends of every piece; AA, non-AA and Thin as for any open list). vgx_mesh::draw = d, subpath_kind = the SOURCE sub-path's index
 *      inside the draw | kind << 28: the pieces of one sub-path share the index;
 *   4. a stroke-disabled draw produces no pieces whatever its record says (the record is still validated);
 *   5. draws of kind VGX_FILL_CONCAVE / _TRILIST / _TEXT behave as in vgx_tessellate_immediate.
 * dev_sizes: the call's totals with vgx_tessellate_immediate's meanings (the flatten totals are those of the source paths). dev_dash_sizes
 * (DEVICE, may be NULL): num_subpaths = pieces of the dashed, stroke-enabled draws, num_poly_vertices = their vertices, other fields 0.
 * With dashes == NULL or every count == 0 the output equals vgx_tessellate_immediate's byte for byte. vgx_set_assembly is honoured as there.
 * dev_status, the union of vgx_tessellate_immediate's and vgx_dash's protocols (the host returns VGX_OK once the work is enqueued):
 *   VGX_E_INVALID_ARG  a dash record, a pattern entry or a cap / join above 2 breaks the rules (a flagged reduction): nothing is written;
 *   VGX_E_RANGE        as for vgx_dash, and beyond 2^32 - 16 polyline vertices or command instances;
 *   VGX_E_NOSPACE      the caller's buffers are too small: num_vertices, num_indices, num_meshes are exact, nothing is written past a capacity;
 *   VGX_E_GROWN        a scratch table of the context is too small: nothing is written past any table, the need goes to pinned mirrors by
 *                      asynchronous copies and the next call grows from them after an event query. The call never blocks.
 * Convergence: repeating the call with the same arguments -- reading dev_status in between and, after VGX_E_NOSPACE, growing the output to
 * dev_sizes -- reaches VGX_OK within four calls; each call can fail for at most one new reason: (1) the flatten scratch is too small (its
 * totals are exact and bound the segment tables), (2) the piece scratch is too small, (3) the caller's buffers are too small. An armed
 * assembly whose draw-command table is too small adds one call. After vgx_reserve_dashed with totals >= the batch's (`totals`: the call's
 * dev_sizes, as for vgx_reserve; `dash_totals`: its dev_dash_sizes) it takes one call.
 * The flatten stage is k_flatten_build's for any number of draws (its mesh descriptors are complete and in frame order, the exact serial
 * builder's included); the dash pass reads the polylines where that stage left them and writes the pieces behind them in the same scratch
 * allocation; the frame's mesh slots are closed-form (csrc/vgx_dashframe.h). Ends any counted state of the context, like
 * vgx_tessellate_immediate; works for any ndraws, on a fresh context and after any other call. */
int vgx_tessellate_dashed(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws,
                          const struct vgx_dash* dashes, const float* pattern, uint64_t npattern,
                          const vgx_mesh_out* out, vgx_sizes* dev_sizes, vgx_sizes* dev_dash_sizes, uint32_t* dev_status, void* stream);
int vgx_reserve_dashed(vgx_ctx* ctx, uint64_t ndraws, const vgx_sizes* totals, const vgx_sizes* dash_totals);

/* ---- draw-command assembly (see vgx_drawcmd / vgx_assembly above) ------------
 * Arms (asm_ != NULL) or disarms (NULL) assembly for the following vgx_tessellate_emit / vgx_tessellate calls on this
 * context. While armed, the uint16 indices in `idx` are vertex-buffer relative (mesh-local index + vertices in front of
 * the mesh inside its vertex buffer, uint16 wrap like the reference's cast, vg_util.cpp:447-520), `drawcmds` receives
 * one record per vertex buffer and vgx_sizes.num_drawcmds their number; pos / color / meshes are unchanged (the vertex
 * streams already are in vertex-buffer order). A mesh with more than max_vb_vertices vertices sets
 * VGX_E_MESH_TOO_LARGE (the reference VG_CHECKs it, vg.cpp:5323); a too small table VGX_E_NOSPACE. The struct is copied.
 * Template batches (see vgx_tessellate) are assembled too: the template pass writes the batch's mesh table for the partition
 * kernels and adds each mesh's base to the indices it emits. */
int vgx_set_assembly(vgx_ctx* ctx, const vgx_assembly* asm_);

/* ---- shape cache: tessellate a drawing once, submit it many times -------------
 * The reference keeps the meshes of a cached command list in the drawing's LOCAL space (addCachedCommand,
 * src/vg.cpp:5808-5841: positions times the inverse of the state transform at record time) and a later submission
 * only transforms them with the current state transform and appends positions, colours and indices to the frame
 * (submitCachedMesh, vg.cpp:6137-6166). All pointers below are DEVICE pointers. */
/* vgx_cache_submit requires PACKED streams in mesh order, which is what vgx_tessellate[_emit] writes: meshes[0] starts at vertex 0 /
 * index 0 and meshes[k + 1].first_vertex == meshes[k].first_vertex + meshes[k].num_vertices (first_index likewise), up to num_vertices /
 * num_indices. It copies an instance's mesh range as ONE block of each stream and sizes it from the first_vertex / first_index of the
 * range's ends. The other readers of this struct (vgx_merge's sequences, vgx_pick, vgx_mesh_bounds) go mesh by mesh. */
typedef struct vgx_cache_desc {   /* CommandListCache::m_Meshes as four streams: what vgx_tessellate[_emit] wrote */
	const float* pos;             /* [num_vertices][2], local space (after vgx_cache_localize) */
	const uint32_t* color;        /* [num_vertices] */
	const uint16_t* idx;          /* [num_indices], mesh-local */
	const vgx_mesh* meshes;       /* [num_meshes] */
	uint64_t num_meshes, num_vertices, num_indices;
} vgx_cache_desc;

typedef struct vgx_cache_instance { /* one submission of a cached command (clCacheRender, vg.cpp:5845-6135). 40 bytes */
	uint64_t first_mesh;          /* CachedCommand::m_FirstMeshID */
	uint32_t num_meshes;          /* CachedCommand::m_NumMeshes */
	uint32_t color;               /* the Color operand of the fill / stroke command being replayed (clCacheRender hands it to
	                               * submitCachedMesh, vg.cpp:5896-5902): meshes cached WITHOUT per-vertex colours -- the non-AA
	                               * flavours, numColors == 1 in addCachedCommand (:5826-5834) -- are drawn with it
	                               * (:6159-6160), the AA flavours with the colours stored at cache time */
	float mtx[6];                 /* State::m_TransformMtx at submission */
} vgx_cache_instance;

/* addCachedCommand: pos[v] <- inverse(draws[meshes[m].draw].mtx) * pos[v] for every vertex of every mesh, with the
 * reference's arithmetic (vgutil::invertMatrix3 in double precision, vg_util.cpp:14-33; transformPos2D). In place. */
int vgx_cache_localize(vgx_ctx* ctx, const vgx_draw* draws, uint64_t ndraws, float* pos, const vgx_mesh* meshes, uint64_t num_meshes, void* stream);
/* submitCachedMesh for `ninst` instances in order: for every mesh of every instance's range, positions through the
 * instance transform (batchTransformPositions), colours (stored ones for AA meshes, the instance's colour for non-AA meshes)
 * and indices copied; mesh records get the instance index as
 * `draw`. Asynchronous like vgx_tessellate (capacities checked on the device, totals in dev_sizes, status in
 * dev_status); honours vgx_set_assembly (createDrawCommand_VertexColor is what submitCachedMesh calls). */
int vgx_cache_submit(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* instances, uint64_t ninst, const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- bounding boxes and view culling (beyond the reference): vgx_mesh_bounds -> vgx_cache_cull -> vgx_cache_submit ----------
 * The reference culls a command only on an empty scissor rectangle (src/vg.cpp:4543-4567). A cached mesh is finished geometry, so
 * its box is an exact min / max, and the box of an instance follows from it exactly (below): instances that miss the view can be
 * dropped on the device before vgx_cache_submit pays 21 bytes per vertex for them. Draws that go through vgx_tessellate* are NOT
 * culled by anything here: no path-level box bounds a Miter stroke, whose joins the reference extrudes up to 200 half widths
 * (kMaxExtrusionScale, src/stroker.cpp:45).
 *
 * vgx_mesh_bounds: bounds[m] = minx, miny, maxx, maxy, the exact minimum and maximum over pos[first_vertex .. first_vertex + num_vertices)
 * of meshes[m], for any mesh stream the library wrote (vgx_tessellate*, vgx_stroke, vgx_cache_submit, vgx_merge, vgx_text_quads:
 * boxes in device space; a localized cache: boxes in local space). Minimum and maximum do not depend on the order of evaluation:
 * the values are the same on every run and for every decomposition of the work. -0 and +0 compare equal and either may be stored.
 * A mesh of 0 vertices gets the empty box (+inf, +inf, -inf, -inf). Positions are never NaN in what the library writes from valid
 * input (path sets reject NaN); the result for a NaN position is unspecified.
 * PRECONDITION, not checked: the mesh table is ascending in first_vertex with disjoint vertex ranges (0-vertex records share their
 * successor's first_vertex or the end of the stream). vgx_tessellate*, vgx_stroke, vgx_cache_submit and vgx_merge write such tables.
 * vgx_text_quads places every run where its record says and writes a 0 / 0 record for a failed run: its table qualifies when the
 * caller laid the runs out ascending (the dense layout does) and no run failed; that is the caller's duty. A table that breaks the
 * rule gets wrong boxes and no status. Only the vertices inside the meshes' ranges are read, whatever the order. All pointers are DEVICE pointers, `pos` 8-byte and `bounds` 16-byte aligned; `bounds` has
 * [num_meshes][4] floats. Asynchronous, no scratch of the context is used, no counted state is ended or disturbed. */
int vgx_mesh_bounds(vgx_ctx* ctx, const float* pos, const vgx_mesh* meshes, uint64_t num_meshes, float* bounds, void* stream);

/* vgx_cache_cull: instances of a cache against view rectangles. views[v] = x0, y0, x1, y1 in device space, closed (the state's
 * scissor, or the canvas); inst_view[i] picks the view of instance i (NULL: view 0 for all), so one call covers a frame whose scissor
 * changes. mesh_bounds = what vgx_mesh_bounds gave for the localized cache. For instance i, in this order:
 *   - Validity. The range [first_mesh, first_mesh + num_meshes) must lie inside the cache and the view index below nviews; else
 *     dev_status receives VGX_E_INVALID_ARG, the record is written with num_meshes = 0, its box is the empty box, it is not kept.
 *   - Local box. L = the union of mesh_bounds[first_mesh .. first_mesh + num_meshes). If L is empty (minx > maxx or miny > maxy: an
 *     empty range, or nothing but 0-vertex meshes) the instance draws nothing: it is culled and its box is the empty box.
 *   - Device box. B = minimum / maximum over the four corners of L, (minx,miny) (maxx,miny) (maxx,maxy) (minx,maxy), each moved
 *     through the very function vgx_cache_submit moves a vertex through: (m0*x + m2*y) + m4, (m1*x + m3*y) + m5 in binary32 without
 *     FMA. Every operation in it is monotone in x and in y, so B contains every vertex the instance submits EXACTLY: no margin, no
 *     tolerance. With m1 == m2 == 0 it is the exact box of those vertices. A NaN among the four corners makes the bound it enters NaN.
 *   - Cull rule. With v = the instance's view: culled iff x0 > x1 || y0 > y1 (an empty view culls everything: the reference's
 *     empty-scissor rule), or B.maxx < x0 || B.minx > x1 || B.maxy < y0 || B.miny > y1. Written this way a NaN bound from a wild
 *     matrix compares false: such an instance is kept (vgx_cache_submit then writes what the reference would).
 * Outputs (all DEVICE):
 *   out->inst[i]    the input record byte for byte when the instance is kept; the same record with num_meshes = 0 when it is not.
 *                   The array keeps its length and order: the next call is vgx_cache_submit with out->inst and ninst, no count
 *                   comes back from the device, and vgx_mesh::draw of the frame still names the original instance. May be the
 *                   input array itself (in place).
 *   out->bounds[i]  B (the empty box for a culled-as-empty or invalid instance). May be NULL.
 *   out->kept       the indices of the kept instances, ascending and dense; out->num_kept their count. Either may be NULL; with
 *                   both NULL the compaction pass is skipped.
 * dev_status (DEVICE uint32, may be NULL): VGX_OK or VGX_E_INVALID_ARG as above. Nothing is written outside the ninst entries of
 * each array (num_kept entries of `kept`). Asynchronous; uses a small scratch of its own, so a counted state survives the call:
 * vgx_tessellate_count -> vgx_mesh_bounds / vgx_cache_cull -> vgx_tessellate_emit works. mesh_bounds and out->bounds are 16-byte
 * aligned. Host return values: VGX_OK once the work is enqueued, VGX_E_INVALID_ARG for null or misaligned pointers or nviews == 0
 * with ninst != 0, VGX_E_RANGE for ninst >= 2^32, VGX_E_HIP. */
typedef struct vgx_cull_out {
	vgx_cache_instance* inst;  /* [ninst]; may be the input array itself */
	float*    bounds;          /* [ninst][4], may be NULL */
	uint32_t* kept;            /* [ninst], may be NULL */
	uint64_t* num_kept;        /* may be NULL */
} vgx_cull_out;
int vgx_cache_cull(vgx_ctx* ctx, const vgx_cache_desc* cache, const float* mesh_bounds, const vgx_cache_instance* inst, uint64_t ninst,
                   const float* views, uint32_t nviews, const uint32_t* inst_view, const vgx_cull_out* out, uint32_t* dev_status, void* stream);

/* ---- hit testing (beyond the reference): vgx_mesh_bounds -> vgx_pick ----------------------------------------------------------
 * Which drawing is under this point? The reference has no hit testing; its users rebuild their shapes on the CPU. Here a frame
 * lives in device memory only, so the library that wrote it answers. `frame` is any mesh stream the library wrote with mesh-LOCAL
 * indices: vgx_tessellate*, vgx_stroke, vgx_cache_submit, vgx_merge and vgx_text_quads without an armed assembly, and a cache
 * (points in local space then). Streams written under vgx_set_assembly carry command-relative indices and are OUT OF SCOPE: the
 * call cannot tell and would test wrong triangles (they go to vgx_pick_commands, below). All pointers are DEVICE pointers. The mesh table must satisfy the ascending
 * precondition of vgx_mesh_bounds (it is what the boxes are computed under).
 *
 * Triangles. Triangle t of mesh m is idx[first_index + 3t .. +3), for t < num_indices / 3.
 *   - A trailing remainder of the index list (num_indices % 3) is ignored.
 *   - A triangle with an index >= num_vertices is skipped, so nothing outside the mesh's own vertex range is ever read.
 *   - With VGX_PICK_SKIP_TRANSPARENT in the query's flags, a triangle with at least one vertex whose colour has alpha 0 (bits 24-31
 *     of the colour word) is skipped. That is the outer ring of an AA fringe, so a pick lands on the solid part only. An AAThin
 *     stroke (VGX_MESH_STROKE_AA_THIN) is nothing but two such rings: it has NO solid triangle under this flag and is never hit.
 * Point in triangle. Let the vertices be a, b, c and the point p, all binary32.
 *   - First the closed box test in binary32 compares: px >= min(ax,bx,cx) && px <= max(ax,bx,cx) && py >= min(ay,by,cy) &&
 *     py <= max(ay,by,cy). A NaN anywhere makes it false.
 *   - Then in binary64 WITHOUT FMA, every difference taken after widening:
 *       A  = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax)
 *       e0 = (bx-ax)*(py-ay) - (by-ay)*(px-ax)        e1, e2: the same for the edges b->c and c->a
 *     A == 0 or NaN: no hit. A > 0: hit iff e0 >= 0 && e1 >= 0 && e2 >= 0. A < 0: hit iff all three are <= 0.
 *   - Why binary64. The difference of two binary32 values whose exponents lie within 29 of each other is exact in binary64
 *     (anything of screen magnitude). Where the two differences of a product have no more than 53 significant bits together -- 24 + 24
 *     = 48 when the four values share a binade, as the corners of a tessellated triangle and a point near them do -- the product is
 *     exact as well, and the sign of a rounded difference of two exact values is its exact sign. Then a point on a shared edge hits
 *     both triangles, no point falls through a seam, and a vertex of a triangle with A != 0 hits it (for p = a: e0 is 0 - 0, e2 is
 *     the difference of one product with itself written both ways round = 0, and e1 equals A as a real number). Outside that range the
 *     expressions still round the same way everywhere under IEEE 754, so every implementation agrees bit for bit; only the
 *     geometric guarantee is lost.
 * Result. Among the meshes m < min(mesh_end, num_meshes), hits[q] takes the LARGEST m that has a hit triangle, and within it the
 *   largest t. Painter's order: the last thing drawn is on top. draw and subpath_kind are copied from that mesh record (draw names
 *   the draw, or the cache instance for a vgx_cache_submit frame). No hit: mesh = triangle = draw = subpath_kind = 0xFFFFFFFF.
 *   mesh_end = 0xFFFFFFFF means all meshes; passing the previous hit's `mesh` walks a stack of overlapping drawings from the top down
 *   (click-through). A maximum does not depend on the order of evaluation: results are identical on every run.
 * mesh_bounds. What vgx_mesh_bounds gave for this stream ([num_meshes][4]), or NULL: then the call computes the boxes itself into
 *   scratch of its own. A mesh whose box does not contain the point (closed, binary32 compares) is never opened. This changes no
 *   result: the triangle test starts with the triangle's own box, and every indexed vertex lies inside the mesh box. For a mesh with
 *   a NaN position, whether its OTHER triangles are found is unspecified, because its box is.
 * Host return values. VGX_OK once the work is enqueued. VGX_E_INVALID_ARG for null or misaligned pointers (queries, hits, mesh_bounds
 *   16-byte; pos 8-byte; color 4-byte; idx 2-byte; meshes 8-byte). VGX_E_RANGE for nqueries > VGX_PICK_MAX_QUERIES or num_meshes >=
 *   2^32 - 1. VGX_E_HIP for a HIP failure. nqueries == 0 or num_meshes == 0 is valid; every hit is "none".
 * Side effects. Exactly nqueries hit records are written and nothing else of the caller's. Asynchronous. Uses scratch of its own
 *   (16 bytes per mesh, 32 with mesh_bounds == NULL), so a counted state survives: vgx_tessellate_count -> vgx_pick ->
 *   vgx_tessellate_emit works. */
#define VGX_PICK_MAX_QUERIES 256
enum { VGX_PICK_SKIP_TRANSPARENT = 1u };
typedef struct vgx_pick_query { float x, y; uint32_t mesh_end; uint32_t flags; } vgx_pick_query;          /* 16 bytes */
typedef struct vgx_pick_hit   { uint32_t mesh, triangle, draw, subpath_kind; } vgx_pick_hit;              /* 16 bytes */
int vgx_pick(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
             const vgx_pick_query* queries, uint32_t nqueries, vgx_pick_hit* hits, void* stream);

/* ---- region queries (beyond the reference): vgx_mesh_bounds -> vgx_pick_rect ---------------------------------------------------
 * Which drawings does this RECTANGLE touch, and which lie wholly inside it? vgx_pick answers for a point and gives one maximum; a
 * pick tolerance (a small square around the cursor: a hairline or an AAThin stroke cannot be clicked with a point) and a marquee
 * (rubber-band) selection ask the same thing of a closed rectangle, and the answer is a SET. `frame` and `mesh_bounds` are as for
 * vgx_pick: mesh-LOCAL indices, the ascending precondition of vgx_mesh_bounds, NULL boxes mean the call computes them into scratch
 * of its own. All pointers are DEVICE pointers. At most VGX_PICK_RECT_MAX_QUERIES = 64 queries per call, deliberately: one 64-bit
 * word per mesh and plane holds one bit per query.
 *
 * Range. Query q looks at the meshes m with mesh_begin <= m < min(mesh_end, num_meshes) (mesh_end = 0xFFFFFFFF: all from
 *   mesh_begin on). mesh_begin >= mesh_end selects nothing.
 * Considered triangles. Exactly vgx_pick's: triangle t < num_indices / 3, skipped when an index is >= num_vertices, skipped under
 *   VGX_PICK_SKIP_TRANSPARENT in the query's flags when a corner has alpha 0; a mesh of kind VGX_MESH_CONTOURS has no triangles.
 * Rectangle touches triangle. R = [x0,x1] x [y0,y1], the corners a, b, c, all binary32.
 *   1. x0 <= x1 && y0 <= y1, else the query selects nothing: an inverted rectangle, or one with a NaN coordinate. A query with a
 *      non-zero `reserved` selects nothing either.
 *   2. The closed box overlap in binary32 compares: x1 >= min(ax,bx,cx) && x0 <= max(ax,bx,cx) && y1 >= min(ay,by,cy) && y0 <=
 *      max(ay,by,cy). A NaN makes it false.
 *   3. A as in vgx_pick: binary64, no FMA, every difference taken after widening. A == 0 or NaN: no.
 *   4. For each of the edges u->v = a->b, b->c, c->a, in that same binary64 form, e(p) = (vx-ux)*(py-uy) - (vy-uy)*(px-ux) at the
 *      four corners p of R: (x0,y0) (x1,y0) (x1,y1) (x0,y1). With A > 0 the edge passes iff some corner has e >= 0, with A < 0 iff
 *      some corner has e <= 0 (a NaN value passes neither). The triangle touches R iff all three edges pass.
 *   This is the separating-axis test of two convex polygons: step 2 is the rectangle's two axes, step 4 the triangle's three.
 *   - Exactness is vgx_pick's argument: differences are exact, products are exact where the operands share a binade, and the sign
 *     of a rounded difference of exact values is its exact sign. So a rectangle that merely touches an edge two triangles share
 *     touches both, and nothing falls through a seam. Checked on the CPU against exact rational arithmetic (a vertex in the
 *     rectangle, or a rectangle corner in the triangle, or an exact segment intersection): 0 disagreements on 60 000 pairs -- a
 *     0..8 integer grid full of touching cases, 1/8-unit coordinates around 300..556, random binary32 in [512, 1024), one pair in
 *     seven and one in eleven with a degenerate side. tests/test_pick_rect_cpu.py repeats it on 2 000 pairs.
 *   - The rectangle x0 == x1, y0 == y1 IS vgx_pick's point test, step for step: step 2 is its box test, the four corners coincide,
 *     and e at them is e0, e1, e2.
 *   - Each rounded product and the rounded difference are monotone in px and in py. So "some corner passes" equals "the corner the
 *     signs of (vx-ux) and (vy-uy) choose passes": with A > 0 the corner (vy-uy >= 0 ? x0 : x1, vx-ux >= 0 ? y1 : y0), with A < 0
 *     the opposite one. An implementation may evaluate that one corner, and must fall back to all four where the chosen corner's
 *     value is NaN (an infinite coordinate times a zero difference): the library does, and the tests hold the two forms equal.
 * Mesh bits, per query and mesh of its range.
 *   touch(m)   some considered triangle of m touches R.
 *   inside(m)  the mesh's vgx_mesh_bounds box lies in R, closed binary32 compares: minx >= x0 && maxx <= x1 && miny >= y0 &&
 *              maxy <= y1. The empty box of a 0-vertex mesh is inside every valid R. The box is that of ALL the mesh's vertices, the
 *              transparent ring of an AA fringe included, whatever the flags: "wholly inside" means the drawing's whole extent.
 * Entries. Without VGX_PICK_RECT_BY_DRAW an entry is a mesh, selected iff touch(m); under VGX_PICK_RECT_WINDOW iff touch(m) &&
 *   inside(m). With VGX_PICK_RECT_BY_DRAW an entry is a maximal run of consecutive meshes OF THE RANGE with equal vgx_mesh::draw --
 *   a draw's fill and stroke meshes, or a whole cache instance of a vgx_cache_submit frame -- selected iff some mesh of the run has
 *   touch and, under VGX_PICK_RECT_WINDOW, every mesh of the run has inside. Its value is the index of the run's first mesh inside
 *   the range. Without VGX_PICK_RECT_WINDOW the selection is a crossing selection.
 * Outputs (all DEVICE; each of the three may be NULL and is then not written).
 *   out->count[q]   the number of selected entries, whatever list_cap is.
 *   out->list[q * list_cap ..]  the min(count[q], list_cap) LOWEST selected entries, ascending. Paging: call again with mesh_begin =
 *                   the last listed mesh + 1, or under VGX_PICK_RECT_BY_DRAW the end of the last listed run (the first mesh behind
 *                   it whose draw differs); the concatenation of the pages equals one call with a large capacity.
 *   out->top[q]     mesh = the largest mesh that has touch and belongs to a selected entry, triangle = its largest touching
 *                   considered triangle, draw and subpath_kind from its record; all four words 0xFFFFFFFF when nothing is selected.
 *   Nothing else of the caller's is written: not the rows behind nqueries, not the entries behind min(count, list_cap) of a row, not
 *   the queries, the frame or mesh_bounds.
 * Host return values and alignment as for vgx_pick (queries, top and mesh_bounds 16-byte; list and count 4-byte). VGX_E_INVALID_ARG
 *   also for out == NULL, out->reserved != 0, or list == NULL with list_cap != 0. VGX_E_RANGE for nqueries >
 *   VGX_PICK_RECT_MAX_QUERIES or num_meshes >= 2^32 - 1. nqueries == 0 (nothing is written) or num_meshes == 0 (every count 0, every
 *   top "none") is valid. There is no dev_status and no VGX_E_GROWN: scratch is bounded by num_meshes alone, 72 bytes per mesh (88
 *   with mesh_bounds == NULL) in buffers of its own, so a counted state and the tables of vgx_pick survive the call.
 * Asynchronous, no host round trip, a fixed number of kernels. Bits are ORed and ANDed, counts summed in a fixed order and maxima
 *   taken: the same bytes on every run. */
#define VGX_PICK_RECT_MAX_QUERIES 64
enum { VGX_PICK_RECT_WINDOW = 2u, VGX_PICK_RECT_BY_DRAW = 4u }; /* beside VGX_PICK_SKIP_TRANSPARENT = 1u */
typedef struct vgx_pick_rect_query { float x0, y0, x1, y1; uint32_t mesh_begin, mesh_end; uint32_t flags, reserved; } vgx_pick_rect_query; /* 32 bytes */
typedef struct vgx_pick_rect_out {
	vgx_pick_hit* top;    /* [nqueries], may be NULL */
	uint32_t*     list;   /* [nqueries][list_cap], may be NULL iff list_cap == 0 */
	uint32_t*     count;  /* [nqueries], may be NULL */
	uint32_t      list_cap, reserved;
} vgx_pick_rect_out;
int vgx_pick_rect(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                  const vgx_pick_rect_query* queries, uint32_t nqueries, const vgx_pick_rect_out* out, void* stream);

/* ---- rendering to an image (beyond the reference): vgx_mesh_bounds -> vgx_raster ------------------------------------------------
 * What does this frame look like? The reference hands its triangles to bgfx (src/vg.cpp:1221-1290); a compute part has no graphics
 * pipeline, and the frame lives in device memory only. vgx_raster draws the meshes [mesh_begin, min(mesh_end, num_meshes)) of `frame`
 * into an RGBA8 image in device memory. `frame` is what vgx_pick accepts: any mesh stream the library wrote with mesh-LOCAL indices
 * (streams written under vgx_set_assembly are drawn by vgx_raster_commands, below), under the ascending precondition of vgx_mesh_bounds. With the mesh range
 * and the scissor a caller replays draw commands one after another. The rule below is written so that every implementation gives the
 * same bytes; there is no tolerance anywhere. All pointers of the frame and the target are DEVICE pointers.
 *
 * Triangles. Enumerated as in vgx_pick: triangle t of mesh m is idx[first_index + 3t .. +3), t < num_indices / 3.
 *   - A trailing remainder of the index list (num_indices % 3) is ignored.
 *   - A triangle with an index >= num_vertices is skipped, so nothing outside the mesh's own vertex range is ever read.
 *   - Meshes of kind VGX_MESH_TEXT and VGX_MESH_TRILIST are skipped whole: they need a texture. Atlas sampling, gradients, image
 *     patterns and stencil clips stay with the display path.
 * Sample. Pixel (i, j) of the image samples the frame at px = (double)(x0 + i) + 0.5, py = (double)(y0 + j) + 0.5. Both are exact.
 * Coverage. Everything in binary64 WITHOUT FMA, vertex coordinates widened first. Let the vertices be a, b, c (binary32).
 *   - Box: px >= min(ax,bx,cx) && px <= max(ax,bx,cx) && py >= min(ay,by,cy) && py <= max(ay,by,cy). A NaN makes it false.
 *   - Canonical edge function of a directed edge u->v. Let lo, hi be the two endpoints ordered by (x, then y) as binary32 values
 *     (lo = u when u.x < v.x, or u.x == v.x and u.y <= v.y). g = (hi.x-lo.x)*(py-lo.y) - (hi.y-lo.y)*(px-lo.x). The edge value is
 *     g when u is lo, else -g; it is 0 when u == v bit for bit. Two triangles that share an edge compute the SAME g, so their two
 *     values are exact negatives of each other whatever rounds: no sample on or near a shared edge is covered twice or not at all
 *     along that edge.
 *   - When is the sign also the exact geometric sign? By the argument of vgx_pick: each difference of two binary32 values whose
 *     exponents lie within 29 of each other is exact in binary64 (the sample is a binary32 value too while |x0 + i| < 2^23), and
 *     where the two differences of a product have no more than 53 significant bits together (24 + 24 when the four values share
 *     a binade, as the corners of a tessellated triangle and a pixel centre near them do) both products are exact; the sign of the
 *     rounded difference of two exact values is its exact sign. Outside that range every implementation still rounds the same way;
 *     only the geometric guarantee is lost, the seam property above is not.
 *   - A = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax). A == 0 or NaN: the triangle covers nothing. s = +1 for A > 0, else -1.
 *     E0 = s * value(a->b), E1 = s * value(b->c), E2 = s * value(c->a).
 *   - Edge k with oriented direction (dx, dy) = s * (v - u) accepts the sample iff Ek > 0, or Ek == 0 && (dy > 0 || (dy == 0 &&
 *     dx < 0)). Of the two directions of a shared edge exactly one takes the tie.
 *   - S = (E0 + E1) + E2. Covered iff the box holds, all three edges accept, and S > 0.
 * Colour at a covered sample. For each of the four 8-bit channels with the vertex values ca, cb, cc: v = ((E1*ca + E2*cb) + E0*cc) / S,
 *   q = min((uint32)(v + 0.5), 255). A mesh with one colour on all vertices (the non-AA kinds) gets exactly that colour: every
 *   operation rounds within 2^-53, so v = c * (1 + e) with |e| < 2^-49, |v - c| < 2^-41, far below the 0.5 that would change q.
 * Blend. The reference's state, BLEND_FUNC_SEPARATE(SRC_ALPHA, INV_SRC_ALPHA, ONE, INV_SRC_ALPHA) (src/vg.cpp:1244-1247), on UNORM8 in
 *   integers, a = the source alpha q, div255(x) = (x + 127) / 255:   RGB d' = div255(s*a + d*(255-a))   A d' = div255(255*a + d*(255-a)).
 *   That is round-to-nearest of the real value (255 is odd: no ties). a == 0 leaves the pixel as it is.
 * Order. A pixel receives its covering triangles in ascending (mesh, triangle) order: painter's order. The image is a function of
 *   that order alone, so every run gives the same bytes.
 * mesh_bounds. As in vgx_pick: what vgx_mesh_bounds gave for this stream, or NULL (the call computes the boxes of the range into
 *   scratch of its own). A prefilter that changes no result, because the rule starts with the triangle's own box; a NaN bound is
 *   taken as no bound.
 * Target. pixels[j * stride + i], 0xAABBGGRR like every colour of this ABI. Only pixels inside image and scissor are ever written;
 *   with VGX_RASTER_CLEAR every such pixel is set to clear_color first.
 * dev_status (DEVICE uint32, may be NULL).
 *   VGX_OK       done.
 *   VGX_E_GROWN  the context's bin scratch was too small (4 x 4 bytes per bin entry = per pair of a mesh and a 16 x 16 tile its box
 *                reaches inside the scissor). NOTHING of the image was written, the clear included. The need went to the context
 *                through a pinned mirror, the next call grows the scratch first: the same call repeated -- dev_status read in
 *                between -- reaches VGX_OK on the second try, or on the first after vgx_raster_reserve. A fresh context holds one
 *                entry per mesh of the range (and the 12.5 % head room of every scratch table).
 *   VGX_E_RANGE  more than 2^32 - 1 triangles or bin entries in the range. Nothing was written.
 * Host return values. VGX_OK once the work is enqueued. VGX_E_INVALID_ARG for null ctx / frame / target, null or misaligned pointers
 *   (mesh_bounds 16-byte; pos 8-byte; pixels, color, dev_status 4-byte; idx 2-byte; meshes 8-byte), stride < width, width or height
 *   above 16384, |x0| or |y0| above 2^23, a scissor outside the image or inverted. VGX_E_RANGE for num_meshes >= 2^32 - 1. VGX_E_HIP
 *   for a HIP failure. An empty scissor, width * height == 0 or an empty mesh range is valid and writes nothing, or only the clear.
 * Side effects. Nothing but pixels inside image and scissor and dev_status is written. Asynchronous. Uses scratch of its own (12 bytes
 *   per mesh of the range, 28 with mesh_bounds == NULL, 16 per bin entry and the sort's temporary storage; vgx_scratch_bytes counts
 *   it), so a counted state survives: vgx_tessellate_count -> vgx_raster of another stream -> vgx_tessellate_emit works.
 * vgx_raster_reserve sizes that scratch ahead for ranges of up to num_meshes meshes and num_bin_entries bin entries. */
enum { VGX_RASTER_CLEAR = 1u };
typedef struct vgx_raster_target {
	uint32_t* pixels;          /* DEVICE [height][stride], 0xAABBGGRR like every colour of this ABI; 4-byte aligned */
	uint32_t width, height, stride;   /* pixels; stride >= width; width, height <= 16384 */
	int32_t  x0, y0;           /* pixel (i, j) samples the frame at (x0 + i + 0.5, y0 + j + 0.5); |x0|, |y0| <= 2^23 */
	uint32_t scissor[4];       /* sx0, sy0, sx1, sy1 in image pixels, half open; pixels outside are never written */
	uint32_t flags;            /* VGX_RASTER_CLEAR: every pixel inside the scissor is set to clear_color first */
	uint32_t clear_color;
} vgx_raster_target;
int vgx_raster(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
               uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_target* target,
               uint32_t* dev_status, void* stream);
int vgx_raster_reserve(vgx_ctx* ctx, uint64_t num_meshes, uint64_t num_bin_entries);

/* ---- a decoded frame to an image: per-draw scissors and clip regions (vgx_cmdlist_decode -> ... -> vgx_raster_frame) -----------------
 * vgx_raster draws every mesh of its range under one scissor. vgx_raster_frame is the same call with the state the reference's submit
 * loop applies between its draw-command table and bgfx: the scissor of each draw command (src/vg.cpp:1226-1235) and the stencil test
 * against the clip region the draw names (:1162-1219). Everything vgx_raster specifies -- triangles, sample, coverage, colour, blend,
 * order, mesh_bounds, target, the skipped kinds VGX_MESH_TEXT and VGX_MESH_TRILIST -- holds here word for word; what follows is added
 * to it, and like it gives the same bytes in every implementation for every input. `state` names two DEVICE arrays indexed by
 * vgx_mesh::draw: the draws (only state_key is read: type = (state_key >> 16) & 0xF, 3 = Clip) and the vgx_draw_state records as
 * vgx_cmdlist_decode wrote them.
 *
 * Draw scissor. Let d = meshes[m].draw and {x, y, w, h} = draw_state[d].scissor. Pixel (i, j) of the image is frame pixel (X, Y) =
 *   (x0 + i, y0 + j); it lies inside the draw's scissor iff x <= X < x + w && y <= Y < y + h, in 64-bit integers (device pixel ratio
 *   1, as in bgfx::setScissor of x, y, w, h). A sample of mesh m takes effect only inside the target's scissor AND the draw's scissor;
 *   w == 0 or h == 0: the mesh does nothing.
 * Stamp. Every pixel carries one word S for the duration of the call: the reference's stencil value without its 8-bit wrap. S is NONE
 *   (0xFFFFFFFF) at the start of every call. Meshes are taken in ascending order, triangles ascending within a mesh, exactly as the
 *   colour order is specified.
 * Clip draws. A mesh whose draw has type 3 writes no colour, whatever its vertex colours are: every sample it covers (the coverage
 *   rule of vgx_raster, the tie rule included) inside both scissors sets S = d. Kind, alpha and winding play no part beyond that rule.
 * Other draws. Let f = clip_first_draw, n = clip_num_draws, rule = clip_rule of draw d. If f == 0xFFFFFFFF or n == 0 there is no test
 *   (the reference's BGFX_STENCIL_NONE for a region that is empty or still open). Otherwise the sample passes iff
 *   (S != NONE && S >= f && S - f < n) == (rule == 0): under Out (rule != 0) a pixel no clip mesh ever touched passes, under In it
 *   fails. A sample that fails is treated as not covered; one that passes is coloured and blended as in vgx_raster.
 *   This is the reference's stencil: regions receive ascending reference values, the last writer of a pixel wins, and the users of a
 *   region all precede the next BeginClip, so "the value the last clip mesh left lies in my region's range" is the EQUAL / NOTEQUAL
 *   test of src/vg.cpp:1207-1213 against the value of :1162-1219 and 3670-3709.
 * Range. S does not survive the call: the mesh range must contain the clip meshes of every region its draws use.
 * Out of scope. Draws of type 1 (ColorGradient) and 2 (ImagePattern) are drawn with their vertex colours, as vgx_raster draws them.
 *   TEXT and TRILIST meshes are skipped and leave S alone.
 * dev_status. As vgx_raster, and VGX_E_INVALID_ARG when a mesh of the range (of any kind) has draw >= num_draws: NOTHING was written,
 *   the clear included. It ranks above VGX_E_GROWN, and VGX_E_RANGE above both; all three are decided in one reduction over the
 *   meshes, so the status does not depend on the order of the work. A bin entry is a pair of a mesh and a 16 x 16 tile its box
 *   reaches inside the target's scissor cut by the draw's; the VGX_E_GROWN protocol is the one of vgx_raster, on the same tables, and
 *   vgx_raster_reserve sizes them for both calls. With an empty target scissor no mesh is looked at and dev_status is VGX_OK.
 * Host return values. As vgx_raster, and VGX_E_INVALID_ARG for a null `state`, null arrays with num_draws > 0, a misaligned `draws`
 *   or `draw_state` (4-byte each), reserved != 0.
 * Side effects. As vgx_raster; beyond its scratch the call keeps 32 bytes per mesh of the range (mode, region, and the two scissors
 *   cut into one rectangle) in a buffer only this call allocates; vgx_scratch_bytes counts it. A counted state survives:
 *   vgx_tessellate_count -> vgx_raster_frame -> vgx_tessellate_emit works. */
typedef struct vgx_raster_draws {
	const vgx_draw*       draws;       /* DEVICE [num_draws]; only state_key is read: type = (state_key >> 16) & 0xF, 3 = Clip */
	const struct vgx_draw_state* draw_state; /* DEVICE [num_draws], as vgx_cmdlist_decode wrote them (declared with that call, below) */
	uint32_t              num_draws;   /* both arrays are indexed by vgx_mesh::draw */
	uint32_t              reserved;    /* 0 */
} vgx_raster_draws;
int vgx_raster_frame(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                     uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                     const vgx_raster_target* target, uint32_t* dev_status, void* stream);

/* ---- text and user meshes in the image: vgx_text_quads -> vgx_merge_uv_stream -> vgx_raster_textured ----------------------------------
 * vgx_raster and vgx_raster_frame skip the two kinds that carry texture coordinates. vgx_raster_textured is vgx_raster_frame word for
 * word -- triangles, sample, coverage, tie rule, draw scissor, stamp, In / Out, order, mesh_bounds, target, and the VGX_E_GROWN /
 * VGX_E_RANGE / VGX_E_INVALID_ARG protocol and ranking -- with ONE difference: a mesh of kind VGX_MESH_TEXT or VGX_MESH_TRILIST is no
 * longer skipped. Such a mesh whose draw has type 0 (Textured; type = (state_key >> 16) & 0xF) is a SAMPLED mesh: its colour is the
 * reference's fs_textured.sc, gl_FragColor = v_color0 * texture2D(s_tex, uv), on the RGBA8 image its draw names (handle =
 * state_key & 0xFFFF, an index into tex->images), under the blend state of vgx_raster. Such a mesh whose draw has type 3 stamps like
 * any clip mesh; one whose draw has type 1 or 2 is drawn with its vertex colours; a mesh of any other kind is drawn exactly as
 * vgx_raster_frame draws it and no UV of it is read.
 * Why is there no second rule for unsampled kinds? The reference samples its white pixel for them, texel 255 in every channel, and
 * the modulate step below gives div255(vc * 255) = vc back exactly: the colour of vgx_raster IS the textured rule on a white image.
 * Like the rest of this section the rule is written so that every implementation gives the same bytes, without a tolerance. None of
 * its constants is a measured number; they are choices that make the result a function of the input alone.
 *
 * UV at a covered sample. With E0, E1, E2, S of the coverage rule and the vertex values ua, ub, uc, per component, in binary64
 *   WITHOUT FMA: u = ((E1*ua + E2*ub) + E0*uc) / S, the form of the colour rule. A vertex value is the binary32 value widened
 *   (uv_bytes 8), or (double)s / 32767.0 of the int16 s (uv_bytes 4: what vgx_text_quads wrote as (int16_t)(s * INT16_MAX)).
 * Texel coordinates. U = u * (double)width, V = v * (double)height. If !(fabs(U) < 2147483648.0) or the same for V (NaN included),
 *   the sample leaves the pixel alone, with the stamp test's result unused: it is treated as not covered.
 * Nearest filter (flags bit 0). ix = (int64)floor(U), iy = (int64)floor(V); the texel is image(wrap(ix), wrap(iy)).
 * Linear filter. T = (int64)floor((U - 0.5) * 256.0 + 0.5): a 24.8 fixed-point coordinate, rounded to nearest. i0 = T >> 8 (floor),
 *   wx = T & 255, i1 = i0 + 1; the same for y with V. Rounding here, not truncating, is what makes a 1:1 blit exact: the
 *   interpolated u may be off by an ulp either way, T still lands on the integer and wx = 0.
 * Wrap, per axis and per index. With the clamp flag of the axis (bit 10 Clamp_U, bit 11 Clamp_V): min(max(i, 0), W - 1); otherwise
 *   the Euclidean remainder of i mod W (in 0 .. W - 1 for negative i too).
 * Filtered channel (linear), in integers, with the four wrapped texels c00 (i0, j0), c10 (i1, j0), c01 (i0, j1), c11 (i1, j1):
 *   (c00*(256-wx)*(256-wy) + c10*wx*(256-wy) + c01*(256-wx)*wy + c11*wx*wy + 32768) >> 16: round-to-nearest of the bilinear value
 *   over 2^16 (the weights sum to 2^16, so the sum stays below 2^32).
 * Modulate, per channel. q = div255(vc * tc): vc the 8-bit vertex channel of vgx_raster's colour rule (already rounded), tc the
 *   texel channel (filtered for linear), div255 the one of the blend.
 * Blend. a = q of the alpha channel. a == 0 leaves the pixel; otherwise the blend of vgx_raster with the four q.
 * Validity. A sampled mesh of the range -- whatever it covers -- is invalid when its handle is >= num_images, or its image has null
 *   or misaligned (4-byte) pixels, a width or height of 0 or above 16384, or stride < width. An invalid sampled mesh ends the call with
 *   VGX_E_INVALID_ARG in dev_status and NOTHING is written, the clear included: decided in the same one reduction as draw >= num_draws,
 *   with the same rank. Image records that no sampled mesh of the range names are not looked at; with num_images == 0 a frame without
 *   sampled meshes is valid.
 * Host return values. As vgx_raster_frame, and VGX_E_INVALID_ARG for a null `tex`, uv_bytes other than 4 or 8, a null or misaligned
 *   `uv` (uv_bytes-aligned) with a non-empty mesh range, null `images` with num_images > 0, a misaligned `images` (8-byte).
 * Out of scope. Gradients and image patterns (draw types 1 and 2, with their paint matrices: vgx_raster_painted, below), mips (the
 *   reference creates none), shaping and the atlas itself. Streams written under vgx_set_assembly: vgx_raster_commands, below.
 * Side effects. As vgx_raster_frame, on the same scratch, and one bit per 16 x 16 tile of the image (which tiles a sampled mesh reaches)
 *   in a buffer only this call allocates; vgx_scratch_bytes counts it. Texels are only read inside [0, height) x [0, width) of a
 *   valid image. */
typedef struct vgx_raster_image {      /* 24 bytes */
	const uint32_t* pixels;            /* DEVICE [height][stride], 0xAABBGGRR, 4-byte aligned */
	uint32_t width, height, stride;    /* 1 .. 16384, stride >= width */
	uint32_t flags;                    /* the reference's ImageFlags bits as Image::m_Flags holds them: bit 0 nearest (Filter_NearestUV),
	                                      bit 10 Clamp_U, bit 11 Clamp_V; every other bit ignored (the reference creates no mips) */
} vgx_raster_image;
enum { VGX_IMAGE_NEAREST = 1u << 0, VGX_IMAGE_CLAMP_U = 1u << 10, VGX_IMAGE_CLAMP_V = 1u << 11 };
typedef struct vgx_raster_textures {
	const void* uv;                    /* DEVICE [frame->num_vertices][uv_bytes]: a stream beside pos / color; read ONLY for vertices of sampled meshes */
	const vgx_raster_image* images;    /* DEVICE [num_images], indexed by state_key & 0xFFFF */
	uint32_t uv_bytes;                 /* 4 (int16 x 2) or 8 (float x 2) */
	uint32_t num_images;
} vgx_raster_textures;
int vgx_raster_textured(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                        uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state, const vgx_raster_textures* tex,
                        const vgx_raster_target* target, uint32_t* dev_status, void* stream);

/* ---- gradient and image-pattern paints in the image: vgx_cmdlist_decode -> vgx_paint_tables -> vgx_raster_painted --------------------------
 * vgx_raster_frame and vgx_raster_textured draw a mesh of a ColorGradient or ImagePattern draw with its vertex colours: black with the
 * global alpha for a gradient, the flat tint for a pattern. vgx_raster_painted is vgx_raster_textured word for word -- triangles, sample,
 * coverage, tie rule, draw scissor, stamp, In / Out, sampled meshes, order, mesh_bounds, target, and the VGX_E_GROWN / VGX_E_RANGE /
 * VGX_E_INVALID_ARG protocol and ranking -- with ONE difference: a mesh whose draw has type 1 (ColorGradient) or 2 (ImagePattern) is a
 * PAINTED mesh, whatever its kind (the reference picks the program by the draw type alone, src/vg.cpp:1251-1283). Its colour is the
 * fragment stage of fs_color_gradient.sc / fs_image_pattern.sc on the vgx_paint record its draw names: handle = state_key & 0xFFFF, an
 * index into paints->gradients (type 1) or paints->patterns (type 2), the records as vgx_cmdlist_decode wrote them (declared with that
 * call, below) and vgx_paint_tables scattered them. Clip draws (type 3) stamp as before. A frame with no draw of type 1 or 2 gives
 * vgx_raster_textured's bytes and status.
 * The reference computes the paint coordinate per vertex (vs_color_gradient.sc: u_paintMat * (pos, 1)) and interpolates it; the map is
 * affine, so it is a function of the sample position alone, and the rule evaluates it at the pixel's sample.
 * Everything below is in binary64 WITHOUT FMA, floats widened first. max(a, b) = a > b ? a : b and min(a, b) = a < b ? a : b, so a NaN
 * has one defined path. px, py are the sample of the coverage rule; m[k] is the paint's matrix[k].
 *
 * Paint coordinate. qx = (m0*px + m3*py) + m6, qy = (m1*px + m4*py) + m7.
 * Gradient (type 1). With ex, ey, rad, fe = params[0..3]:
 *   ax = fabs(qx) - (ex - rad), ay = fabs(qy) - (ey - rad), in = min(max(ax, ay), 0.0), ox = max(ax, 0.0), oy = max(ay, 0.0),
 *   len = sqrt(ox*ox + oy*oy), correctly rounded (IEEE squareRoot), sd = (in + len) - rad, t = (sd + fe*0.5) / fe,
 *   t = t > 0.0 ? t : 0.0 (a NaN gives 0), t = t < 1.0 ? t : 1.0.
 * Gradient ends. Taken as 8-bit values, per channel: x = (double)c * 255.0 + 0.5; q8(c) is 0 when !(x > 0), 255 when x >= 256, else
 *   (uint32)x. The decoder's c / 255.0f gives c back exactly. I = q8(inner_color[k]), O = q8(outer_color[k]).
 * Gradient colour and alpha. Channel: v = I*(1.0 - t) + O*t (GLSL mix), g = min((uint32)(v + 0.5), 255). Alpha: a = div255(g_A * vc_A),
 *   vc_A the vertex alpha of vgx_raster's colour rule, already rounded: the shader's gradient.w * v_color0.w. Vertex RGB is not used.
 *   a == 0 leaves the pixel; otherwise the blend of vgx_raster with (g_R, g_G, g_B, a).
 * Image pattern (type 2). (u, v) = (qx, qy). From there the texel rule of vgx_raster_textured unchanged, on images[paint.image & 0xFFFF]:
 *   texel coordinates with the 2^31 / NaN rule (the sample leaves the pixel), nearest or linear, wrap, modulate div255(vc * tc) on all
 *   four channels with the interpolated vertex colour (the pattern's tint), blend. No UV of the stream is read for a painted mesh.
 * Validity. A painted mesh of the range -- whatever it covers -- is invalid when its handle is at or beyond the table of its type, or
 *   the entry's `type` is not the draw's type, or, for a pattern, image & 0xFFFF >= num_images or that image record is invalid by
 *   vgx_raster_textured's test. An invalid painted mesh is decided in the same one reduction as draw >= num_draws and has the same
 *   rank: VGX_E_INVALID_ARG in dev_status, NOTHING written, the clear included. Entries that no painted mesh of the range names are
 *   not looked at.
 * Host return values. As vgx_raster_textured, and VGX_E_INVALID_ARG for a null `paints`, a null table with a count above 0, a
 *   misaligned table (4-byte).
 * Out of scope. Mips. Streams written under vgx_set_assembly are drawn by vgx_raster_commands, below.
 * Side effects. As vgx_raster_textured, on the same scratch (the 32 bytes per mesh of the range now also name the paint), and a second
 *   bit per 16 x 16 tile of the image (which tiles a painted mesh reaches) in a buffer only this call allocates; vgx_scratch_bytes
 *   counts it. A counted state survives: vgx_tessellate_count -> vgx_raster_painted -> vgx_tessellate_emit works.
 *
 * vgx_paint_tables (HOST only, no context) scatters the list vgx_cmdlist_decode wrote into the two tables: table[p.handle] = p goes
 * into the table of p.type, a later record with the same handle wins, and every entry no record names gets type = 0xFFFFFFFF (an
 * entry a painted mesh must not name). VGX_E_NOSPACE when a handle is at or beyond its table's capacity, VGX_E_INVALID_ARG for a type
 * other than 1 or 2 or a null array with a count above 0; the tables' contents are then unspecified. */
typedef struct vgx_raster_paints {
	const struct vgx_paint* gradients; /* DEVICE [num_gradients], indexed by state_key & 0xFFFF of draws of type 1 */
	const struct vgx_paint* patterns;  /* DEVICE [num_patterns],  indexed by state_key & 0xFFFF of draws of type 2; .image & 0xFFFF indexes tex->images */
	uint32_t num_gradients, num_patterns;
} vgx_raster_paints;
int vgx_raster_painted(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                       uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state, const vgx_raster_textures* tex,
                       const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* dev_status, void* stream);
int vgx_paint_tables(const struct vgx_paint* paints, uint32_t n, struct vgx_paint* gradients, uint32_t cap_gradients,
                     struct vgx_paint* patterns, uint32_t cap_patterns);

/* ---- concave fills in the image: vgx_concave_contours -> vgx_merge -> vgx_raster_concave ------------------------------------------------
 * The calls above draw triangles and skip a mesh of kind VGX_MESH_CONTOURS whole (no bin entry, no stamp). vgx_raster_concave is
 * vgx_raster_painted word for word -- sample, triangle coverage, colour, blend, order, draw scissor, stamp, In / Out, sampled and painted
 * meshes, mesh_bounds, target, and the VGX_E_GROWN / VGX_E_RANGE / VGX_E_INVALID_ARG protocol and ranking -- with ONE difference: a mesh
 * of kind VGX_MESH_CONTOURS is filled by the winding number of its edges, below. It is the compute form of stencil-then-cover, exact in
 * integers. A frame without such a mesh gives vgx_raster_painted's bytes and status. As everywhere in this section every implementation
 * gives the same bytes; there is no tolerance.
 *
 * Edges. Edge e of mesh m is idx[first_index + 2e] -> idx[first_index + 2e + 1], e < num_indices / 2. A trailing odd index is ignored;
 *   an edge with an index >= num_vertices is skipped, so nothing outside the mesh's own vertex range is ever read.
 * Winding at the sample (px, py). Binary64 WITHOUT FMA, coordinates widened first. W is a signed 32-bit sum over the valid edges u -> v:
 *   up = u.y < py && py <= v.y, dn = v.y < py && py <= u.y. Neither holds for a horizontal edge or with a NaN in y: the edge adds 0.
 *   E = the canonical edge value of u -> v exactly as the triangle rule of vgx_raster defines it: lo, hi ordered by (x, then y),
 *   g = (hi.x-lo.x)*(py-lo.y) - (hi.y-lo.y)*(px-lo.x), E = g when u is lo, else -g, and 0 when u == v bit for bit. An edge and its
 *   reverse give exact negatives. up && E < 0 adds +1; dn && E > 0 adds -1 (a NaN E adds 0). Integer addition is associative, so every
 *   decomposition of the work gives the same W, and coincident opposite edges cancel exactly, whatever rounds.
 * Covered iff both hold:
 *   - the sample lies in the closed box B of the mesh: px >= B.minx && px <= B.maxx && py >= B.miny && py <= B.maxy, a NaN bound making
 *     it false. B is the mesh's entry of mesh_bounds. A caller's table is therefore part of the input here, not only a prefilter: it must
 *     hold what vgx_mesh_bounds gives for the stream -- as the parameter has always required -- and what it holds decides. With
 *     mesh_bounds == NULL the call computes exactly those boxes. For closed rings (what vgx_concave_contours writes) the clause changes
 *     nothing, every sample with W != 0 lies inside; it is there because an open edge soup would otherwise cover a half-line to its right;
 *   - W != 0 (NonZero), or (W & 1) != 0 (EvenOdd: bit 0 of the low 28 bits of subpath_kind, VGX_CONTOUR_EVEN_ODD).
 * Why these inequalities. They make the rule the triangle rule's twin: the region takes ties on its right and bottom edges, as the tie
 *   rule of vgx_raster does, and in exact arithmetic the winding of a triangle's three edges equals the triangle's coverage at EVERY
 *   sample, on edges, at vertices and on horizontal edges included. So the interior of vgx_concave_contours' AA pair and its fringe
 *   share every inner edge bit for bit, and a sample on that seam is drawn exactly once.
 * Colour. The mesh is flat: c = color[first_vertex]; a mesh with no vertices does nothing. A covered sample is treated as a covered
 *   sample of vertex colour c in every rule downstream: blended under a colour draw; stamping S = d under a Clip draw (type 3); tested
 *   In / Out like any sample; painted under a draw of type 1 / 2 with vc = c; drawn with c under a Textured draw (type 0), since the
 *   kind carries no UV and is never a sampled mesh. Both scissors apply as to any mesh.
 * Order. The mesh takes ONE place in painter's order, at its mesh index: a pixel sees at most one sample of it.
 * Status. The element count of VGX_E_RANGE becomes triangles plus edges (of the contour meshes that have a bin entry); a contour mesh has
 *   bin entries like any mesh, by its box. Everything else as vgx_raster_painted. Positions that are NaN: as vgx_mesh_bounds says, the
 *   box of such a mesh is unspecified, and so is what the mesh covers; nothing outside image and scissor is written in any case.
 * Host return values, out of scope (streams written under vgx_set_assembly go to vgx_raster_commands): as vgx_raster_painted. Hit testing of what this call draws,
 *   contour meshes included, is vgx_pick_frame, below; vgx_pick still skips the kind.
 * Side effects. As vgx_raster_painted, on the same scratch, and a third bit per 16 x 16 tile of the image (which tiles a contour mesh
 *   reaches) in a buffer only this call allocates; vgx_scratch_bytes counts it. A counted state survives. */
int vgx_raster_concave(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                       uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state, const vgx_raster_textures* tex,
                       const vgx_raster_paints* paints, const vgx_raster_target* target, uint32_t* dev_status, void* stream);

/* ---- hit testing of a decoded frame: what is under the point in the image of vgx_raster_concave (... -> vgx_pick_frame) ------------------
 * vgx_pick answers for bare triangles: it knows no draw scissor, no clip region and no contour mesh, it reports the meshes of a Clip draw,
 * and its closed point-in-triangle rule names both triangles of a seam. vgx_pick_frame answers for the IMAGE: a mesh is hit where
 * vgx_raster_concave would let a sample of it take effect. It takes the frame, range and `state` of vgx_raster_frame and the queries and
 * hit records of vgx_pick; it needs no target, no textures and no paints, because a hit is a statement about geometry and draw state, not
 * about colour. Everything below gives the same words in every implementation for every input; there is no tolerance. All pointers are
 * DEVICE pointers; `frame` is what vgx_raster accepts.
 *
 * Point. px = (double)x, py = (double)y. If !(fabs(px) < 2147483648.0) or the same for py (NaN included) the hit is "none". Otherwise the
 *   point lies in frame pixel X = (int64)floor(px), Y = (int64)floor(py).
 * Range. The meshes m of [mesh_begin, min(mesh_end, num_meshes)) are taken in ascending order. The stamp S of the point is NONE
 *   (0xFFFFFFFF) at the start, exactly as in a vgx_raster_frame call with that range: the range must contain the clip meshes of every
 *   region its draws use.
 * Draw scissor. With d = meshes[m].draw and {x, y, w, h} = draw_state[d].scissor, mesh m exists at the point iff x <= X < x + w &&
 *   y <= Y < y + h, in 64-bit integers. Otherwise it neither stamps nor is hit.
 * Mesh box. With B = the mesh's entry of mesh_bounds, mesh m exists at the point iff px >= B.minx && px <= B.maxx && py >= B.miny &&
 *   py <= B.maxy in binary64, a NaN bound making it false; for every kind. As in vgx_raster_concave the caller's table is part of the input
 *   and must hold what vgx_mesh_bounds gives for the stream; with mesh_bounds == NULL the call computes exactly those boxes (of the range)
 *   into scratch of its own. For a triangle mesh with true boxes the clause changes nothing: the triangle rule starts with the
 *   triangle's own box, which lies inside.
 * Coverage at the point: the raster's rule, not vgx_pick's.
 *   - A mesh of any kind but VGX_MESH_CONTOURS (TEXT and TRILIST included; no UV is read): some valid triangle t < num_indices / 3, all
 *     three indices < num_vertices, satisfies the coverage rule of vgx_raster at the sample (px, py): the binary64 box, the canonical
 *     edge values, the tie rule, S > 0.
 *   - A mesh of kind VGX_MESH_CONTOURS: the rule of vgx_raster_concave at the sample (px, py): W over the valid edges, the fill-rule bit,
 *     and "a mesh with no vertices does nothing".
 *   - Flags. With VGX_PICK_SKIP_TRANSPARENT in the query's flags a triangle with a vertex of alpha 0 is skipped, as in vgx_pick, and a
 *     contour mesh with color[first_vertex] >> 24 == 0 is skipped whole.
 * Clip draws (type 3). A point the mesh covers -- query flags play no part here -- sets S = d. Such a mesh is never a hit.
 * Other draws. Mesh m is a hit for query q iff m < q.mesh_end, it is covered under the query's flags, and the stamp test of
 *   vgx_raster_frame passes with the S the meshes below m left: no test when clip_first_draw == 0xFFFFFFFF or clip_num_draws == 0, else
 *   (S != NONE && S >= f && S - f < n) == (rule == 0).
 * Result. The largest hit m. triangle = the largest covering t of that mesh under the flags, 0xFFFFFFFF for a contour mesh; draw and
 *   subpath_kind come from the mesh record. No hit: all four words are 0xFFFFFFFF. q.mesh_end limits hits only; stamps always come from
 *   every mesh of the range below m, so passing the previous hit's `mesh` walks the VISIBLE stack downward consistently.
 * dev_status (DEVICE uint32, may be NULL). VGX_OK when done. VGX_E_INVALID_ARG when a mesh of the range (of any kind) has draw >=
 *   num_draws: every hit record is then written as "none". Decided in one reduction over the meshes, so it does not depend on the order of
 *   the work. There is no VGX_E_GROWN: every table is sized from the range length and nqueries, which the host knows.
 * Host return values. VGX_OK once the work is enqueued. VGX_E_INVALID_ARG for a null ctx, frame or state, null queries or hits with
 *   nqueries > 0, reserved != 0, null arrays with num_draws > 0, null streams with num_meshes > 0, misaligned pointers (queries, hits,
 *   mesh_bounds 16-byte; pos, meshes 8-byte; color, draws, draw_state, dev_status 4-byte; idx 2-byte). VGX_E_RANGE for nqueries >
 *   VGX_PICK_MAX_QUERIES or num_meshes >= 2^32 - 1. VGX_E_HIP for a HIP failure. nqueries == 0 or an empty range is valid.
 * Side effects. Exactly nqueries hit records and dev_status are written, nothing else of the caller's. Asynchronous. Uses scratch of its
 *   own -- 84 bytes per mesh of the range (32 its state under its draw; as a candidate 4 + 4 + 4 + 8 for its places in the lists and 32
 *   for one covered bit per query), 16 more per mesh of the frame with mesh_bounds == NULL; vgx_scratch_bytes counts it -- so a counted
 *   state survives: vgx_tessellate_count -> vgx_pick_frame -> vgx_tessellate_emit works, and vgx_pick's tables are not touched.
 * Two relations follow from the rule; the tests assert both.
 *   (a) The image is the oracle. For a query at a pixel centre (x0 + i + 0.5, y0 + j + 0.5) with flags 0 and mesh_end = 0xFFFFFFFF,
 *       hit.mesh is the mesh whose identifier vgx_raster_concave leaves in pixel (i, j) of the ID frame: the same streams with every
 *       vertex colour of mesh m set to 0xFF000000 | (m + 1), every non-Clip draw retyped to 0, the kinds TEXT and TRILIST rewritten to
 *       VGX_MESH_FILL, drawn over a clear of 0 under a target scissor that cuts nothing. Opaque source alpha makes the blend a copy, so
 *       no arithmetic of the colour path takes part.
 *   (b) vgx_pick. On a frame with no Clip draw, no region, no contour mesh and scissors that contain the point, at a point where no edge
 *       value of any candidate triangle is 0, vgx_pick_frame equals vgx_pick in all four words: away from the edges the closed rule and
 *       the tie rule agree.
 * Out of scope. Alpha of textures or paints deciding a hit (a fully transparent texel under the cursor still hits its quad), streams
 *   written under vgx_set_assembly (vgx_pick_commands, below), more than VGX_PICK_MAX_QUERIES queries per call. */
int vgx_pick_frame(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds /* may be NULL */,
                   uint64_t mesh_begin, uint64_t mesh_end, const vgx_raster_draws* state,
                   const vgx_pick_query* queries, uint32_t nqueries, vgx_pick_hit* hits,
                   uint32_t* dev_status /* may be NULL */, void* stream);

/* ---- incremental update (beyond the reference): vgx_cache_submit -> vgx_cache_layout -> [vgx_pick -> edit -> vgx_cache_update]* ----
 * Moving or recolouring an instance of a submitted frame changes nothing of the frame's structure: a cached mesh has a fixed size, so
 * the instance keeps its vertex, index and mesh ranges; indices, mesh records, draw commands and UVs do not depend on the transform.
 * Only its positions change, and the colours of its non-AA meshes, which take the instance's colour. vgx_cache_layout tells where
 * every instance lives in the frame; vgx_cache_update rewrites the slices of a few listed instances and keeps the caller's
 * vgx_mesh_bounds table current, so that pick -> edit -> update -> pick needs no pass over the whole frame. All pointers are DEVICE
 * pointers unless marked HOST.
 *
 * vgx_cache_layout: slots[i] = the exclusive prefix sums of meshes, vertices and indices over instances 0 .. i-1, which are exactly
 * the offsets vgx_cache_submit(cache, inst, ninst) writes instance i to (both run the same per-instance function), and the record's
 * first_mesh; slots[ninst] = the totals, with cache_first_mesh = 0. An instance whose range [first_mesh, first_mesh + num_meshes) lies
 * outside the cache contributes zero and sets dev_status (DEVICE uint32, may be NULL) to VGX_E_INVALID_ARG; else VGX_OK. Exactly
 * ninst + 1 records are written. Asynchronous; capacities are not checked (no frame is written). vgx_set_assembly is ignored: the
 * vertex streams of an assembled frame are in the same order, so first_mesh and first_vertex hold for it (first_index then names the
 * position in the index stream, whose VALUES are command-relative). Uses scratch of its own, like vgx_cache_cull and vgx_pick:
 * vgx_tessellate_count -> vgx_cache_layout / vgx_cache_update -> vgx_tessellate_emit works.
 * Host return values: VGX_OK once the work is enqueued; VGX_E_INVALID_ARG for null or misaligned pointers (inst, slots 8-byte,
 * dev_status 4-byte); VGX_E_RANGE for ninst >= 2^32; VGX_E_HIP.
 *
 * vgx_cache_update: `inst` is the instance array with the edited records (mtx, color), `slots` what vgx_cache_layout gave for the
 * array the frame was submitted from. The effective list is dirty[0 .. min(ndirty, *dev_ndirty)); with dev_ndirty == NULL it is
 * dirty[0 .. ndirty), so a list a kernel compacted needs no count on the host. The list may be in any order and may hold duplicates;
 * the result is as if each index were listed once. For each listed d, in this order:
 *   1. d >= ninst, or the range of inst[d] lies outside the cache: the entry is INVALID and is skipped.
 *   2. inst[d].first_mesh != slots[d].cache_first_mesh, or inst[d].num_meshes != slots[d+1].first_mesh - slots[d].first_mesh, or the
 *      range's vertex count in the cache != slots[d+1].first_vertex - slots[d].first_vertex: the entry is STALE and is skipped. The
 *      structure changed, or the slots belong to another array: the caller must submit again.
 *   3. slots[d+1].first_vertex > frame->num_vertices or slots[d+1].first_mesh > frame->num_meshes: INVALID, skipped.
 *   4. Otherwise the slice is rewritten: for every vertex v of the range, frame->pos[slots[d].first_vertex + (v - first vertex of the
 *      range)] = cache.pos[v] moved through the function vgx_cache_submit uses, (m0*x + m2*y) + m4, (m1*x + m3*y) + m5 in binary32
 *      without FMA: the bytes a fresh submit of the edited array would write.
 *   5. Every vertex colour of a mesh of kind VGX_MESH_FILL or VGX_MESH_STROKE is set to inst[d].color.
 *   6. Colours of all other meshes are not written (they do not depend on the instance).
 *   7. Indices, mesh records, draw commands and UVs are never touched.
 *   8. Nothing outside the slices of valid, non-stale listed instances is written.
 * dev_status (DEVICE uint32, may be NULL) does not depend on the order of the work: VGX_E_INVALID_ARG if any listed entry is invalid,
 * otherwise VGX_E_STALE if any is stale, otherwise VGX_OK. Entries that pass are written in every case.
 * frame->mesh_bounds, when given, is the table vgx_mesh_bounds computed for this frame: every frame mesh of an updated instance gets
 * its exact min / max box over the new positions, with the bytes vgx_mesh_bounds would produce on the updated frame (the minimum of
 * -0 and +0 is -0, the maximum +0, as the integer images order them); a 0-vertex mesh gets the empty box; every other entry is
 * untouched. The result for a NaN position is unspecified, as in vgx_mesh_bounds.
 * Culled frames. A frame written from records vgx_cache_cull zeroed (num_meshes = 0) updates like any other: a culled instance has an
 * empty slice, and listing it writes nothing. An instance that ENTERS or LEAVES the view changes the structure (its num_meshes differs
 * from what the slots say: VGX_E_STALE) and needs a new submit. The bounds / kept outputs of vgx_cache_cull are not refreshed here.
 * Host return values: VGX_OK once the work is enqueued; VGX_E_INVALID_ARG for null or misaligned pointers (inst, slots, dev_ndirty
 * 8-byte; frame->pos 8-byte; frame->mesh_bounds 16-byte; dirty, frame->color, dev_status 4-byte); VGX_E_RANGE for ninst or ndirty >=
 * 2^32; VGX_E_HIP. ndirty == 0 is valid and writes nothing but VGX_OK to dev_status. Asynchronous; scratch of its own (16 bytes per
 * listed entry), so a counted state survives. Two calls on one stream take effect in order. */
typedef struct vgx_cache_slot {   /* where instance i lives in the frame vgx_cache_submit writes. 32 bytes */
	uint64_t first_mesh;          /* first FRAME mesh of the instance */
	uint64_t first_vertex;        /* into the frame's pos / color streams */
	uint64_t first_index;         /* into the frame's idx stream */
	uint64_t cache_first_mesh;    /* the record's vgx_cache_instance::first_mesh (0 in the closing entry) */
} vgx_cache_slot;
int vgx_cache_layout(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst,
                     vgx_cache_slot* slots /* DEVICE [ninst + 1] */, uint32_t* dev_status, void* stream);

typedef struct vgx_update_frame {
	float*    pos;                /* DEVICE: the frame's streams as vgx_cache_submit wrote them */
	uint32_t* color;
	uint64_t  num_vertices, num_meshes;   /* HOST: the frame's totals; nothing is written at or beyond them */
	float*    mesh_bounds;        /* DEVICE [num_meshes][4], may be NULL: vgx_mesh_bounds' table for this frame, refreshed */
} vgx_update_frame;
int vgx_cache_update(vgx_ctx* ctx, const vgx_cache_desc* cache, const vgx_cache_instance* inst, uint64_t ninst,
                     const vgx_cache_slot* slots, const uint32_t* dirty /* DEVICE [ndirty] */, uint64_t ndirty,
                     const uint64_t* dev_ndirty /* DEVICE, may be NULL */, const vgx_update_frame* frame,
                     uint32_t* dev_status, void* stream);

/* ---- damage redraw: redraw only the tiles an edit can have changed -------------------------------------------------------------
 * vgx_cache_update rewrites a few instances; vgx_raster_concave would draw the whole frame again. Every effect a mesh has on a
 * sample -- coverage, a contour mesh's winding rule, a clip stamp -- starts with "the sample lies in the mesh's box", so redrawing
 * the 16 x 16 tiles the OLD and the NEW boxes of the edited meshes reach gives the image of a full redraw, byte for byte.
 *
 * The damage bitmap. TW = ceil(width / 16), TH = ceil(height / 16), NT = TW * TH. Tile (tx, ty) covers image pixels
 * [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16) -- aligned to pixel (0, 0) of the image, not to a scissor -- and is bit k = ty * TW + tx:
 * word k >> 5, bit k & 31 of a DEVICE array of vgx_damage_words(width, height) = ceil(NT / 32) uint32 the caller owns and zeroes.
 * The mark calls only OR into it; bits at or beyond NT are never set and never read. Every bit set: everything is damaged.
 * The tiles a box B = (minx, miny, maxx, maxy) -- one vgx_mesh_bounds record -- reaches in an image of width x height at origin
 * (x0, y0): the columns [i0, i1] of the pixels whose sample x0 + i + 0.5 may lie in [minx, maxx] and the rows [j0, j1] likewise, by
 * the span rule of the raster (csrc/vgx_raster.h, vgx_raster_span, over [0, width) and [0, height)): with a = minx - (x0 + 0.5) and
 * b = maxx - (x0 + 0.5) in binary64, i0 = max(0, floor(a)) and i1 = min(width - 1, ceil(b)), none if not i0 <= i1; the tiles are
 * [i0 / 16, i1 / 16] x [j0 / 16, j1 / 16]. A superset of the pixels the box holds, never less. If either span is empty the box
 * reaches no tile: the empty box of a 0-vertex mesh, a box outside the image. A NaN bound compares false and bounds nothing, as in
 * the raster: its side of the span stays at the image's edge. Neither the target's scissor nor the mesh's kind or index count
 * plays a part.
 *
 * vgx_damage_meshes marks the boxes mesh_bounds[m], m in [mesh_begin, min(mesh_end, num_meshes)): for a range of draws that was
 * tessellated again, once over the old frame's table and once over the new one's. vgx_damage_instances marks the boxes of the frame
 * meshes [slots[d].first_mesh, slots[d+1].first_mesh) of every d of the effective dirty list, whose rules are vgx_cache_update's:
 * dirty[0 .. min(ndirty, *dev_ndirty)), any order, duplicates allowed. An entry with d >= ninst, slots[d+1].first_mesh > num_meshes or
 * slots[d+1].first_mesh < slots[d].first_mesh is INVALID and is skipped; dev_status (DEVICE uint32, may be NULL) is
 * VGX_E_INVALID_ARG if any entry was invalid, else VGX_OK, whatever the order of the work. ndirty == 0 writes nothing but the
 * status. Of `target` only width, height, x0 and y0 are read (pixels may be NULL): the tile grid is the one the raster call uses.
 * The chain, all on one stream: zero the bits; vgx_damage_instances (the old boxes); vgx_cache_update with the same table as
 * frame->mesh_bounds; vgx_damage_instances (the new boxes); vgx_raster_damaged with VGX_RASTER_CLEAR.
 * Host return values: VGX_OK once the work is enqueued; VGX_E_INVALID_ARG for null or misaligned pointers (mesh_bounds 16-byte;
 * slots, dev_ndirty 8-byte; dirty, tile_bits, dev_status 4-byte) or a target wider or higher than 16384 or with |x0|, |y0| > 2^23;
 * VGX_E_RANGE for num_meshes >= 2^32 - 1, ninst or ndirty >= 2^32; VGX_E_HIP. Asynchronous; scratch of their own (8 bytes per listed
 * entry), so a counted state survives.
 *
 * vgx_raster_damaged is vgx_raster_concave word for word with ONE difference: a pixel is written, cleared or blended only if it
 * lies inside the image, inside the target's scissor AND in a tile whose bit is set. Sample, coverage, winding rule, colour, blend,
 * order, draw scissor, stamp, In / Out, sampled and painted meshes and the ranking of VGX_E_RANGE / VGX_E_INVALID_ARG hold as they
 * stand; VGX_E_INVALID_ARG for a mesh with draw >= num_draws is decided over every mesh of the range, whatever the bits say. With
 * every bit set the call leaves vgx_raster_concave's bytes and status; with no bit set it writes nothing, the clear included.
 * The property: let I0 be the image vgx_raster_concave with VGX_RASTER_CLEAR draws of frame F0 and I1 that of F1, and let every tile
 * be marked that the box of any mesh that differs between F0 and F1 reaches under either frame's boxes. Then vgx_raster_damaged of
 * F1 over I0, with the same target, tables and VGX_RASTER_CLEAR, leaves I1 byte for byte. Proof:
 *   a sample outside every such box sees the same sequence of effects in both frames, stamps included, so its pixel of I0 is I1's;
 *   a sample in a marked tile is cleared and receives ALL meshes of the range through the tile's bin entries, as in the full call;
 *   a sample in an unmarked tile lies outside every such box (a box's tiles hold all its samples) and is not written.
 * A bin entry is a pair of a mesh and a MARKED tile its box reaches inside the two scissors. The call sorts a WINDOW of entries, not
 * the capacity a full render left behind: min(max_entries, the entry tables' capacity) when max_entries != 0, else what the previous
 * vgx_raster_damaged on this context measured plus 12.5 % + 256 once that has come back to the host, else 16384 (cut to meshes x
 * tiles of the scissor in every case). A call with more entries than its window ends with VGX_E_GROWN as vgx_raster does: nothing
 * is written, the need comes back to the host behind the call, and the next call -- once the need has landed -- takes a window of
 * at least that need, max_entries or not: the same call repeated reaches VGX_OK. The count is kept apart from the full calls', so
 * a full render in between does not widen the window. Host return values, alignment and the scratch are vgx_raster_concave's;
 * `damage` NULL, damage->tile_bits NULL or misaligned (4-byte) or damage->reserved != 0: VGX_E_INVALID_ARG. */
uint64_t vgx_damage_words(uint32_t width, uint32_t height); /* HOST: ceil(ceil(width / 16) * ceil(height / 16) / 32) */
int vgx_damage_meshes(vgx_ctx* ctx, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end, uint64_t num_meshes,
                      const vgx_raster_target* target, uint32_t* tile_bits, void* stream);
int vgx_damage_instances(vgx_ctx* ctx, const float* mesh_bounds, uint64_t num_meshes, const vgx_cache_slot* slots, uint64_t ninst,
                         const uint32_t* dirty, uint64_t ndirty, const uint64_t* dev_ndirty /* may be NULL */,
                         const vgx_raster_target* target, uint32_t* tile_bits, uint32_t* dev_status /* may be NULL */, void* stream);
typedef struct vgx_raster_damage {
	const uint32_t* tile_bits;    /* DEVICE [vgx_damage_words(width, height)] */
	uint32_t max_entries;         /* HOST: bin entries this call sorts at most; 0 = the library chooses (above) */
	uint32_t reserved;            /* 0 */
} vgx_raster_damage;
int vgx_raster_damaged(vgx_ctx* ctx, const vgx_cache_desc* frame, const float* mesh_bounds, uint64_t mesh_begin, uint64_t mesh_end,
                       const vgx_raster_draws* state, const vgx_raster_textures* tex, const vgx_raster_paints* paints,
                       const vgx_raster_target* target, const vgx_raster_damage* damage, uint32_t* dev_status, void* stream);

/* ---- a draw-command table to an image: vgx_set_assembly -> vgx_raster_cmds_from_assembly -> vgx_raster_commands ---------------------
 * The calls above read mesh streams with mesh-local indices. vgx_raster_commands draws the frame as the reference hands it to bgfx
 * (src/vg.cpp:1162-1288): vertex streams, ONE index buffer with command-relative indices, and a table of draw commands, each with
 * its scissor, its clip state and its type / handle. It plays the part bgfx plays after vg::end. It adds no pixel arithmetic: the
 * rule is vgx_raster_painted word for word -- sample, coverage, tie rule, colour, blend, draw scissor, stamp, In / Out, texel,
 * gradient and pattern rules, target -- with command c playing both mesh c and draw c. Every implementation gives the same bytes.
 *
 * Triangles. Triangle t of command c is idx[first_index + 3t .. + 3), t < num_indices / 3; a trailing remainder is ignored. A
 *   triangle with an index >= num_vertices is skipped; vertex i of the command is first_vertex + i in pos, color and uv, so nothing
 *   outside the command's own vertex range is ever read.
 * Order. A pixel receives its covering triangles in ascending (command, triangle) order: painter's order.
 * Scissor. The command's scissor is the draw scissor of vgx_raster_frame: {x, y, w, h} in frame pixels, w == 0 or h == 0 draws nothing.
 * Type 3 (Clip). Every covered sample inside both scissors sets the stamp S = c. No colour is read: the reference leaves a clip
 *   command's colours unwritten.
 * Types 0 - 2. The command is tested by the stamp rule of vgx_raster_frame with f = clip_first_cmd, n = clip_num_cmds, rule =
 *   clip_rule; f == 0xFFFFFFFF or n == 0: no test. The range is a range of COMMAND indices of this table.
 * Type 0 (Textured). Every triangle is SAMPLED from images[handle & 0xFFFF] through the UV stream by the rule of vgx_raster_textured:
 *   what fs_textured.sc does for every Textured command. The reference's colour meshes carry the white-pixel UV, and div255(vc * 255)
 *   = vc gives their vertex colour back.
 * Types 1 / 2. The command is painted as in vgx_raster_painted: handle & 0xFFFF indexes paints->gradients / paints->patterns.
 * Precondition. None on order or overlap of the commands' vertex and index ranges; no mesh table and no mesh_bounds are involved.
 * dev_num_cmds (DEVICE, may be NULL). The real command count, cut to num_cmds; records behind it are not looked at.
 * dev_status (DEVICE uint32, may be NULL). All statuses are decided in one reduction before anything is written, the clear included.
 *   VGX_E_RANGE > VGX_E_INVALID_ARG > VGX_E_GROWN.
 *   VGX_E_INVALID_ARG  a command of the table has type > 3, reserved != 0, num_vertices > 65536, a vertex or index range beyond the
 *                streams (in 64 bits), clip_first_cmd != 0xFFFFFFFF with clip_first_cmd + clip_num_cmds > the real count, type 0 with
 *                uv == NULL, handle >= num_images or an image record invalid by vgx_raster_textured's test, or type 1 / 2 invalid by
 *                vgx_raster_painted's validity rule (paints == NULL: every such command is invalid).
 *   VGX_E_GROWN  more chunks or bin entries than the context's scratch holds. A chunk is up to 64 consecutive triangles of one command
 *                (the last chunk of a command is shorter); a bin entry is a pair of a chunk and a 16 x 16 tile inside the union of the
 *                tile rectangles of those of the chunk's triangles that cover something and whose box reaches the target's scissor cut
 *                by the command's. An integer union: a NaN contributes nothing. The protocol is vgx_raster's: nothing is written, the
 *                need goes to the context through a pinned mirror, the repeated call succeeds, and after vgx_raster_commands_reserve
 *                the first call does. A fresh context holds num_cmds + num_indices / 192 chunks and as many entries (and the 12.5 %
 *                head room of every scratch table).
 *   VGX_E_RANGE  more than 2^32 - 1 chunks or bin entries.
 * Host return values. As vgx_raster_painted, on the new structs: VGX_E_INVALID_ARG for null ctx / streams / target, null pos, color
 *   or idx with a count above 0, null cmds with num_cmds > 0, misaligned pointers (pos, cmds, images 8-byte; color, dev_num_cmds,
 *   dev_status, pixels, paint tables 4-byte; idx 2-byte; uv uv_bytes-aligned), uv_bytes other than 0, 4, 8 (0 only with uv == NULL),
 *   reserved != 0, null images with num_images > 0, the target checks of vgx_raster. With an empty target scissor no command is looked
 *   at and dev_status is VGX_OK.
 * Side effects. Nothing but pixels inside image and scissor and dev_status is written. Asynchronous. Scratch of its own in the
 *   context (48 bytes per command, 32 per chunk, 16 per bin entry, two bits per tile, the sort's storage; vgx_scratch_bytes counts it),
 *   so a counted state survives: vgx_tessellate_count -> vgx_raster_commands -> vgx_tessellate_emit works.
 *
 * vgx_raster_cmds_from_assembly turns the product's own assembled frame into that table, on the device. Precondition: assembly was
 * armed with VGX_ASM_SPLIT_STATE. One record per draw command k < min(cap_drawcmds, *dev_num_drawcmds): the ranges are the draw
 * command's, type = (state_key >> 16) & 0xF, handle = state_key & 0xFFFF, scissor and clip rule are those of draw_state[d], d =
 * meshes[first_mesh].draw. The clip region goes from draws to commands: clip_first_cmd = the first command whose d >=
 * clip_first_draw, the end = the first command whose d >= clip_first_draw + clip_num_draws (d does not decrease over the table; a
 * region never starts inside a command, because the generation in state_key changes at BeginClip / EndClip). An open or absent region
 * stays 0xFFFFFFFF / 0. *dev_num_cmds receives the count. dev_status: VGX_E_INVALID_ARG for a command whose first_mesh or d lies
 * outside its table, or when any of the num_meshes meshes has kind VGX_MESH_CONTOURS (edge pairs are not triangles: contour fills
 * stay with vgx_raster_concave); else VGX_OK. Host: VGX_E_INVALID_ARG for null ctx / state / out / dev_num_cmds, null tables with a
 * count above 0, misaligned pointers (8-byte; dev_num_cmds, dev_status, draw_state 4-byte), VGX_E_RANGE for cap_drawcmds > 2^32 - 1.
 *
 * vgx_submit_order (HOST only, no context) is the loop of src/vg.cpp:1162-1219: the reference's two tables in the order vg::end
 * submits them. It walks draw_cmds in order; when a command's clip_first_cmd differs from the previous command's and clip_num_cmds
 * > 0, those clip commands are appended first with type = 3; the command follows with clip_first_cmd rewritten to where the copies
 * landed. A region met again after an interruption is appended again, as the reference redraws it. VGX_E_NOSPACE when cap is too
 * small (*num_out is then exact), VGX_E_INVALID_ARG for a clip range beyond nclip or null arrays with a count above 0. */
typedef struct vgx_raster_cmd {     /* the reference's DrawCommand as its submit loop reads it. 56 bytes */
	uint64_t first_vertex;          /* ABSOLUTE, into pos / color / uv (vertex-buffer base + m_FirstVertexID) */
	uint64_t first_index;           /* m_FirstIndexID, into idx */
	uint32_t num_vertices;          /* <= 65536 */
	uint32_t num_indices;
	uint32_t type;                  /* 0 Textured, 1 ColorGradient, 2 ImagePattern, 3 Clip */
	uint32_t handle;                /* low 16 bits: image (type 0), gradient (1), pattern (2); ignored for 3 */
	uint16_t scissor[4];            /* x, y, w, h */
	uint32_t clip_rule;             /* 0 In, 1 Out */
	uint32_t clip_first_cmd;        /* index into THIS table; 0xFFFFFFFF = none */
	uint32_t clip_num_cmds;
	uint32_t reserved;              /* 0 */
} vgx_raster_cmd;
typedef struct vgx_raster_streams {
	const float* pos;               /* DEVICE [num_vertices][2] */
	const uint32_t* color;          /* DEVICE [num_vertices] */
	const void* uv;                 /* DEVICE [num_vertices][uv_bytes]; may be NULL when no command has type 0 */
	const uint16_t* idx;            /* DEVICE [num_indices], command-relative */
	uint64_t num_vertices, num_indices;
	uint32_t uv_bytes;              /* 0 (uv == NULL), 4 (int16 x 2) or 8 (float x 2) */
	uint32_t reserved;              /* 0 */
} vgx_raster_streams;
int vgx_raster_commands(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds /* DEVICE */, uint32_t num_cmds,
                        const uint32_t* dev_num_cmds /* DEVICE, may be NULL: the real count, <= num_cmds */,
                        const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints /* may be NULL */,
                        const vgx_raster_target* target, uint32_t* dev_status, void* stream);
int vgx_raster_commands_reserve(vgx_ctx* ctx, uint32_t num_cmds, uint64_t num_chunks, uint64_t num_bin_entries);
int vgx_raster_cmds_from_assembly(vgx_ctx* ctx, const vgx_drawcmd* drawcmds, uint64_t cap_drawcmds, const uint64_t* dev_num_drawcmds,
                                  const vgx_mesh* meshes, uint64_t num_meshes, const vgx_raster_draws* state,
                                  vgx_raster_cmd* out /* DEVICE [cap_drawcmds] */, uint32_t* dev_num_cmds, uint32_t* dev_status, void* stream);
int vgx_submit_order(const vgx_raster_cmd* draw_cmds, uint32_t ndraw, const vgx_raster_cmd* clip_cmds, uint32_t nclip,
                     vgx_raster_cmd* out, uint32_t cap, uint32_t* num_out);

/* ---- hit testing of a draw-command table: what is under the point in the image of vgx_raster_commands (... -> vgx_pick_commands) --------
 * vgx_pick_frame reads mesh streams with mesh-local indices; on streams written under vgx_set_assembly it would test wrong triangles.
 * vgx_pick_commands is its twin for the assembled frame: it takes the streams and the table of vgx_raster_commands and the kind of
 * queries and hit records vgx_pick_frame takes. It adds no arithmetic: the rule is vgx_pick_frame's word for word with command c
 * playing both mesh c and draw c, exactly as vgx_raster_commands states its pixel rule through vgx_raster_painted. It takes no target,
 * no images, no paints and reads no UV: a hit is a statement about geometry and state. Every implementation gives the same words for
 * every input; there is no tolerance. All pointers are DEVICE pointers unless marked HOST; `streams` and `owners` are HOST structs.
 *
 * Point. As vgx_pick_frame: px = (double)x, py = (double)y; !(fabs(px) < 2147483648.0) or the same for py (NaN included): the hit is
 *   "none". Otherwise X = (int64)floor(px), Y = (int64)floor(py). A query with reserved != 0 is answered "none".
 * Triangles. Those of vgx_raster_commands: triangle t of command c is idx[first_index + 3t .. + 3), t < num_indices / 3; an index >=
 *   num_vertices skips the triangle; vertex i is first_vertex + i. No precondition on order or overlap of the commands' vertex or index
 *   ranges; no mesh box and no mesh_bounds are involved.
 * Scissor. Command c exists at the point iff x <= X < x + w && y <= Y < y + h of its scissor, in 64-bit integers. Otherwise it neither
 *   stamps nor is hit.
 * Coverage. The raster's rule at the sample (px, py), as in vgx_pick_frame: the binary64 box, the canonical edge values, the tie rule,
 *   S > 0 (csrc/vgx_raster.h: vgx_raster_setup, vgx_raster_cover).
 * Type 3 (Clip). A command that exists at the point and has ANY covering triangle sets the stamp S = c. Query flags and limits play no
 *   part, and no colour is read: the reference leaves a clip command's colours unwritten. A clip command is never a hit.
 * Types 0 - 2. Triangle (c, t) is a hit for query q iff the command exists at the point, the triangle covers, (c, t) < (q.cmd_end,
 *   q.tri_end) lexicographically (cmd_end = 0xFFFFFFFF: everything), with VGX_PICK_SKIP_TRANSPARENT in q.flags no vertex of the triangle
 *   has alpha 0, and the stamp test of vgx_raster_frame passes with f = clip_first_cmd, n = clip_num_cmds, rule = clip_rule and the S
 *   the commands below c left: no test when f == 0xFFFFFFFF or n == 0, else (S != NONE && S >= f && S - f < n) == (rule == 0).
 * Result. The largest hit (c, t): cmd = c, triangle = t. The limit cuts hits only; stamps always come from every command below c.
 *   With `owners`, let p = cmds[c].first_index + 3t: mesh = the smallest m with meshes[m].first_index + meshes[m].num_indices > p,
 *   provided that m also has first_index <= p; draw = meshes[mesh].draw. Precondition: the index ranges of the table ascend and are
 *   disjoint, as in the mesh table of an assembled frame, whose first_index names the position in the index stream. With no such mesh,
 *   or without owners, mesh = draw = 0xFFFFFFFF. No hit: all four words are 0xFFFFFFFF.
 * Why a triangle limit. One command holds many drawings -- a whole Tiger is one command -- so click-through steps down INSIDE a command:
 *   with owners, cmd_end = hit.cmd and tri_end = (meshes[hit.mesh].first_index - cmds[hit.cmd].first_index) / 3 reach the next drawing
 *   below the one that was hit.
 * dev_num_cmds (DEVICE, may be NULL). As in vgx_raster_commands: the real count, cut to num_cmds; records behind it are not looked at.
 * dev_status (DEVICE uint32, may be NULL). Decided in one reduction; it does not depend on the order of the work. VGX_E_INVALID_ARG when
 *   a command of the real table has type > 3, reserved != 0, num_vertices > 65536, a vertex or index range beyond the streams (in 64
 *   bits), or clip_first_cmd != 0xFFFFFFFF with clip_first_cmd + clip_num_cmds > the real count: every hit record is then written
 *   "none". Otherwise VGX_OK. Handles are not checked: nothing they name is read. There is no VGX_E_GROWN: overlapping index ranges
 *   leave the number of chunks unbounded by num_indices, so nothing is kept per chunk or per triangle, and every table is sized from
 *   num_cmds and nqueries, which the host knows.
 * Host return values. VGX_OK once the work is enqueued. VGX_E_INVALID_ARG for a null ctx or streams, null cmds with num_cmds > 0, null
 *   queries or hits with nqueries > 0, null pos, color or idx with a count above 0, streams->reserved != 0, uv_bytes other than 0, 4, 8
 *   (0 only with uv == NULL) or a uv not uv_bytes-aligned (validated as vgx_raster_commands does; never read), owners with a null table
 *   and num_meshes > 0, misaligned pointers (hits 16-byte; queries, cmds, pos, owners->meshes 8-byte; color, dev_num_cmds, dev_status
 *   4-byte; idx 2-byte). VGX_E_RANGE for nqueries > VGX_PICK_MAX_QUERIES. VGX_E_HIP for a HIP failure. nqueries == 0 or num_cmds == 0 is
 *   valid. A vgx_pick_cmd_query is 24 bytes and 8-byte aligned, a vgx_pick_cmd_hit 16 bytes and 16-byte aligned.
 * Side effects. Exactly nqueries hit records and dev_status are written, nothing else of the caller's. Asynchronous. Scratch of its
 *   own -- 40 bytes per command (32 its state, 8 its first chunk) and 4 per pair of a command and a query (the largest hit triangle);
 *   vgx_scratch_bytes counts it -- so a counted state survives: vgx_tessellate_count -> vgx_pick_commands -> vgx_tessellate_emit works,
 *   and the tables of vgx_pick, vgx_pick_frame and vgx_raster_commands are not touched.
 * Two relations follow from the rule; the tests assert both.
 *   (a) The image is the oracle. For a query at a pixel centre with flags 0 and cmd_end = 0xFFFFFFFF, (cmd, triangle) is the triangle
 *       whose identifier vgx_raster_commands leaves in that pixel of the ID table: every triangle de-indexed to three vertices of its
 *       own, coloured 0xFF000000 | (g + 1) with g the triangle's ordinal in (command, triangle) order, every non-Clip command retyped
 *       to 0 on a white image with a constant UV (div255 of vc * 255 is vc: no colour arithmetic takes part), drawn over a clear of 0.
 *   (b) vgx_pick_frame. With tri_end = 0, cmd and triangle equal mesh and triangle of vgx_pick_frame with mesh_end = cmd_end on the
 *       one-mesh-per-command frame of the same table, boxes true (where that frame meets the ascending precondition of
 *       vgx_mesh_bounds). */
typedef struct vgx_pick_cmd_query { float x, y; uint32_t cmd_end, tri_end; uint32_t flags, reserved; } vgx_pick_cmd_query; /* 24 bytes */
typedef struct vgx_pick_cmd_hit   { uint32_t cmd, triangle, mesh, draw; } vgx_pick_cmd_hit;                              /* 16 bytes */
typedef struct vgx_pick_owners    { const vgx_mesh* meshes; uint64_t num_meshes; } vgx_pick_owners;                      /* DEVICE table, optional */
int vgx_pick_commands(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds,
                      const uint32_t* dev_num_cmds /* may be NULL */, const vgx_pick_owners* owners /* may be NULL */,
                      const vgx_pick_cmd_query* queries, uint32_t nqueries, vgx_pick_cmd_hit* hits,
                      uint32_t* dev_status /* may be NULL */, void* stream);

/* ---- boxes of a draw-command table: vgx_command_bounds -> vgx_raster_commands_damaged, vgx_pick_commands_boxed -------------------------
 * A mesh stream has vgx_mesh_bounds, and every call that takes its table skips what a box rules out. A command had no box, so
 * vgx_pick_commands reads every triangle of the frame, and after a vgx_cache_update of one drawing of an assembled frame only a full
 * vgx_raster_commands gave a correct image. vgx_command_bounds gives the command table its box table, computed once and refreshed over
 * the few commands an edit touched; vgx_raster_commands_damaged and vgx_pick_commands_boxed take it. None of them adds coverage or
 * pixel arithmetic: every rule is an existing one restricted by a box or a bit. All pointers are DEVICE pointers unless marked HOST;
 * `streams`, `paints`, `target`, `damage` and `owners` are HOST structs.
 *
 * vgx_command_bounds.
 * Range. bounds[c] is written for c in [cmd_begin, min(cmd_end, real count)), the real count being num_cmds cut by *dev_num_cmds as in
 *   vgx_raster_commands. Entries outside the range are neither written nor read, and records outside it are not looked at: after an
 *   edit of a few commands only those are recomputed.
 * Box. bounds[c] = minx, miny, maxx, maxy over the corners of every triangle of command c that vgx_raster_commands draws from: triangle
 *   t is idx[first_index + 3t .. + 3), t < num_indices / 3, a trailing remainder is ignored; a triangle with an index >= num_vertices
 *   takes no part; vertex i is pos[first_vertex + i]. A vertex no such triangle names takes no part either. A command with no such
 *   triangle gets the empty box (+inf, +inf, -inf, -inf).
 * Values. As vgx_mesh_bounds: minimum and maximum do not depend on the order of evaluation, the values are the same on every run and
 *   for every decomposition of the work; -0 and +0 compare equal and either may be stored; the result for a NaN position is
 *   unspecified.
 * Precondition. None on order or overlap of the commands' vertex and index ranges: that is the difference from vgx_mesh_bounds, whose
 *   table must ascend. Where a one-mesh-per-command table does ascend and every vertex of a command is named by one of its triangles,
 *   the two calls give the same table.
 * dev_status (DEVICE uint32, may be NULL). Decided in one reduction over the range. VGX_E_INVALID_ARG when a record of the range has
 *   num_vertices > 65536 or a vertex or index range beyond the streams (in 64 bits): such a record gets the empty box, every other box
 *   is right. Otherwise VGX_OK. type, handle, scissor, the clip fields and `reserved` are not examined: nothing they name is read.
 * Host return values. VGX_OK once the work is enqueued. VGX_E_INVALID_ARG for a null ctx or streams, null cmds with num_cmds > 0, null
 *   bounds when [cmd_begin, min(cmd_end, num_cmds)) is not empty, the stream checks of vgx_pick_commands (color and uv are validated
 *   and never read), misaligned pointers (bounds 16-byte; cmds, pos 8-byte; color, dev_num_cmds, dev_status 4-byte; idx 2-byte).
 *   VGX_E_HIP for a HIP failure. An empty range is valid: dev_status alone is written.
 * Side effects. Exactly the entries of the range and dev_status are written. Asynchronous. Scratch of its own -- 8 bytes per command of
 *   the range, its first chunk of 64 triangles; vgx_scratch_bytes counts it -- so a counted state survives: vgx_tessellate_count ->
 *   vgx_command_bounds -> vgx_tessellate_emit works, and no table of another call is touched.
 *
 * vgx_pick_commands_boxed is vgx_pick_commands word for word -- arguments, point, triangles, scissor, coverage, types, result,
 * statuses, host return values, side effects and scratch -- with one clause added:
 * Box. With cmd_bounds != NULL, command c exists at the point of query q only if minx <= x && x <= maxx && miny <= y && y <= maxy for
 *   the query's x, y and the four floats of cmd_bounds[c], compared in binary32: the closed box, as in vgx_pick. Otherwise it neither
 *   stamps nor is hit FOR THAT QUERY. An entry with a NaN, and the empty box, hold no point.
 * cmd_bounds == NULL: vgx_pick_commands word for word. With cmd_bounds holding what vgx_command_bounds gives for the table no answer
 *   changes: a covering triangle's corners enclose the point, and its command's box encloses them. What the table holds decides, as
 *   mesh_bounds does in vgx_raster_concave: an entry that is too small hides its command from the points outside it, whether it draws
 *   or clips. cmd_bounds has [num_cmds][4] floats and is 16-byte aligned (else VGX_E_INVALID_ARG); entries at and behind the real
 *   count are not read.
 *
 * vgx_raster_commands_damaged is vgx_raster_commands word for word -- triangles, order, scissor, types, paints, dev_num_cmds, the
 * ranking VGX_E_RANGE > VGX_E_INVALID_ARG > VGX_E_GROWN, host return values, side effects -- with two differences:
 * (a) Bits. A pixel is written, cleared or blended only if it lies inside the image, inside the target's scissor AND in a tile whose
 *   bit is set in damage->tile_bits: the bitmap of vgx_damage_meshes, with the same numbering (tile (tx, ty) of the image is bit
 *   ty * TW + tx).
 * (b) Boxes. With cmd_bounds != NULL, command c takes no part -- it neither draws nor stamps -- when the tiles cmd_bounds[c] reaches
 *   over the whole image (the span rule vgx_damage_meshes marks by: vgx_damage_box_tiles, whatever the scissors) hold no set bit.
 *   cmd_bounds must hold what vgx_command_bounds gives for the table; what it holds decides, as mesh_bounds does in
 *   vgx_raster_concave: an entry that is too small drops its command from tiles it reaches, whether it draws or clips.
 * VGX_E_INVALID_ARG is decided over every command of the real table, whatever bits and boxes say. With every bit set and boxes true
 * or NULL the call leaves vgx_raster_commands' bytes and status; with no bit set it writes nothing, the clear included.
 * The property: let I0 be the image vgx_raster_commands with VGX_RASTER_CLEAR draws of table and streams F0 and I1 that of F1, the
 * tables of equal length, and let every tile be marked that the vgx_command_bounds box of any command that differs between F0 and F1
 * (its record, or anything its ranges name) reaches under either frame's boxes. Then vgx_raster_commands_damaged of F1 over I0, with
 * F1's boxes or NULL, the same target, tables and VGX_RASTER_CLEAR, leaves I1 byte for byte. Proof:
 *   a sample outside every such box sees the same sequence of effects in both frames, stamps included, so its pixel of I0 is I1's;
 *   a sample in a marked tile is cleared and receives ALL commands whose box reaches a marked tile -- every command that covers it --
 *     through the tile's bin entries, as in the full call;
 *   a sample in an unmarked tile lies outside every such box (a box's tiles hold all its samples) and is not written.
 * The marks may be finer than the command's box: any boxes that hold every triangle that differs, under both frames, do -- the
 * vgx_mesh_bounds boxes of the edited meshes of an assembled frame, which vgx_cache_update refreshes, mark less than the box of a
 * command of many drawings does. The first and the third line hold for them word for word; the second needs F1's COMMAND boxes true.
 * The chain for an assembled frame, all on one stream: zero the bits; vgx_damage_instances or vgx_damage_meshes (the old boxes:
 * vgx_damage_meshes takes a command box table as its box table); vgx_cache_update or any edit of the streams; vgx_command_bounds over
 * the edited commands; the marks again (the new boxes); vgx_raster_commands_damaged with VGX_RASTER_CLEAR.
 * A bin entry is a pair of a chunk and a MARKED tile inside the chunk's tile rectangle: a chunk that reaches no marked tile costs no
 * entry. The call sorts a WINDOW of entries by vgx_raster_damaged's rule: min(max_entries, the entry tables' capacity) when
 * max_entries != 0, else what the previous vgx_raster_commands_damaged on this context measured plus 12.5 % + 256 once that has come
 * back to the host, else 16384 (cut to chunks x tiles of the scissor in every case). A call with more entries than its window ends
 * with VGX_E_GROWN: nothing is written, the need comes back to the host behind the call, and the next call -- once the need has
 * landed -- takes a window of at least that need, max_entries or not: the same call repeated reaches VGX_OK. The count is kept apart
 * from vgx_raster_commands' and from vgx_raster_damaged's, so a full render in between does not change the window. Chunk capacity
 * follows vgx_raster_commands' protocol and shares its tables (vgx_raster_commands_reserve sizes both); commands skipped by their box
 * contribute no chunks, which is the point of (b): without boxes the count pass reads every triangle of the frame.
 * Host return values and alignment are vgx_raster_commands'; `damage` NULL, damage->tile_bits NULL or misaligned (4-byte),
 * damage->reserved != 0 or cmd_bounds not 16-byte aligned: VGX_E_INVALID_ARG. Scratch: vgx_raster_commands' tables; a counted state
 * survives. */
int vgx_command_bounds(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds,
                       const uint32_t* dev_num_cmds /* may be NULL */, uint32_t cmd_begin, uint32_t cmd_end,
                       float* bounds /* DEVICE [num_cmds][4], 16-byte aligned */, uint32_t* dev_status /* may be NULL */, void* stream);
int vgx_raster_commands_damaged(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds /* DEVICE */, uint32_t num_cmds,
                                const uint32_t* dev_num_cmds /* may be NULL */, const float* cmd_bounds /* may be NULL */,
                                const vgx_raster_image* images, uint32_t num_images, const vgx_raster_paints* paints /* may be NULL */,
                                const vgx_raster_target* target, const vgx_raster_damage* damage, uint32_t* dev_status, void* stream);
int vgx_pick_commands_boxed(vgx_ctx* ctx, const vgx_raster_streams* streams, const vgx_raster_cmd* cmds, uint32_t num_cmds,
                            const uint32_t* dev_num_cmds /* may be NULL */, const float* cmd_bounds /* may be NULL */,
                            const vgx_pick_owners* owners /* may be NULL */, const vgx_pick_cmd_query* queries, uint32_t nqueries,
                            vgx_pick_cmd_hit* hits, uint32_t* dev_status /* may be NULL */, void* stream);

/* ---- concave fills with AA fringes -------------------------------------------------
 * strokerConcaveFillEndAA (src/stroker.cpp:868-1006) alternates libtess2 and the stroker's own loops:
 *   (1) tessTesselate(TESS_BOUNDARY_CONTOURS) of the contours added with strokerConcaveFillAddContour     [caller, CPU]
 *   (2) per boundary-contour vertex two fringe vertices + six indices; the contour vertex moves to the inner fringe
 *       vertex (:887-973)                                                                                  [vgx_concave_move / _emit]
 *   (3) tessAddContour of the moved contours, tessTesselate(TESS_POLYGONS)                                 [caller, CPU]
 *   (4) the interior appended behind the fringe, indices rebased (:976-994)                                [vgx_concave_emit]
 * libtess2 stays on the CPU side of the caller; these two calls do (2) and (4) for a BATCH of concave fills.
 * All pointers are DEVICE pointers. The boundary contours of one fill must be stored back to back in `contour_verts`
 * in tessGetElements order (what tessGetVertices returns), contours sorted by first_vertex. */
typedef struct vgx_contour {       /* one boundary contour of step (1): contourData[2i], contourData[2i+1]. 16 bytes */
	uint64_t first_vertex;         /* into contour_verts */
	uint32_t num_vertices;
	uint32_t fill;                 /* index of the concave fill it belongs to */
} vgx_contour;
typedef struct vgx_concave_fill {  /* one strokerConcaveFillBegin .. EndAA. 48 bytes */
	uint64_t first_contour;        /* its boundary contours [first_contour, first_contour + num_contours) */
	uint32_t num_contours;
	uint32_t color;                /* colour handed to strokerConcaveFillEndAA */
	float fringe;                  /* Stroker::m_FringeWidth */
	uint32_t num_tess_vertices;    /* step (3): tessGetVertexCount            (vgx_concave_emit only) */
	uint32_t num_tess_indices;     /*           tessGetElementCount * 3 */
	uint32_t reserved;
	uint64_t first_tess_vertex;    /* into tess_pos */
	uint64_t first_tess_index;     /* into tess_idx */
} vgx_concave_fill;
/* Step (2), first half: moved[v] = the inner fringe vertex of contour vertex v (what the reference writes back into the
 * contour before it hands it to libtess2 again). `moved` has the layout of contour_verts. Asynchronous. */
int vgx_concave_move(vgx_ctx* ctx, const float* contour_verts, uint64_t num_contour_vertices, const vgx_contour* contours, uint64_t ncontours,
                     const vgx_concave_fill* fills, uint64_t nfills, float* moved, void* stream);
/* Steps (2) + (4): one mesh per fill = [2 vertices, 6 indices per contour vertex][interior from tess_pos / tess_idx with
 * indices rebased by the fringe's vertex count], meshes concatenated in fill order; mesh records carry draw = fill index,
 * kind VGX_MESH_CONCAVE_FILL_AA. contour_verts are the ORIGINAL boundary contours (not the moved ones). Asynchronous
 * like vgx_tessellate (capacities checked on the device, totals in dev_sizes, status in dev_status). */
int vgx_concave_emit(vgx_ctx* ctx, const float* contour_verts, uint64_t num_contour_vertices, const vgx_contour* contours, uint64_t ncontours,
                     const vgx_concave_fill* fills, uint64_t nfills, const float* tess_pos, const uint16_t* tess_idx,
                     const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- concave fills without libtess2 (beyond the reference): vgx_flatten -> vgx_concave_contours -> vgx_merge -> vgx_raster_concave ----
 * A triangulation is needed only when triangles go to a graphics pipeline. A rasteriser that owns the pixel loop fills from the contours
 * by winding number (vgx_raster_concave), so a concave fill needs no triangles, no libtess2 and no host visit: vgx_concave_contours turns
 * the flattened sub-paths of the frame's concave draws into meshes of kind VGX_MESH_CONTOURS on the device.
 * Inputs, all DEVICE pointers: poly, subpaths, draw_info = what vgx_flatten(..., apply_transform = 1, ...) wrote for the frame's draws
 * (poly, subpaths and draw_info 8-byte aligned), and the ndraws vgx_draw records themselves (4-byte aligned).
 * Which draws make meshes. Draw d with VGX_FILL_CONCAVE and without VGX_FILL_ENABLE, with at least one sub-path, of which NONE has fewer
 *   than 3 vertices (the reference's return, src/vg.cpp:3136-3138: one short sub-path drops the whole fill). Every other draw makes
 *   nothing. Let V be the sum of the vertex counts of d's sub-paths.
 * Without VGX_FILL_AA: one mesh of kind VGX_MESH_CONTOURS. Its V vertices are the polyline vertices in order, every colour is fill_color;
 *   each sub-path contributes its closed ring of edges (i, i + 1), the closing edge (last, first) included: 2V indices, the pair of
 *   vertex i at 2i. The rule bit VGX_CONTOUR_EVEN_ODD comes from VGX_FILL_EVEN_ODD. draw = d.
 * With VGX_FILL_AA: two meshes, in the index order of strokerConcaveFillEndAA: fringe, then interior.
 *   Mesh 1, kind VGX_MESH_CONCAVE_FILL_AA, holds ONLY the fringe: 2V vertices and 6V indices, bit for bit what vgx_concave_emit writes
 *   for the same contours with num_tess_vertices = num_tess_indices = 0 and the draw's fringe and fill_color; the draw's own sub-paths
 *   play the part of the boundary contours.
 *   Mesh 2, kind VGX_MESH_CONTOURS: its V vertices are what vgx_concave_move gives for those contours, its rings are the same rings,
 *   its colour is fill_color, its rule bit as above. draw = d on both.
 * Meshes come out ascending by draw, streams dense: the result is sequence `b` of vgx_merge as it stands.
 * Where this differs from the reference. libtess2's first pass (TESS_BOUNDARY_CONTOURS) follows the boundary of the FILLED REGION; this
 *   route follows the INPUT contours. For a simple path (no self-intersection, no overlap between sub-paths) the geometry is the same.
 *   For the rest, fringe and half-fringe inset are per input contour, so an edge that lies inside the filled region gets a fringe too.
 *   Non-AA fills have no such difference: the winding number of the input contours IS the fill rule's definition. A caller who needs the
 *   reference's mesh keeps the libtess2 route (vgx_concave_move / vgx_concave_emit).
 * Asynchronous, with the dev_sizes / dev_status protocol of vgx_concave_emit: capacities are checked on the device; on VGX_E_NOSPACE the
 *   need is in dev_sizes (num_meshes, num_vertices, num_indices) and nothing is written past a capacity; a mesh above 65536 vertices
 *   (V > 65536, with AA V > 32768) sets VGX_E_MESH_TOO_LARGE; sub-paths of a draw that do not lie back to back in poly (vgx_flatten
 *   writes them so) set VGX_E_INVALID_ARG. With any status but VGX_OK no vertex and no index is written. Host return values:
 *   VGX_E_INVALID_ARG for null pointers and for the misalignments vgx_mesh_out names, VGX_E_RANGE for ndraws >= 2^32 - 1. Ends a counted
 *   state, like vgx_concave_emit. */
int vgx_concave_contours(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                         const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- concave fills to TRIANGLES on the device (beyond the reference): vgx_flatten -> vgx_concave_triangulate -> vgx_merge ----------------
 * A contour mesh is understood by vgx_raster_concave and vgx_pick_frame alone. vgx_concave_triangulate is vgx_concave_contours with one
 * difference: a concave draw that is ONE simple closed ring (an arrow, a star, an L, a notch) comes out as triangles, by ear clipping on
 * the device, under the rule below. Every other mesh-making draw comes out exactly as vgx_concave_contours writes it, at its place in the
 * same dense output, so the frame is always drawable; draw_route says which draws are triangles. Holes, multi-contour fills and
 * self-intersecting rings are out of scope: they stay with the contour route or with libtess2.
 * Inputs, alignment, host return values, "which draws make meshes", the dev_sizes / dev_status protocol (VGX_E_NOSPACE with the exact
 *   need and nothing written past a capacity; with any status but VGX_OK no vertex and no index is written; VGX_E_INVALID_ARG for
 *   sub-paths that do not lie back to back), ascending dense output (sequence `b` of vgx_merge as it stands), asynchronous and
 *   stream-ordered with no host round trip, ends a counted state: vgx_concave_contours' word for word.
 * draw_route (DEVICE [ndraws], 4-byte aligned, may be NULL) receives per draw: 0 = the draw makes no mesh, VGX_TRI_ROUTE_TRIANGLES = it
 *   was triangulated, or the reason it was refused (VGX_TRI_REFUSED_*): then the draw holds vgx_concave_contours' meshes. The routes
 *   depend on the input alone and are written whatever status the call ends with (VGX_E_INVALID_ARG aside).
 * The ring R. Without VGX_FILL_AA: the draw's polyline vertices. With VGX_FILL_AA: the moved ring, the vertices vgx_concave_move gives
 *   (the inner fringe vertices), which is what the reference triangulates in its step (3). An inset can cross itself where the input does
 *   not: such a draw is refused and gets the AA pair of the contour route. V = its vertex count. Refusals, tested in this order:
 *   MULTI       the draw has more than one sub-path;
 *   TOO_LONG    V > VGX_TRIANGULATE_MAX_VERTICES (the kernel holds R in LDS: 8 bytes of position and two 16-bit links per vertex);
 *   NONFINITE   a coordinate of R is not finite;
 *   DEGENERATE  the orientation s is 0;
 *   NOT_SIMPLE  two edges of R meet;
 *   STALLED     the clipping loop found no ear in a whole turn.
 * The rule. c(a, b, p) = the canonical edge value E of a -> b at p exactly as the winding rule of vgx_raster_concave defines it:
 *   coordinates widened to binary64, no FMA, lo and hi ordered by (x, then y), 0 when a == b bit for bit.
 *   Orientation. k = the vertex of R that is smallest by (x, y, index); s = sign of c(prev k, k, next k).
 *   Simplicity. Every pair of edges (u1 -> v1, u2 -> v2) of R that share no vertex index (V = 3 has none) MEETS when c(u1,v1,u2) and
 *     c(u1,v1,v2) have strictly opposite signs and c(u2,v2,u1) and c(u2,v2,v1) have strictly opposite signs, or when one of the four
 *     values is 0 and that endpoint lies in the closed coordinate box of the other edge. One pair that meets refuses the ring. This is
 *     conservative -- a ring that touches itself is refused -- while collinear edges that do not overlap pass (a comb is triangulated).
 *   Clipping. R is a doubly linked ring; the cursor b starts at vertex 0, misses = 0. While more than three vertices remain:
 *     a = prev b, c = next b, t = s * c(a, b, c). b is an EAR when t == 0 (a flat ear, no containment test), or when t > 0 and no vertex
 *     p still linked in the ring, other than a, b, c, has s * c(a,b,p) >= 0 && s * c(b,c,p) >= 0 && s * c(c,a,p) >= 0. On an ear: emit
 *     the triangle (a, b, c), unlink b, b = next c, misses = 0. Otherwise b = c and misses grows by one; when it exceeds the number of
 *     vertices still linked the draw is STALLED. The last three vertices are emitted as (prev b, b, next b).
 *   So a triangulated ring always has V vertices and 3 (V - 2) indices, and its triangles' directed boundary telescopes to the ring:
 *   by the winding rule's own words (opposite edges cancel exactly; a triangle's three edges give its coverage) vgx_raster_concave
 *   draws every sample of the triangles exactly as often as it draws it for the contour mesh of the same ring.
 * What a triangulated draw writes. ONE mesh of kind VGX_MESH_CONCAVE_FILL_AA (what vgx_concave_emit gives, also for a fill of zero
 *   boundary contours), draw = d. Without AA: the V polyline vertices in order, every colour fill_color, the 3 (V - 2) mesh-local
 *   indices in emission order. With AA, in vgx_concave_emit's layout: 2V fringe vertices and 6V indices, bit for bit vgx_concave_emit's
 *   fringe (strokerConcaveFillEndAA's), then the interior: the V moved vertices, colour fill_color, and the 3 (V - 2) indices rebased
 *   by 2V. 3V > 65536 sets VGX_E_MESH_TOO_LARGE; a refused draw sets it as vgx_concave_contours does.
 * Scratch (the context's buffer list, vgx_scratch_bytes counts it): 36 bytes per draw and 6 bytes per vertex of
 *   min(out->cap_vertices, ndraws * VGX_TRIANGULATE_MAX_VERTICES). */
#define VGX_TRIANGULATE_MAX_VERTICES 4096u
enum { VGX_TRI_ROUTE_TRIANGLES = 1, VGX_TRI_REFUSED_MULTI = 2, VGX_TRI_REFUSED_TOO_LONG = 3, VGX_TRI_REFUSED_NONFINITE = 4,
       VGX_TRI_REFUSED_DEGENERATE = 5, VGX_TRI_REFUSED_NOT_SIMPLE = 6, VGX_TRI_REFUSED_STALLED = 7 };
int vgx_concave_triangulate(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                            const vgx_mesh_out* out, uint32_t* draw_route /* DEVICE [ndraws], may be NULL */, vgx_sizes* dev_sizes, uint32_t* dev_status,
                            void* stream);

/* ---- fills with HOLES to triangles on the device: vgx_flatten -> vgx_concave_triangulate_rings -> vgx_merge -----------------------------
 * vgx_concave_triangulate_rings is vgx_concave_triangulate for draws of several sub-paths that are ONE outer ring with any number of
 * holes directly inside it (a donut, a frame, a gear, the counters of a letter). Inputs, alignment, host return values, "which draws
 * make meshes", the dev_sizes / dev_status protocol, ascending dense output (sequence `b` of vgx_merge), draw_route, asynchronous and
 * stream-ordered with no host round trip, ends a counted state: vgx_concave_triangulate's word for word. A draw with ONE sub-path gets
 * exactly the route, mesh record, vertices and indices vgx_concave_triangulate gives it; a refused draw gets vgx_concave_contours'
 * meshes. VGX_TRI_REFUSED_MULTI is never returned. Islands inside holes, separate outlines and rings that touch stay with the contour
 * route or with libtess2.
 * The rule for a draw of S >= 2 sub-paths. c(a, b, p) and MEETS are those of vgx_concave_triangulate. The rings are the draw's
 *   sub-paths: the polyline vertices, with VGX_FILL_AA the vertices vgx_concave_move gives for every contour. V = their total vertex
 *   count, the vertices numbered 0 .. V - 1 in sub-path order; prev / next of a vertex are taken inside its ring; H = S - 1.
 *   Refusals, tested in this order:
 *   TOO_LONG    V + 2 H > VGX_TRIANGULATE_MAX_VERTICES;
 *   NONFINITE   a coordinate is not finite;
 *   DEGENERATE  the orientation s_r of some ring r is 0: k = the ring's smallest vertex by (x, y, index), s_r = sign c(prev k, k, next k);
 *   NOT_SIMPLE  two edges u -> next u of the draw that have no vertex index in common MEET, of one ring or of two;
 *   NESTING     the rings are not one outer ring with holes directly inside it. The outer ring o owns the draw's smallest vertex by
 *               (x, y, index); s = s_o. Every other ring h is a hole with bridge vertex m_h, its GREATEST vertex by (x, y, index).
 *               Without VGX_FILL_EVEN_ODD a hole needs s_h = -s; with it any orientation passes. inside(p, r) = the parity of the
 *               number of edges u -> v of ring r with (u.y <= p.y) != (v.y <= p.y) and sign c(u, v, p) == sign (v.y - u.y). Every m_h
 *               must be inside o and outside every other hole;
 *   NO_BRIDGE   a hole finds no bridge (below);
 *   STALLED     as in vgx_concave_triangulate.
 *   Slots. The merged ring is a doubly linked ring of SLOTS: slot i < V is vertex i; slots V + 2 j and V + 2 j + 1 are second copies of
 *     the two bridge ends of the j-th processed hole (j from 0). A slot's position is its vertex's. The merged ring starts as ring o.
 *   Bridges. The holes are processed in DESCENDING order of m_h by (x, y, index). For hole h with M = m_h a CANDIDATE is a slot q of the
 *     merged ring as it stands with: (position) q.x > M.x, or q.x == M.x and q.y > M.y; (cone) with a = prev q, n = next q in the merged
 *     ring, t = s c(a,q,n), e1 = s c(a,q,M), e2 = s c(q,n,M): t > 0 ? (e1 > 0 && e2 > 0) : (e1 > 0 || e2 > 0); (visibility) the segment
 *     M -> q MEETS no edge of any ring of the draw and no earlier bridge, those that have vertex M or q's vertex as an end aside. The
 *     bridge goes to the candidate smallest by (d2, slot), d2 = dx * dx + dy * dy in binary64 from the widened coordinates, no FMA. No
 *     candidate: NO_BRIDGE. The splice: q -> M -> h's vertices (forwards, by next, when s_h = -s; else backwards) -> slot V + 2 j (M
 *     again) -> slot V + 2 j + 1 (q's vertex again) -> the old next q.
 *   Clipping. vgx_concave_triangulate's loop over the N = V + 2 H slots, the cursor starting at slot 0, with one amendment: a slot whose
 *     position compares equal in both coordinates to that of a, b or c does not block an ear.
 * Why the image is the same. Each bridge is walked once in each direction, and opposite edges cancel exactly; every emitted triangle
 *   has s c >= 0; the rings' winding is 0 or s everywhere (under even-odd with a hole traversed backwards the PARITY is that of the
 *   rings). So every sample is covered by at most one triangle, and exactly where the contour mesh covers it.
 * What a triangulated draw writes. ONE mesh of kind VGX_MESH_CONCAVE_FILL_AA: the V vertices in order (with AA, first the 2V fringe
 *   vertices and 6V fringe indices of vgx_concave_contours / vgx_concave_emit for all contours, then the V moved vertices), and
 *   3 (V + 2 H - 2) indices in emission order, each slot replaced by its vertex (rebased by 2V with AA).
 * Scratch (the context's buffer list): 36 bytes per draw and 6 bytes per SLOT of min(5 / 3 out->cap_vertices, ndraws *
 *   VGX_TRIANGULATE_MAX_VERTICES): a draw has fewer than V / 3 holes, so fewer than 5 V / 3 slots. */
enum { VGX_TRI_REFUSED_NESTING = 8, VGX_TRI_REFUSED_NO_BRIDGE = 9 };
int vgx_concave_triangulate_rings(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                  const vgx_mesh_out* out, uint32_t* draw_route /* DEVICE [ndraws], may be NULL */, vgx_sizes* dev_sizes, uint32_t* dev_status,
                                  void* stream);

/* ---- SEVERAL OUTLINES and ISLANDS IN HOLES to triangles: vgx_flatten -> vgx_concave_triangulate_nested -> vgx_merge ---------------------
 * vgx_concave_triangulate_nested is vgx_concave_triangulate_rings for draws whose sub-paths are any number of outlines, each with holes,
 * each hole with islands, and so on (a word converted to outlines, "i", "%", a target, a gear with a hub). Such a draw is a disjoint
 * union of draws the rings entry triangulates: the rings are classified by containment depth, cut into GROUPS of one even-depth ring
 * and the odd-depth rings directly inside it, and every group is triangulated by the rings rule. Inputs, alignment, host return values,
 * "which draws make meshes", the dev_sizes / dev_status protocol, ascending dense output (sequence `b` of vgx_merge), draw_route,
 * asynchronous and stream-ordered with no host round trip, ends a counted state: vgx_concave_triangulate_rings' word for word. A draw
 * with ONE sub-path gets vgx_concave_triangulate's words; a refused draw gets vgx_concave_contours' meshes. No new route code.
 * The rule for a draw of S >= 2 sub-paths. c, MEETS, inside(p, r), the rings (moved with VGX_FILL_AA), V, m_r (the GREATEST vertex of
 *   ring r by (x, y, index)) and s_r are those of the two sections above. Refusals, tested in this order:
 *   TOO_LONG    V + 2 (S - 1) > VGX_TRIANGULATE_MAX_VERTICES: the rings entry's test, known without geometry; it bounds the slots of
 *               any grouping;
 *   NONFINITE, DEGENERATE, NOT_SIMPLE   as in the rings entry, over the whole draw, pairs of edges of different groups included;
 *   NESTING     the containment is not a forest this rule can use. C(r) = { r' != r : inside(m_r, r') }, depth(r) = |C(r)|. For
 *               depth(r) > 0, parent(r) is the ring of C(r) whose depth is depth(r) - 1: not exactly one such ring is NESTING. A ring of
 *               even depth is the OUTER ring of a group, in any orientation under either fill rule; a ring of odd depth is a HOLE of its
 *               parent's group. Without VGX_FILL_EVEN_ODD a hole needs s_h = -s_parent, else NESTING (at depth 1 as at depth 3);
 *   NO_BRIDGE, STALLED   the refusal of the lowest-numbered group that has one.
 *   Groups are numbered ascending by the sub-path index of their outer ring; G = their number, H_g = the holes of group g, B_g = the
 *     holes of the groups before g. Group g goes through the rings entry's Slots / Bridges / Clipping with: "the draw's rings" = the
 *     group's rings; o = the group's outer ring, s = s_o; its vertex slots are its rings' vertices; the two bridge slots of its j-th
 *     processed hole are V + 2 (B_g + j) and V + 2 (B_g + j) + 1; the cursor starts at the group's lowest slot; in the visibility test
 *     and in the ear test "every slot / edge / earlier bridge" ranges over the GROUP's slots only. A group of one ring is clipped by
 *     vgx_concave_triangulate's loop, with no amendment and the cursor at its first vertex.
 *   So the triangles of a group are the ones vgx_concave_triangulate_rings gives a draw made of that group's sub-paths alone, in their
 *   order, with the indices translated; and a draw with G = 1 gets the rings entry's bytes.
 * Why the image is the same. Inside a group, bridges cancel and the triangles telescope to the group's rings (the rings section); a
 *   group's region -- inside its outer ring, outside its holes -- has winding 0 or s_o (parity under even-odd). No two edges of the
 *   draw meet, so rings nest or lie apart, and the regions of two groups are disjoint: an island lies in a hole of the group around it.
 *   The draw's winding (or parity) is non-zero exactly on the union of the groups' regions. So every sample is covered by at most one
 *   triangle, and exactly where the contour mesh covers it.
 * What a triangulated draw writes. ONE mesh of kind VGX_MESH_CONCAVE_FILL_AA: the V vertices in order (with AA behind the 2V fringe
 *   vertices and 6V fringe indices of all contours, exactly as the rings entry writes them), then the triangles group after group, each
 *   group's V_g + 2 H_g - 2 in emission order: 3 (V + 2 S - 4 G) indices in all.
 * Scratch (the context's buffer list): the rings entry's -- 36 bytes per draw and 6 bytes per SLOT of min(5 / 3 out->cap_vertices,
 *   ndraws * VGX_TRIANGULATE_MAX_VERTICES) -- and 4 bytes per draw for G. */
int vgx_concave_triangulate_nested(vgx_ctx* ctx, const float* poly, const vgx_subpath* subpaths, const vgx_draw_info* draw_info, const vgx_draw* draws, uint64_t ndraws,
                                   const vgx_mesh_out* out, uint32_t* draw_route /* DEVICE [ndraws], may be NULL */, vgx_sizes* dev_sizes, uint32_t* dev_status,
                                   void* stream);

/* ---- merging external meshes into a frame -----------------------------------------------------------------
 * The reference appends every mesh to the frame in submission order (createDrawCommand_VertexColor, src/vg.cpp:5207-5244).
 * vgx_merge builds that order from two mesh sequences that are each sorted by draw: `a` = what vgx_tessellate[_emit] wrote for
 * the frame's draws, `b` = meshes built elsewhere for draws that have none in `a` (concave fills: vgx_concave_emit), with
 * b_draw[j] (DEVICE, may be NULL: b->meshes[j].draw) = the frame draw of b's mesh j. Output = both sequences interleaved by draw
 * index (a mesh of `a` before a mesh of `b` of the same draw), streams copied, mesh records renumbered (first_vertex /
 * first_index = the merged offsets, draw = the frame draw). Honours vgx_set_assembly like vgx_tessellate does (`draws` / ndraws:
 * the frame's draw records, DEVICE, only read for VGX_ASM_SPLIT_STATE; may be NULL otherwise). All pointers are DEVICE pointers;
 * the num_* members of `a` / `b` are host values. Asynchronous (capacities checked on the device, totals in dev_sizes, status in
 * dev_status); a sequence that is not sorted by draw sets VGX_E_INVALID_ARG.
 * `b` may have HOLES: its meshes are read one by one through first_vertex / first_index, so vertices and indices that no mesh of `b`
 * owns may lie between them (vgx_text_quads writes runs at caller-chosen places); they are not copied. The output is packed. */
int vgx_merge(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const vgx_draw* draws, uint64_t ndraws,
              const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);
/* The same with per-vertex UVs for the meshes of `b` (user meshes with texture coordinates): b_uv (DEVICE, [b->num_vertices] x the
 * armed assembly's uv_bytes, or NULL) overwrites the white-pixel UV the assembly step writes for every vertex. Needs an armed
 * assembly with a UV stream to have an effect. */
int vgx_merge_uv(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const void* b_uv, const vgx_draw* draws, uint64_t ndraws,
                 const vgx_mesh_out* out, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);
/* vgx_merge with a UV stream of the caller's beside pos / color, for the calls that read one without draw-command assembly
 * (vgx_raster_textured): b_uv (DEVICE, [b->num_vertices][uv_bytes]) is copied to out_uv (DEVICE, [out->cap_vertices][uv_bytes]) at
 * the merged places of the vertices of b's meshes; out_uv is written nowhere else (the vertices of a's meshes keep what they held:
 * no sampled mesh is among them). uv_bytes is 4 or 8. The call ignores vgx_set_assembly for the UV stream: an armed assembly does
 * its part as in vgx_merge, but its own UV stream is neither written nor read here. VGX_E_INVALID_ARG for a null b_uv or out_uv,
 * another uv_bytes, or pointers that are not 4-byte aligned. */
int vgx_merge_uv_stream(vgx_ctx* ctx, const vgx_cache_desc* a, const vgx_cache_desc* b, const uint32_t* b_draw, const void* b_uv, uint32_t uv_bytes,
                        const vgx_draw* draws, uint64_t ndraws, const vgx_mesh_out* out, void* out_uv, vgx_sizes* dev_sizes, uint32_t* dev_status,
                        void* stream);

/* ---- text: the device half of renderTextQuads (src/vg.cpp:5541-5621) ------------------------------------------
 * Glyph layout and the atlas (FontStash + stb_truetype) stay with the caller, as libtess2 does for concave fills. What the
 * reference does AFTER FontStash produced the glyph quads of a string is done here for a batch of strings ("runs"):
 *   the matrix: ctxText's pushState + transformTranslate(x + dx / scale, y + dy / scale) (:4228-4229, 4055-4062), then the inverse
 *     font scale folded into m[0..3] (1.0f / scale, :5545-5558);
 *   vgutil::batchTransformTextQuads (src/vg_util.cpp:332-445): corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) through transformPos2D;
 *   the colour replicated (memset32, :5575), the UVs (s0,t0) (s1,t0) (s1,t1) (s0,t1) as float pairs or as
 *     (int16_t)(s * INT16_MAX) pairs (:5577-5613; truncation towards zero, defined for the 0..1 FontStash produces);
 *   vgutil::genQuadIndices_unaligned (vg_util.cpp:275-330): b, b+1, b+2, b, b+2, b+3 with b = 4 * (quad - first_quad), mesh-local.
 * One run = one renderTextQuads call = one ctxText = one mesh; a TextBox is one run per row (ctxTextBox, :4234-4271).
 * The PLACES of a run's vertices and indices are the caller's: a frame's external meshes (`b` of vgx_merge_uv) are one sequence
 * sorted by draw that may hold user meshes (vgx_cmdlist_out::tri_*) and text runs in any order; the sizes of both are known on
 * the host (4 and 6 per quad), so the host lays the sequence out and each producer writes at its places.
 * Not done here: shaping, the atlas and its growth, measureText*, draw-command assembly (that stays vgx_merge_uv's job; this call
 * ignores vgx_set_assembly). */
typedef struct vgx_text_run {      /* one renderTextQuads call. 80 bytes */
	uint64_t first_quad;           /* into quads */
	uint32_t num_quads;            /* numBakedChars */
	uint32_t color;                /* colour with the global alpha already folded in (vgx_text_cmd::color) */
	float mtx[6];                  /* State::m_TransformMtx at the Text command (vgx_text_cmd::mtx) */
	float x, y;                    /* ctxText's x, y (TextBox: the row's) */
	float dx, dy;                  /* fonsAlignString's result */
	float scale;                   /* State::m_FontScale * devicePixelRatio (vgx_text_cmd::scale) */
	uint32_t draw;                 /* frame draw of the Text command -> vgx_mesh.draw */
	uint64_t first_vertex;         /* where the mesh goes in out->pos / color (and out_uv); 4 * num_quads vertices */
	uint64_t first_index;          /* where its 6 * num_quads indices go in out->idx */
} vgx_text_run;
/* quads: DEVICE [nquads][8] = FONSquad in its FONS_QUAD_SIMD layout {x0, y0, x1, y1, s0, t0, s1, t1}, 16-byte aligned.
 * runs: DEVICE [nruns], in quad order without overlap (runs[r + 1].first_quad >= runs[r].first_quad + runs[r].num_quads, the last
 * one ending inside nquads; else VGX_E_INVALID_ARG in dev_status, the places of the runs then hold undefined data and nothing
 * outside them is touched); quads between runs are ignored. out_uv: DEVICE
 * [out->cap_vertices][uv_bytes] or NULL; uv_bytes 0 (none), 4 (int16 x 2) or 8 (float x 2).
 * One vgx_mesh per run at out->meshes[first_mesh + r] (out->meshes may be NULL): the run's places, 4 n / 6 n, its draw,
 * subpath_kind = VGX_MESH_TEXT << 28; a run of zero quads writes an empty record. Asynchronous like vgx_concave_emit / vgx_cache_submit
 * (capacities checked on the device, nothing written past one, no host round trip). dev_status: a run of more than 16 384 quads sets
 * VGX_E_MESH_TOO_LARGE (the reference VG_CHECKs a command's vertex count, vg.cpp:5323; the uint16 indices would wrap), a place
 * beyond a capacity VGX_E_NOSPACE, a non-finite matrix or scale (0 included) VGX_E_NONFINITE; such a run writes no vertex and no
 * index (its record says 0 / 0), the others are written (also one whose RECORD has no room in out->meshes). dev_sizes: num_meshes = first_mesh + nruns, num_vertices / num_indices =
 * the capacities the placement needs (the highest end of a run: the totals for a dense layout), num_elements = quads in runs. */
int vgx_text_quads(vgx_ctx* ctx, const float* quads, uint64_t nquads, const vgx_text_run* runs, uint64_t nruns, uint64_t first_mesh,
                   const vgx_mesh_out* out, void* out_uv, uint32_t uv_bytes, vgx_sizes* dev_sizes, uint32_t* dev_status, void* stream);

/* ---- command-list byte-code as input ---------------------------------------------
 * vg::CommandList::m_CommandBuffer as the reference's cl* functions write it (src/vg.cpp:243-247, 2403-2690, 5694-5723):
 * {CommandHeader{uint32 type, uint32 size}, 16-byte aligned}{payload, 16-byte aligned}... in HOST memory.
 * vgx_cmdlist_decode replays it the way ctxSubmitCommandList does (:4273-4637) into what the batch entry points take: one
 * path per BeginPath group (vgx_pathset_desc arrays) and one vgx_draw per fill / stroke command -- all six of them:
 * FillPathColor / Gradient / ImagePattern (ctxFillPath*, :3061-3399), StrokePathColor / Gradient / ImagePattern
 * (ctxStrokePath*, :3401-3668) -- with the interpreter's state folded in: transform stack (PushState / PopState /
 * Transform* / SetViewBox, :3934-4122; the transform is latched at the path's first fill / stroke like transformPath
 * :4957-4975), global alpha, stroke width scaling / clamping / Thin switch, scissor (per draw, vgx_draw_state), clip
 * regions (BeginClip / EndClip / ResetClip, :3670-3709: the draws recorded inside are non-AA black DrawCommand::Type::Clip
 * draws), gradients and image patterns created by the list (vgx_paint records, :3711-3932), command culling
 * (CommandListFlags::AllowCommandCulling), and nested lists (SubmitCommandList, :4611-4620, through `lists`).
 * vgx_draw::state_key = generation << 20 | DrawCommand::Type << 16 | handle: what allocDrawCommand / allocClipCommand
 * compare before merging (:5359-5460); the generation changes whenever the reference sets m_ForceNewDrawCommand /
 * m_ForceNewClipCommand between two draws (scissor changes, PopState onto a different scissor, EndClip, ResetClip).
 * Concave fills (PathType::Concave) become draws with VGX_FILL_CONCAVE [| VGX_FILL_AA] [| VGX_FILL_EVEN_ODD] and no
 * VGX_FILL_ENABLE: vgx_tessellate makes no mesh for them, the caller builds it (vgx_flatten -> vgx_concave_contours, or vgx_flatten_* -> libtess2 -> vgx_concave_move /
 * vgx_concave_emit) and vgx_merge puts it at the draw's place in the frame.
 * IndexedTriList commands become draws with VGX_FILL_TRILIST; their meshes come back in vgx_cmdlist_out::tri_*.
 * Commands without an equivalent here are counted in num_skipped and otherwise ignored: Text / TextBox (vgx_cmdlist_decode_text
 * below turns them into draws), path commands issued after a path's first fill / stroke
 * without a new BeginPath (the reference VG_CHECKs this, :2984-3059), nested lists without a table entry.
 * Host only, no device needed; re-entrant (no shared state between calls). `bytes` must be 4-byte aligned (the reference's
 * buffers are 16-byte aligned). Call with the array members NULL to get the counts, allocate, call again. */
typedef struct vgx_cmdlist_ref {   /* one vg::CommandList, addressed by CommandListHandle::idx (SubmitCommandList) */
	const void* bytes;             /* HOST CommandList::m_CommandBuffer */
	uint32_t size;                 /* m_CommandBufferPos */
	uint32_t flags;                /* m_Flags (VGX_CL_*) */
} vgx_cmdlist_ref;
enum { VGX_CL_CACHEABLE = 1u,      /* CommandListFlags::Cacheable: fills / strokes ignore the global alpha and transparent
                                    * colours are not dropped while the list populates its cache (hasCache, :3063-3075) */
       VGX_CL_ALLOW_CULLING = 2u, /* CommandListFlags::AllowCommandCulling (:4299-4300, 4548-4577) */
       VGX_CL_UV_FLOAT = 0x200u,  /* not a reference flag: the build's uv_t is float (VG_CONFIG_UV_INT16 = 0, include/vg/vg.h:27-29): IndexedTriList payloads
                                    * carry 8 bytes of UV per vertex instead of 4 */
       VGX_CL_SCISSOR_SET = 0x100u };/* not a reference flag: vgx_cmdlist_state::scissor holds a rectangle even when it is all zero (a real
                                    * empty scissor left by an earlier list of the frame); set it when chaining vgx_cmdlist_out::end_scissor */
typedef struct vgx_cmdlist_state { /* the Context / State values at submission */
	float mtx[6];          /* State::m_TransformMtx */
	float global_alpha;    /* State::m_GlobalAlpha */
	float tess_tol;        /* Context::m_TesselationTolerance */
	float fringe;          /* Context::m_FringeWidth */
	float canvas_width;    /* Context::m_CanvasWidth / Height (SetViewBox, scissor clamps) */
	float canvas_height;
	uint32_t flags;        /* VGX_CL_* of the list being decoded */
	float scissor[4];      /* State::m_ScissorRect; all zero WITHOUT VGX_CL_SCISSOR_SET in flags = {0, 0, canvas_width, canvas_height} (resetScissor) */
	uint32_t first_gradient;      /* Context::m_NextGradientID at submission (local handles are relative to it) */
	uint32_t first_image_pattern; /* Context::m_NextImagePatternID */
	uint32_t max_gradients;       /* Config::m_MaxGradients, 0 = 64 */
	uint32_t max_image_patterns;  /* Config::m_MaxImagePatterns, 0 = 64 */
	uint32_t max_depth;           /* Config::m_MaxCommandListDepth, 0 = 16 */
	uint32_t num_lists;           /* entries of `lists` */
	const vgx_cmdlist_ref* lists; /* HOST handle -> list table for SubmitCommandList; NULL: nested lists are skipped */
	uint16_t prev_cmd_scissor[4]; /* scissor of the frame's last draw command before this list (PopState rule, :3950-3965) */
	uint32_t prev_cmd_valid;      /* 0: the frame has no draw command yet */
	uint32_t first_generation;    /* generation of the first draw's state_key (chain successive decodes of one frame) */
	/* Context::m_ClipState / m_RecordClipCommands at submission: a clip region outlives the list that recorded it (vg.cpp:71-76,
	 * 3670-3709). All zero = no region. Indices are in the frame's draw numbering: this decode's draw i is draw draw_base + i. */
	uint32_t clip_valid;          /* 1: a region is active (m_ClipState.m_FirstCmdID != ~0) */
	uint32_t clip_rule;
	uint32_t clip_first_draw;
	uint32_t clip_num_draws;
	uint32_t clip_recording;      /* 1: submitted between BeginClip and EndClip */
	uint32_t draw_base;           /* draws decoded earlier in this frame */
	uint32_t white_uv[2];         /* getWhitePixelUV as raw words (one word with int16 UVs): the UV of IndexedTriList vertices that come without UVs (vg.cpp:4148-4156) */
	uint32_t font_image;          /* Context::m_FontImages[0].idx: the image an IndexedTriList with an invalid handle is drawn with (:4131-4133) */
} vgx_cmdlist_state;
typedef struct vgx_draw_state {   /* per draw: what allocDrawCommand copies into the DrawCommand (vg.cpp:5391-5400). 24 bytes */
	uint16_t scissor[4];          /* (uint16_t) State::m_ScissorRect */
	uint32_t clip_rule;           /* ClipState::m_Rule (0 In, 1 Out) */
	uint32_t clip_first_draw;     /* the active clip region = the draws of type Clip among [clip_first_draw, + clip_num_draws) of
	                               * this decode (the reference stores the range of clip COMMANDS they merge into; gradient and
	                               * image-pattern paints inside BeginClip .. EndClip are ordinary draws and may lie between
	                               * them); 0xFFFFFFFF = none. A draw recorded while the region is still open sees it empty
	                               * (clip_num_draws = 0), as in the reference (vg.cpp:3670-3697) */
	uint32_t clip_num_draws;
	uint32_t raw_color;           /* the Color operand of the fill / stroke command as recorded (0 for gradient paints): what a
	                               * replay from the shape cache uses for non-AA meshes (vgx_cache_instance::color) */
} vgx_draw_state;
typedef struct vgx_paint {        /* vg::Gradient / vg::ImagePattern as the Create* calls compute them (vg.cpp:84-96). 96 bytes */
	uint32_t type;                /* DrawCommand::Type of the draws that use it: 1 ColorGradient, 2 ImagePattern */
	uint32_t handle;              /* the id in the low 16 bits of those draws' state_key */
	float matrix[9];              /* m_Matrix */
	float params[4];              /* Gradient::m_Params {extent.x, extent.y, radius, feather} */
	float inner_color[4];
	float outer_color[4];
	uint32_t image;               /* ImagePattern::m_ImageHandle */
} vgx_paint;
typedef struct vgx_cmdlist_out {
	uint8_t* cmd_type;        /* HOST [cap_cmds]      -> vgx_pathset_desc.cmd_type */
	uint32_t* cmd_arg_off;    /* HOST [cap_cmds + 1] */
	float* args;              /* HOST [cap_args] */
	uint32_t* path_cmd_begin; /* HOST [cap_paths + 1] */
	vgx_draw* draws;          /* HOST [cap_draws]; vgx_draw.path indexes the paths produced here */
	vgx_draw_state* draw_state; /* HOST [cap_draws], may be NULL */
	vgx_paint* paints;        /* HOST [cap_paints], may be NULL */
	uint32_t cap_cmds, cap_args, cap_paths, cap_draws, cap_paints;
	uint32_t num_cmds, num_args, num_paths, num_draws, num_paints; /* out */
	uint32_t num_skipped;     /* out: commands without an equivalent in this path */
	uint32_t next_gradient;   /* out: Context::m_NextGradientID / m_NextImagePatternID after the list */
	uint32_t next_image_pattern;
	uint32_t next_generation; /* out: first_generation for the next decode of the same frame */
	float end_mtx[6];         /* out: State::m_TransformMtx / m_GlobalAlpha after the list (state changes of a list leak into
	                           * its caller unless VG_CONFIG_COMMAND_LIST_PRESERVE_STATE, vg.cpp:4323-4325) */
	float end_global_alpha;
	uint32_t end_clip_valid;  /* out: the clip state after the list, for the next decode's vgx_cmdlist_state::clip_* */
	uint32_t end_clip_rule, end_clip_first_draw, end_clip_num_draws, end_clip_recording;
	float end_scissor[4];     /* out: State::m_ScissorRect after the list (chain it with VGX_CL_SCISSOR_SET: it may be a real empty rectangle) */
	uint32_t reserved;
	/* IndexedTriList commands (user meshes, vg.cpp:4129-4175 / 4461-4477): one draw each (VGX_FILL_TRILIST, state_key = Textured |
	 * image) and the mesh in these HOST arrays, ready to be uploaded as a sequence for vgx_merge: positions through the state
	 * transform at the command (batchTransformPositions), one colour per vertex (a single colour replicated, :4160-4165), the
	 * command's UVs or the white-pixel UV, indices mesh-local; tri_meshes[k].draw = the draw's index in this decode,
	 * subpath_kind = VGX_MESH_TRILIST << 28. The count pass reports num_tri_*; a store pass over a list that holds such commands
	 * without these arrays (or with too small ones) returns VGX_E_NOSPACE -- never a frame with a mesh silently missing.
	 * tri_uv alone may be NULL (no UVs wanted). */
	float* tri_pos;           /* HOST [cap_tri_vertices][2] */
	uint32_t* tri_color;      /* HOST [cap_tri_vertices] */
	void* tri_uv;             /* HOST [cap_tri_vertices][4 or 8 bytes (VGX_CL_UV_FLOAT)] */
	uint16_t* tri_idx;        /* HOST [cap_tri_indices] */
	vgx_mesh* tri_meshes;     /* HOST [cap_tri_meshes] */
	uint32_t cap_tri_vertices, cap_tri_indices, cap_tri_meshes;
	uint32_t num_tri_vertices, num_tri_indices, num_tri_meshes; /* out */
} vgx_cmdlist_out;
int vgx_cmdlist_decode(const void* bytes, uint32_t size, const vgx_cmdlist_state* state, vgx_cmdlist_out* out);

/* The same interpreter with Text / TextBox commands (clText / clTextBox, vg.cpp:2914-2957; interpreter :4505-4533) as draws:
 * vgx_cmdlist_decode is this call with text = NULL. Each command that survives the reference's early-outs -- font_size * scale <
 * min_font_size (:4184, 4241), an empty string (:4189), colour alpha 0 after the global alpha (:5547-5550) -- becomes one vgx_draw
 * with VGX_FILL_TEXT and no VGX_FILL_ENABLE (no mesh from vgx_tessellate, like VGX_FILL_TRILIST), state_key = Textured | font_image
 * with the current generation, its vgx_draw_state record (scissor, clip) and one vgx_text_cmd; the ones dropped are neither draws nor
 * skipped. Text always folds the global alpha, also in a VGX_CL_CACHEABLE list; command culling does not touch it (:4338 skips the
 * six fill / stroke commands only); between BeginClip and EndClip it is an ordinary Textured draw (renderTextQuads calls
 * allocDrawCommand whatever m_RecordClipCommands says); a path being built is left alone. ctxText's own pushState / popState
 * restore the state they found and no scissor changes in between, so no generation changes. String ranges outside strings_size
 * return VGX_E_INVALID_ARG (the reference only VG_CHECKs, :4512-4513). Count pass with texts = NULL (num_texts), VGX_E_NOSPACE for
 * a too small array. Nested lists (SubmitCommandList) share `strings` with their parent here: offsets of a nested list's text
 * must be relative to the same buffer.
 * From a vgx_text_cmd to vgx_text_run records: the caller's shaper (fonsSetSize(font_size * scale), fonsBakeString,
 * fonsAlignString) makes the quads and dx / dy; a Text command is one run at (x, y); a TextBox is handed over whole -- the
 * shaper breaks the rows (textBreakLines) and makes one run per row with ctxTextBox's per-row x / y and the FONS_ALIGN_LEFT | valign
 * alignment (:4245-4267); the runs of one command share its draw, which vgx_merge accepts (non-decreasing b_draw).
 * Out of scope: shaping, the atlas and its growth (allocTextAtlas switches m_FontImageID mid-frame; a decode has ONE font_image,
 * a caller whose atlas grew rewrites the handle in the state_key of later text draws), measureText*, text inside a Cacheable
 * list's shape cache. */
typedef struct vgx_text_cmd {      /* one Text / TextBox command. 76 bytes */
	uint32_t draw;                 /* its draw in this decode */
	uint32_t kind;                 /* 0 Text, 1 TextBox */
	uint32_t font;                 /* TextConfig as recorded: m_FontHandle.idx, m_FontSize, m_Alignment */
	float font_size;
	uint32_t alignment;
	uint32_t color;                /* colorSetAlpha(cfg.color, (uint8_t)(globalAlpha * alpha)), vg.cpp:5547 */
	float x, y, break_width;       /* break_width: TextBox only */
	uint32_t textbox_flags;
	uint32_t string_offset, string_len; /* into CommandList::m_StringBuffer */
	float scale;                   /* State::m_FontScale (updateState's 0.1 quantisation, vg.cpp:4937-4942) * device_pixel_ratio */
	float mtx[6];                  /* State::m_TransformMtx at the command */
} vgx_text_cmd;
typedef struct vgx_cmdlist_text {
	const char* strings;           /* in: HOST CommandList::m_StringBuffer (only the ranges are checked, the bytes are not read) */
	uint32_t strings_size;         /* in: m_StringBufferPos */
	float device_pixel_ratio;      /* in: Context::m_DevicePixelRatio */
	float min_font_size;           /* in: VG_CONFIG_MIN_FONT_SIZE; 0 = 4.0 */
	vgx_text_cmd* texts;           /* out: HOST [cap_texts]; NULL = count */
	uint32_t cap_texts;            /* in */
	uint32_t num_texts;            /* out */
} vgx_cmdlist_text;
int vgx_cmdlist_decode_text(const void* bytes, uint32_t size, const vgx_cmdlist_state* state, vgx_cmdlist_out* out, vgx_cmdlist_text* text);

/* Diagnostics of the last asynchronous call on this context: the device status word and, when a kernel of
 * vgx_tessellate gave up, why (reason = one of the VGX_FAIL_* codes of csrc/vgx_internal_types.h: a table of
 * the kernel was too small for the batch -- run vgx_tessellate_count on a batch like it --, the polyline heap or the
 * caller's output capacity was exhausted, ...). Synchronises `stream`. Not needed on the happy path. */
typedef struct vgx_failure_info {
	uint32_t status;        /* vgx_status of the device status word */
	uint32_t reason;        /* 0 = none */
	uint32_t aux;           /* reason specific (a count) */
	uint32_t segment_items; /* (historic name) flatten kernel the last vgx_tessellate_count chose for batches like its own:
	                         * 0 = k_flatten_build (one lane per path command), 1 = k_flatten_inst, periodic draws, 2 = k_flatten_inst, draws
	                         * sorted by path, 3 = k_flatten_inst, draws sorted by (path, tolerance class) -- instances of different scales,
	                         * 4 = k_flatten_inst, periodic draws with the INSTANCES sorted by tolerance class, 5 = template mode (no flatten
	                         * per call), 6 = k_flatten_thin: like 0 for a path set of moveTo / lineTo / close paths only, whose polyline
	                         * layout was decided when the set was created */
	uint64_t segment;       /* work item (segment / task) that failed first */
	uint64_t prof[16];      /* -DVGX_INST_PROFILE builds of libvgx only (else 0): wave clock ticks (100 MHz) summed over all waves
	                         * per phase of k_flatten_inst (profiles/inst_phases.py) */
} vgx_failure_info;
int vgx_get_failure_info(vgx_ctx* ctx, vgx_failure_info* out, void* stream);

/* ---- multi-GPU: partition of a batch into contiguous draw ranges of about equal predicted output ----------------
 * "Partitioning: contiguous ranges of path instances per GPU ...; for heterogeneous batches balance on the count-pass result
 * (predicted out-verts)". Runs the flatten count pass over the whole batch (per-draw polyline vertex counts; no output buffers,
 * no mesh scratch), weights every draw with polyline vertices x output vertices per polyline vertex of its fill / stroke
 * flavour (+ 1), and cuts the draw sequence where the weight prefix crosses k / nparts of the total:
 *   out_bounds[0] = 0 <= out_bounds[1] <= ... <= out_bounds[nparts] = ndraws   (HOST, nparts + 1 entries)
 *   out_weights[k] = predicted weight of part k (HOST, nparts entries; may be NULL)
 * Rank r then tessellates draws [out_bounds[r], out_bounds[r + 1]); rank order = draw order, so the gathered streams are the
 * single-GPU result. Homogeneous batches (Tiger x K) come out as equal instance counts; when the draws repeat one sequence of
 * paths (a drawing submitted for many instances, at whatever scales) every cut falls BETWEEN instances, so that each part is
 * again a batch of whole instances for the instanced / template paths of vgx_tessellate. Synchronises the stream.
 * vgx_partition is a count call over the WHOLE batch: it replaces what an earlier vgx_tessellate_count left in the context
 * (scratch sizes, the instanced / template classification). Every rank calls vgx_tessellate_count on its own range afterwards. */
int vgx_partition(vgx_ctx* ctx, const vgx_pathset* ps, const vgx_draw* draws, uint64_t ndraws, uint32_t nparts, uint64_t* out_bounds, uint64_t* out_weights, void* stream);

/* ---- multi-GPU: gather of the per-rank streams to one root over RCCL / xGMI ---------------------------------
 * Independent path instances shard embarrassingly: one process per GPU, rank r tessellates a contiguous range of the
 * draws, no data-path collective. Indices are mesh-local, so the single-GPU result is the per-rank streams concatenated
 * in rank order; only the mesh table's first_vertex / first_index / draw need the rank's base added. This is the one
 * exchange step, for a C / C++ host that owns an RCCL communicator (`rccl_comm` is its ncclComm_t, created on the
 * context's device; librccl is bound at the first call from the library already loaded in the process, libvgx.so itself
 * has no link-time dependency on it). vg-renderer_amd/dist.py is the same layout over torch.distributed.
 *
 *   vgx_gather_sizes  all-gathers the four per-rank totals on the device (ncclAllGather of 4 x uint64 through context
 *                     scratch) and copies them to `all` (HOST, [nranks], rank order). Synchronises `stream`. Batches that
 *                     keep their shape from frame to frame call it once.
 *   vgx_gather        enqueues on `stream`, without any host synchronisation: on every other rank four ncclSend (positions,
 *                     colours, indices, mesh table) to `root`; on the root the matching ncclRecv straight into `global` at
 *                     each rank's offset, all inside ONE group (each peer -> root transfer rides its own xGMI link), a
 *                     device-to-device copy of the root's own block, and the rebase of the gathered mesh table (one
 *                     kernel). `global` is only read on the root (capacities checked against the totals: VGX_E_NOSPACE).
 *                     To overlap the gather of frame i with the tessellation of frame i + 1, call it on a second stream
 *                     with double-buffered outputs: nothing in it touches context scratch that vgx_tessellate uses.
 *                     Transfers go out in pieces of at most VGX_GATHER_CHUNK_MB (default 256 MiB), one group per piece. The
 *                     piece size is part of the wire protocol (sender and root cut a stream the same way) and is read once
 *                     per process from the environment: it must be the same on every rank; vgx_gather_sizes compares the
 *                     ranks' values and returns VGX_E_INVALID_ARG when they differ.
 * Errors: VGX_E_NO_DEVICE when no RCCL library can be bound, VGX_E_HIP when an RCCL call fails (vgx_last_hip_error() then
 * holds 10000 + the ncclResult_t). */
typedef struct vgx_rank_sizes { uint64_t num_vertices, num_indices, num_meshes, num_draws; } vgx_rank_sizes;
int vgx_gather_sizes(vgx_ctx* ctx, void* rccl_comm, const vgx_rank_sizes* mine, vgx_rank_sizes* all, void* stream);
int vgx_gather(vgx_ctx* ctx, void* rccl_comm, int root, const vgx_mesh_out* local, const vgx_rank_sizes* all, const vgx_mesh_out* global, void* stream);
/* vgx_gather with explicit placement: rank r's block (all[r] elements of `local` on rank r) lands at place[r] in `global` --
 * {num_vertices, num_indices, num_meshes} = first vertex / index / mesh of the block, num_draws = what is added to the `draw`
 * of its mesh records (vgx_gather = the exclusive prefix of `all`). This is what a frame tessellated in TILES needs: a rank cuts
 * its draws into sub-batches, tessellates tile t into the local buffers behind tile t - 1 and gathers tile t (local = a view of
 * the tile's part of the buffers, place = the rank's base + the tiles in front) on a second stream while tile t + 1 is being
 * tessellated -- the gathered frame is the same bytes, in the same order. Messages larger than VGX_GATHER_CHUNK_MB (default
 * 256 MiB) are split into pieces, one RCCL group per piece index. Capacities are checked against place + all. */
int vgx_gather_at(vgx_ctx* ctx, void* rccl_comm, int root, const vgx_mesh_out* local, const vgx_rank_sizes* all, const vgx_rank_sizes* place,
                  const vgx_mesh_out* global, void* stream);

/* Static batches (default off; also VGX_TMPL_BATCH=1). The caller promises that the batches it submits between two vgx_tessellate_count
 * calls keep their STRUCTURE -- the same paths with the same fill / stroke styles, widths, scale, tolerance and fringe at the same
 * positions of the draw list -- and only move transforms, colours and state keys: the draw list a retained scene produces frame after
 * frame (vg::submitCommandList of an unchanged list under a new camera; an instanced scene after culling, whose draws no longer repeat
 * a period). vgx_tessellate_count then flattens the whole draw list ONCE, in local space (the reference flattens before transformPath,
 * src/vg.cpp:4957-4975), and keeps it as one template (vgx_tmpl.hip: local polyline, mesh and element tables: ~30 bytes per output
 * vertex of device memory); vgx_tessellate is then ONE kernel per call -- every draw record verified against the counted one,
 * transformPos2D, the stroker -- instead of flatten + scans + fill + stroke. A structural change ends the call with VGX_E_STALE
 * (nothing usable in the buffers): count again. Batches above 2^29 vertices or 2^31 indices / elements keep the ordinary pipeline.
 * Results are the same bytes either way. */
int vgx_set_static_batches(vgx_ctx* ctx, int enable);

/* Per-kernel timing of the last vgx_tessellate.. / vgx_flatten.. sequence, measured with HIP events
 * on the stream the kernels ran on. Enable before the call; read after synchronising. */
#define VGX_MAX_STAGES 16
typedef struct vgx_stage_times {
	uint32_t num_stages;
	float ms[VGX_MAX_STAGES];
	const char* name[VGX_MAX_STAGES];
} vgx_stage_times;
int vgx_set_profiling(vgx_ctx* ctx, int enable);
int vgx_get_stage_times(vgx_ctx* ctx, vgx_stage_times* out);
/* The same, averaged over the last `ncalls` profiled calls of this context (at most VGX_PROF_RING, and only calls with the
 * same stage sequence as the last one): a caller that times K back-to-back calls reads the per-kernel durations of those
 * very calls afterwards, without having synchronised between them. Read after synchronising. */
#define VGX_PROF_RING 32
int vgx_get_stage_times_avg(vgx_ctx* ctx, vgx_stage_times* out, uint32_t ncalls);

#ifdef __cplusplus
}
#endif
#endif /* VGX_H */
