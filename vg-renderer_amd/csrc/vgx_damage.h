// vgx_damage.h -- the damage bitmap of vgx_damage_meshes / vgx_damage_instances / vgx_raster_damaged (include/vgx.h): host + device.
// One bit per 16 x 16 tile of the image, tile (tx, ty) = bit ty * tilesW + tx, the numbering of the raster's bin keys. The kernels
// of vgx_damage.hip and vgx_raster.hip and the loops of vgx_hosttest.cpp run the same functions.
#ifndef VGX_DAMAGE_H
#define VGX_DAMAGE_H

#include "vgx_raster.h"

VGX_HD uint32_t vgx_damage_tiles_w(uint32_t width) { return (width + VGX_RASTER_TILE - 1) / VGX_RASTER_TILE; }

// The tiles the box (one vgx_mesh_bounds record) reaches in an image of width x height at origin (x0, y0): the raster's span rule
// over the whole image, whatever the scissor, the kind or the index count. false: none (empty box, outside, a NaN bound)
VGX_HD bool vgx_damage_box_tiles(const float* box, int32_t x0, int32_t y0, uint32_t width, uint32_t height, VgxRasterRect* r)
{
	uint32_t i0, i1, j0, j1;
	if (!vgx_raster_span(box[0], box[2], x0, 0u, width, &i0, &i1) || !vgx_raster_span(box[1], box[3], y0, 0u, height, &j0, &j1)) { return false; }
	r->tx0 = i0 / VGX_RASTER_TILE; r->tx1 = i1 / VGX_RASTER_TILE; r->ty0 = j0 / VGX_RASTER_TILE; r->ty1 = j1 / VGX_RASTER_TILE;
	return true;
}

// bits lo .. hi (inclusive, < 32) of a word
VGX_HD uint32_t vgx_tile_word_mask(uint32_t lo, uint32_t hi) { return (0xFFFFFFFFu >> (31u - hi)) & (0xFFFFFFFFu << lo); }

// The tiles of rectangle r in a bitmap of one bit per tile: a row's tiles are consecutive bits, so orWord(word, mask) is called once per
// word of 32, not per tile (the device ORs atomically, the host plainly). The rectangle lies inside the image: every bit < tiles
template <class Or>
VGX_HD void vgx_tile_rect_words(const VgxRasterRect& r, uint32_t tilesW, Or orWord)
{
	for (uint32_t ty = r.ty0; ty <= r.ty1; ++ty) {
		const uint32_t k0 = ty * tilesW + r.tx0, k1 = ty * tilesW + r.tx1;
		for (uint32_t w = k0 >> 5; w <= (k1 >> 5); ++w) {
			orWord(w, vgx_tile_word_mask(w == (k0 >> 5) ? (k0 & 31u) : 0u, w == (k1 >> 5) ? (k1 & 31u) : 31u));
		}
	}
}

#ifdef __HIPCC__
// ... on the device: one atomicOr per 32-tile word per tile row (the raster's class bitmaps and the damage marks)
__device__ __forceinline__ void mark_tiles(uint32_t* bits, const VgxRasterRect& r, uint32_t tilesW)
{
	vgx_tile_rect_words(r, tilesW, [bits](uint32_t w, uint32_t mask) { atomicOr(&bits[w], mask); });
}
#endif

VGX_HD bool vgx_damage_bit(const uint32_t* bits, uint32_t key) { return ((bits[key >> 5] >> (key & 31u)) & 1u) != 0u; }

// the marked tiles of rectangle r: the bin entries of a mesh under vgx_raster_damaged
VGX_HD uint32_t vgx_damage_rect_count(const uint32_t* bits, const VgxRasterRect& r, uint32_t tilesW)
{
	uint32_t n = 0;
	vgx_tile_rect_words(r, tilesW, [&n, bits](uint32_t w, uint32_t mask) { n += (uint32_t)__builtin_popcount(bits[w] & mask); });
	return n;
}

// Entry d of a dirty list: the frame meshes [*first, *first + *count) whose boxes it marks. false: INVALID, skipped
VGX_HD bool vgx_damage_entry(const vgx_cache_slot* slots, uint64_t ninst, uint64_t numMeshes, uint64_t d, uint64_t* first, uint64_t* count)
{
	*first = 0; *count = 0;
	if (d >= ninst) { return false; }
	const uint64_t a = slots[d].first_mesh, b = slots[d + 1].first_mesh;
	if (b > numMeshes || b < a) { return false; }
	*first = a; *count = b - a;
	return true;
}

// the vgx_raster_damage record of a damaged call (host only): VGX_OK or VGX_E_INVALID_ARG
static inline int vgx_damage_record_check(const vgx_raster_damage* d)
{
	return !d || !d->tile_bits || ((uintptr_t)d->tile_bits & 3u) || d->reserved != 0u ? VGX_E_INVALID_ARG : VGX_OK;
}

// The window of entries vgx_raster_damaged sorts when the caller names none (include/vgx.h): before any call has been measured, and
// the head room over a measured count
#define VGX_DAMAGE_INITIAL_WINDOW 16384u
static inline uint64_t vgx_damage_head_room(uint64_t measured) { return measured + measured / 8u + 256u; }

// What the host knows of the damaged calls of one kind (vgx_raster_damaged; vgx_raster_commands_damaged) from their own mirror alone:
// known: a call has been measured, need: its entry count, grown: it ended with VGX_E_GROWN. A full render in between teaches nothing
struct VgxDamageWindow { bool known, grown; uint64_t need; };

// a landed mirror of the last damaged call: its status and its entry count. A call that ended otherwise measured nothing
static inline void vgx_damage_learn(VgxDamageWindow* w, uint64_t status, uint64_t entries)
{
	if (status != (uint64_t)VGX_OK && status != (uint64_t)VGX_E_GROWN) { return; }
	w->known = true; w->need = entries; w->grown = status == (uint64_t)VGX_E_GROWN;
}

// The entries the next damaged call sorts (include/vgx.h): the caller's max_entries, no more than `cap` (what the call can offer);
// without one the measured count with head room, or the initial window. At least the need of a call that ended with VGX_E_GROWN,
// whatever max_entries says; never more than `bound` (the entries the call can have at all) nor than 2^32 - 1
static inline uint64_t vgx_damage_window(const VgxDamageWindow& w, uint64_t max_entries, uint64_t cap, uint64_t bound)
{
	uint64_t window = max_entries ? (max_entries < cap ? max_entries : cap) : (w.known ? vgx_damage_head_room(w.need) : (uint64_t)VGX_DAMAGE_INITIAL_WINDOW);
	if (w.grown && w.need > window) { window = vgx_damage_head_room(w.need); }
	if (window > bound) { window = bound; }
	return window > 0xFFFFFFFFull ? 0xFFFFFFFFull : window;
}

#endif
