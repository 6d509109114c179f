// damage_window_test.cpp -- the sort window of the damaged raster calls (vg-renderer_amd/csrc/vgx_damage.h: VgxDamageWindow,
// vgx_damage_learn, vgx_damage_window), as vgx_raster_damaged and vgx_raster_commands_damaged call it. Host only; prints "ok" and
// returns 0, or names the first check that failed. Built and run by tests/test_damage_window_host.py. The sequences are the ones
// tests/test_gpu_damage.py and tests/test_gpu_commands_damage.py pin on the device; the expected windows are worked out by hand from
// include/vgx.h (initial window 16 384; measured count + 1/8 + 256), never taken from vgx_damage_window itself.
#include <stdio.h>
#include "vgx_damage.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (!failures++) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } } while (0)

static const uint64_t FAR = ~0ull; // no bound, no cap

int main()
{
	CHECK(VGX_DAMAGE_INITIAL_WINDOW == 16384u);
	CHECK(vgx_damage_head_room(16) == 16 + 2 + 256 && vgx_damage_head_room(1120) == 1120 + 140 + 256 && vgx_damage_head_room(0) == 256);

	// a fresh context: the initial window, whatever the tables hold; a small frame's bound cuts it
	{
		const VgxDamageWindow w = {};
		CHECK(vgx_damage_window(w, 0, 72, FAR) == 16384);
		CHECK(vgx_damage_window(w, 0, 1u << 17, FAR) == 16384);
		CHECK(vgx_damage_window(w, 0, 72, 16 * 16) == 256);
	}
	// test_max_entries_too_small_grows_then_succeeds (commands): tables reserved for 64 entries hold 72. max_entries = 1 is the window of
	// the first call, which needs 16 and ends GROWN; the repeat, still asking for 1, gets the need with its head room; then the
	// library's window follows the measured 16, and a wish of 2^20 is cut to what the tables hold
	{
		VgxDamageWindow w = {};
		CHECK(vgx_damage_window(w, 1, 72, FAR) == 1);
		vgx_damage_learn(&w, VGX_E_GROWN, 16);
		CHECK(w.known && w.grown && w.need == 16);
		CHECK(vgx_damage_window(w, 1, 72, FAR) == 274);
		vgx_damage_learn(&w, VGX_OK, 16);
		CHECK(w.known && !w.grown && w.need == 16);
		CHECK(vgx_damage_window(w, 1, 72, FAR) == 1); // no longer grown: the caller's window is the caller's again
		CHECK(vgx_damage_window(w, 0, 72, FAR) == 274);
		CHECK(vgx_damage_window(w, 1u << 20, 72, FAR) == 72);
		CHECK(vgx_damage_window(w, 1u << 20, 1u << 17, FAR) == 1u << 17);
	}
	// the same test of vgx_raster_damaged: max_entries = 2 against tables of 2^17
	{
		VgxDamageWindow w = {};
		CHECK(vgx_damage_window(w, 2, 1u << 17, FAR) == 2);
		vgx_damage_learn(&w, VGX_E_GROWN, 500);
		CHECK(vgx_damage_window(w, 2, 1u << 17, FAR) == 500 + 62 + 256);
		CHECK(vgx_damage_window(w, 1000, 1u << 17, FAR) == 1000); // a need below the caller's window changes nothing
	}
	// test_full_renders_in_between_do_not_move_the_damaged_window: 16 entries, then a call of 1 120 against 16 + 2 + 256 ends GROWN and
	// its repeat passes. A full render in between has a mirror and a window of its own: this one is not told. What a call that ended
	// neither VGX_OK nor VGX_E_GROWN left in the mirror teaches nothing either
	{
		VgxDamageWindow w = {}, full = {};
		vgx_damage_learn(&w, VGX_OK, 16);
		vgx_damage_learn(&full, VGX_OK, 3200);
		CHECK(vgx_damage_window(w, 0, 9216, FAR) == 274 && 274 < 1120);
		vgx_damage_learn(&w, VGX_E_GROWN, 1120);
		CHECK(vgx_damage_window(w, 0, 9216, FAR) == 1516 && 1516 >= 1120);
		vgx_damage_learn(&w, VGX_OK, 1120);
		vgx_damage_learn(&full, VGX_OK, 16);
		CHECK(vgx_damage_window(w, 0, 9216, FAR) == 1516);
		vgx_damage_learn(&w, VGX_E_INVALID_ARG, 7);
		vgx_damage_learn(&w, VGX_E_RANGE, 1ull << 40);
		CHECK(w.known && !w.grown && w.need == 1120);
	}
	// test_library_window_on_a_fresh_context_converges_within_two_calls: 1 100 x 16 entries against the initial window
	{
		VgxDamageWindow w = {};
		CHECK(vgx_damage_window(w, 0, 1100, 1100 * 16) == 16384 && 16384 < 17600);
		vgx_damage_learn(&w, VGX_E_GROWN, 17600);
		CHECK(vgx_damage_window(w, 0, 1100, 1100 * 16) == 17600); // 17 600 + 2 200 + 256, cut to the bound: all the call can have
		CHECK(vgx_damage_window(w, 0, 1100, FAR) == 20056);
	}
	// the clips: to the bound, and to 2^32 - 1
	{
		VgxDamageWindow w = {};
		CHECK(vgx_damage_window(w, 0, FAR, 0) == 0);
		CHECK(vgx_damage_window(w, 1ull << 40, 1ull << 41, FAR) == 0xFFFFFFFFull);
		CHECK(vgx_damage_window(w, 1ull << 40, 1ull << 41, 1000) == 1000);
		vgx_damage_learn(&w, VGX_E_GROWN, 1ull << 33);
		CHECK(vgx_damage_window(w, 0, FAR, FAR) == 0xFFFFFFFFull);
		CHECK(vgx_damage_window(w, 5, FAR, 100) == 100);
	}
	if (!failures) { printf("ok\n"); }
	return failures ? 1 : 0;
}
