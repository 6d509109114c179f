// scratch_test.cpp -- the context's grow-only scratch (vg-renderer_amd/csrc/vgx_scratch.h) over a counting allocator: the growth
// rule, the typed view, the retry when old and new block do not fit at once, the owner list. Host only; prints "ok" and
// returns 0, or names the first check that failed. Built and run by tests/test_scratch_host.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace fake {
enum { kOom = 2 };
std::map<void*, size_t> live;        // blocks handed out and not freed yet
std::set<void*> freed;               // addresses freed and not handed out again since
std::vector<std::string> events;     // "alloc" / "fail" / "free", in order
std::vector<void*> freedLog;         // every address freed, in order
int failNext = 0, doubleFrees = 0, strangerFrees = 0;
size_t allocs = 0, lastBytes = 0;
int malloc_(void** pp, size_t n)
{
	lastBytes = n;
	if (failNext > 0) { --failNext; events.push_back("fail"); return kOom; }
	void* p = malloc(n);
	if (!p) { abort(); }
	freed.erase(p);
	live[p] = n;
	++allocs;
	events.push_back("alloc");
	*pp = p;
	return 0;
}
void free_(void* p)
{
	events.push_back("free");
	freedLog.push_back(p);
	const auto it = live.find(p);
	if (it == live.end()) { if (freed.count(p)) { ++doubleFrees; } else { ++strangerFrees; } return; }
	memset(p, 0xDD, it->second); // poison: a reader of a released block sees it
	live.erase(it);
	freed.insert(p);
	free(p);
}
size_t timesFreed(void* p, size_t since) { size_t n = 0; for (size_t i = since; i < freedLog.size(); ++i) { n += freedLog[i] == p; } return n; } // (an address may come back from malloc: count from a mark)
}

#define VGX_SCRATCH_MALLOC(pp, bytes) fake::malloc_((pp), (bytes))
#define VGX_SCRATCH_FREE(p) fake::free_(p)
#define VGX_SCRATCH_E_OOM ((int)fake::kOom)
#include "vgx_scratch.h"

#include <type_traits>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct E24 { char c[24]; };
static_assert(std::is_trivial<DevBuf>::value && std::is_trivial<Buf<E24>>::value && std::is_trivial<DevBufList>::value, "the context is zeroed as a whole");
static_assert(sizeof(Buf<E24>) == sizeof(DevBuf), "a view adds nothing");

static size_t grown(size_t bytes) { return bytes + bytes / 8 + 256; }
static bool onList(const DevBufList& L, const DevBuf* b) { size_t n = 0; for (const DevBuf* q = L.head; q; q = q->next) { n += q == b; } return n == 1; }
static size_t listLength(const DevBufList& L) { size_t n = 0; for (const DevBuf* q = L.head; q; q = q->next) { ++n; } return n; }

static void testGrowth()
{
	DevBufList L = {};
	DevBuf b = {};
	int err = -1;
	const size_t mark = fake::freedLog.size();
	CHECK(vgx_scratch_grow(L, b, 0, &err) == VGX_OK && b.p == nullptr && fake::allocs == 0 && !b.listed); // nothing asked, nothing held
	CHECK(vgx_scratch_grow(L, b, 1, &err) == VGX_OK);
	CHECK(b.cap == 257 && b.p != nullptr && fake::lastBytes == 257 && fake::allocs == 1);
	void* const first = b.p;
	memset(b.p, 0, b.cap); // the whole capacity is the caller's
	CHECK(vgx_scratch_grow(L, b, 257, &err) == VGX_OK && b.p == first && b.cap == 257); // at the capacity
	CHECK(vgx_scratch_grow(L, b, 100, &err) == VGX_OK && b.p == first && b.cap == 257); // below it
	CHECK(fake::allocs == 1 && fake::freedLog.size() == mark);
	CHECK(vgx_scratch_grow(L, b, 258, &err) == VGX_OK && b.cap == grown(258) && b.p != nullptr); // one byte past it
	CHECK(fake::timesFreed(first, mark) == 1 && fake::freedLog.size() == mark + 1);
	void* const second = b.p;
	const size_t eventsBefore = fake::events.size();
	CHECK(vgx_scratch_grow(L, b, 4096, &err) == VGX_OK);
	CHECK(b.cap == 4096 + 512 + 256 && fake::lastBytes == b.cap);
	CHECK(fake::freedLog.size() == mark + 2 && fake::freedLog[mark + 1] == second);
	// the new block first, the old one released afterwards
	CHECK(fake::events.size() == eventsBefore + 2 && fake::events[eventsBefore] == "alloc" && fake::events[eventsBefore + 1] == "free");
	CHECK(err == -1); // only a failure writes it
	CHECK(fake::live.size() == 1 && fake::live.count(b.p) == 1 && fake::live[b.p] == b.cap);
	vgx_scratch_release(L);
	CHECK(fake::live.empty() && b.p == nullptr && b.cap == 0);
}

template<class T> static void typedView(uint64_t n)
{
	DevBufList L = {};
	Buf<T> b = {};
	int err = -1;
	const size_t before = fake::allocs;
	CHECK(b.grow(L, n, &err) == VGX_OK);
	CHECK(fake::allocs == before + 1 && fake::lastBytes == grown((size_t)n * sizeof(T))); // n * sizeof(T) bytes were asked for
	CHECK(b.cap == grown((size_t)n * sizeof(T)));
	CHECK(b.items() == b.cap / sizeof(T) && b.items() >= n);
	CHECK((void*)b.ptr() == b.p);
	CHECK(b.grow(L, b.items(), &err) == VGX_OK && fake::allocs == before + 1);     // what it holds fits
	CHECK(b.grow(L, b.items() + 1, &err) == VGX_OK && fake::allocs == before + 2); // one more does not
	CHECK(b.cap == fake::lastBytes && b.items() == b.cap / sizeof(T));
	// an element count whose bytes do not fit size_t: refused, nothing asked of the allocator
	const size_t cap = b.cap;
	if (sizeof(T) > 1) {
		CHECK(b.grow(L, UINT64_MAX / sizeof(T) + 1, &err) == VGX_E_HIP && err == fake::kOom && fake::allocs == before + 2 && b.cap == cap);
	}
	vgx_scratch_release(L);
}

static void testRetry()
{
	DevBufList L = {};
	DevBuf b = {};
	int err = -1;
	CHECK(vgx_scratch_grow(L, b, 1000, &err) == VGX_OK);
	void* const old = b.p;
	size_t mark = fake::freedLog.size();
	// the first allocation fails once: the old block goes first, the retry's block is installed
	fake::failNext = 1;
	size_t e0 = fake::events.size();
	CHECK(vgx_scratch_grow(L, b, 2000, &err) == VGX_OK);
	CHECK(fake::events.size() == e0 + 3 && fake::events[e0] == "fail" && fake::events[e0 + 1] == "free" && fake::events[e0 + 2] == "alloc");
	CHECK(fake::freedLog.size() == mark + 1 && fake::freedLog[mark] == old && b.p != nullptr && b.cap == grown(2000) && fake::live.count(b.p) == 1 && fake::live.size() == 1);
	CHECK(err == -1 && onList(L, &b));
	// it fails twice: the error comes back, the buffer is empty and still the owner's
	void* const second = b.p;
	mark = fake::freedLog.size();
	fake::failNext = 2;
	e0 = fake::events.size();
	CHECK(vgx_scratch_grow(L, b, 4000, &err) == VGX_E_HIP);
	CHECK(err == fake::kOom);
	CHECK(fake::events.size() == e0 + 3 && fake::events[e0] == "fail" && fake::events[e0 + 1] == "free" && fake::events[e0 + 2] == "fail");
	CHECK(b.p == nullptr && b.cap == 0 && fake::freedLog.size() == mark + 1 && fake::freedLog[mark] == second && fake::live.empty());
	CHECK(onList(L, &b) && listLength(L) == 1 && vgx_scratch_bytes(L) == 0);
	// a later growth succeeds, and the buffer is not listed twice
	err = -1;
	CHECK(vgx_scratch_grow(L, b, 10, &err) == VGX_OK && b.p != nullptr && b.cap == grown(10) && err == -1);
	CHECK(onList(L, &b) && listLength(L) == 1 && vgx_scratch_bytes(L) == b.cap);
	// an empty buffer has no old block to give up: one attempt, and it never joined the list
	DevBuf fresh = {};
	fake::failNext = 1;
	e0 = fake::events.size();
	CHECK(vgx_scratch_grow(L, fresh, 10, &err) == VGX_E_HIP && err == fake::kOom && fake::events.size() == e0 + 1);
	CHECK(fresh.p == nullptr && fresh.cap == 0 && !fresh.listed && listLength(L) == 1 && fake::failNext == 0);
	vgx_scratch_release(L);
	CHECK(fake::live.empty());
}

static void testOwnerList()
{
	DevBufList L = {};
	Buf<uint32_t> a = {};
	Buf<E24> twice = {};
	DevBuf c = {};
	Buf<uint64_t> never = {};
	int err = -1;
	CHECK(vgx_scratch_bytes(L) == 0);
	CHECK(a.grow(L, 7, &err) == VGX_OK);
	CHECK(twice.grow(L, 3, &err) == VGX_OK);
	CHECK(vgx_scratch_grow(L, c, 513, &err) == VGX_OK);
	CHECK(twice.grow(L, 300, &err) == VGX_OK);
	CHECK(listLength(L) == 3 && onList(L, &a) && onList(L, &twice) && onList(L, &c) && !onList(L, &never));
	CHECK(vgx_scratch_bytes(L) == a.cap + twice.cap + c.cap);
	CHECK(fake::live.size() == 3);
	// two buffers trade blocks; one that had none joins the list with the block it receives
	Buf<uint32_t> late = {};
	void* const pa = a.p; const size_t ca = a.cap;
	vgx_scratch_swap(L, a, late);
	CHECK(late.p == pa && late.cap == ca && a.p == nullptr && a.cap == 0 && onList(L, &late) && onList(L, &a) && listLength(L) == 4);
	CHECK(vgx_scratch_bytes(L) == late.cap + twice.cap + c.cap);
	void* const blocks[3] = { late.p, twice.p, c.p };
	const size_t freesBefore = fake::freedLog.size();
	vgx_scratch_release(L);
	CHECK(fake::freedLog.size() == freesBefore + 3);
	for (void* p : blocks) { CHECK(fake::timesFreed(p, freesBefore) == 1); }
	CHECK(fake::live.empty() && L.head == nullptr && vgx_scratch_bytes(L) == 0);
	CHECK(a.p == nullptr && twice.p == nullptr && c.p == nullptr && late.p == nullptr && twice.cap == 0 && !twice.listed);
	CHECK(never.p == nullptr && never.cap == 0 && never.next == nullptr && !never.listed); // never visited
	vgx_scratch_release(L); // nothing left to free
	CHECK(fake::freedLog.size() == freesBefore + 3);
	// the buffers serve again
	CHECK(twice.grow(L, 1, &err) == VGX_OK && listLength(L) == 1 && vgx_scratch_bytes(L) == grown(24));
	vgx_scratch_release(L);
}

int main()
{
	testGrowth();
	typedView<E24>(10);
	typedView<uint32_t>(100);
	typedView<E24>(1);
	testRetry();
	testOwnerList();
	CHECK(fake::live.empty());
	CHECK(fake::doubleFrees == 0 && fake::strangerFrees == 0);
	if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
	printf("ok\n");
	return 0;
}
