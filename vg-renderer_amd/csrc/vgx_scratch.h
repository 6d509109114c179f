// vgx_scratch.h -- the context's grow-only device scratch (host code only).
//
// DevBuf is one device block and its capacity in bytes; Buf<T> is the same block seen as an array of T, so that the element
// type of a buffer is written once, at its declaration. A buffer joins its owner's list the first time it receives memory:
// releasing the scratch and counting its bytes walk that list, nobody keeps a second list of names.
//
// The header needs no device and nothing of vgx_ctx: its three dealings with the runtime go through the macros below, and a
// host program may define them before the include (tests/native/scratch_test.cpp puts a counting allocator there).
#ifndef VGX_SCRATCH_H
#define VGX_SCRATCH_H

#include <stddef.h>
#include <stdint.h>
#include "../../include/vgx.h"

#ifndef VGX_SCRATCH_MALLOC
#include <hip/hip_runtime.h>
#define VGX_SCRATCH_MALLOC(pp, bytes) ((int)hipMalloc((pp), (bytes))) // 0 = success, else the runtime's error value
#define VGX_SCRATCH_FREE(p) ((void)hipFree(p))
#define VGX_SCRATCH_E_OOM ((int)hipErrorOutOfMemory)
#endif

struct DevBuf
{
	void* p;
	size_t cap;   // bytes
	DevBuf* next; // the owner's list (DevBufList)
	bool listed;
};

struct DevBufList
{
	DevBuf* head;
};

inline void vgx_scratch_join(DevBufList& owner, DevBuf& b)
{
	if (b.listed) { return; }
	b.listed = true;
	b.next = owner.head;
	owner.head = &b;
}

// Makes `b` hold at least `bytes` bytes (contents are scratch: nothing is copied). When the allocator refuses: VGX_E_HIP, its error
// value in *err, and the buffer holds no block (the old one was given up for the second attempt).
inline int vgx_scratch_grow(DevBufList& owner, DevBuf& b, size_t bytes, int* err)
{
	if (bytes <= b.cap) {
		return VGX_OK;
	}
	// grow with 12.5 % head room so that near-identical batches do not reallocate
	const size_t want = bytes + bytes / 8 + 256;
	if (want < bytes) { *err = VGX_SCRATCH_E_OOM; return VGX_E_HIP; }
	void* fresh = nullptr;
	int e = VGX_SCRATCH_MALLOC(&fresh, want);
	if (e != 0 && b.p) { // not enough room for old + new at once: release the old block first (contents are scratch)
		VGX_SCRATCH_FREE(b.p);
		b.p = nullptr;
		b.cap = 0;
		e = VGX_SCRATCH_MALLOC(&fresh, want);
	}
	if (e != 0) {
		*err = e;
		return VGX_E_HIP;
	}
	if (b.p) { VGX_SCRATCH_FREE(b.p); }
	b.p = fresh;
	b.cap = want;
	vgx_scratch_join(owner, b);
	return VGX_OK;
}

// The two buffers trade blocks (both stay where they are in the list; one that had no memory before joins it)
inline void vgx_scratch_swap(DevBufList& owner, DevBuf& a, DevBuf& b)
{
	void* const p = a.p; a.p = b.p; b.p = p;
	const size_t c = a.cap; a.cap = b.cap; b.cap = c;
	if (a.p) { vgx_scratch_join(owner, a); }
	if (b.p) { vgx_scratch_join(owner, b); }
}

inline uint64_t vgx_scratch_bytes(const DevBufList& owner)
{
	uint64_t n = 0;
	for (const DevBuf* b = owner.head; b; b = b->next) { n += b->cap; }
	return n;
}

// Frees every block; the buffers are empty and off the list afterwards
inline void vgx_scratch_release(DevBufList& owner)
{
	for (DevBuf* b = owner.head; b;) {
		DevBuf* const n = b->next;
		if (b->p) { VGX_SCRATCH_FREE(b->p); }
		b->p = nullptr; b->cap = 0; b->next = nullptr; b->listed = false;
		b = n;
	}
	owner.head = nullptr;
}

// A DevBuf of elements T. No constructor: the context is zeroed as a whole.
template<class T> struct Buf : DevBuf
{
	T* ptr() const { return (T*)p; }
	uint64_t items() const { return cap / sizeof(T); }
	int grow(DevBufList& owner, uint64_t n, int* err)
	{
		if (n > (uint64_t)SIZE_MAX / sizeof(T)) { *err = VGX_SCRATCH_E_OOM; return VGX_E_HIP; }
		return vgx_scratch_grow(owner, *this, (size_t)n * sizeof(T), err);
	}
};

#endif
