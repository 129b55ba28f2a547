// vk_devbuf.h -- a workspace that owns its memory and knows its size.
//
// A corpus handle keeps some fifty device workspaces that grow with the queries it serves.  Each used to be a raw pointer with a
// capacity kept beside it by hand, and every site that needed more room spelled out compare / free / clear / allocate / store again
// -- not always the same way: a failed allocation could leave a freed pointer with its old capacity behind, or a capacity without
// its pointer.  Now the rule has one home:
//
//     the pointer is non-null exactly when the capacity is non-zero, and the capacity describes the memory the pointer names --
//     after every call, failed ones included.
//
// The buffer converts to T *, so code that reads a workspace (kernel parameters, copies, pointer arithmetic) is written as for a
// raw pointer; only the code that sizes one calls reserve().
//
// Host only, no HIP types: the allocator is two plain functions, defined over hipMalloc / hipFree (hipHostMalloc / hipHostFree for
// pinned host staging) in vk_corpus.cpp and over malloc with injected failures in tests/devbuf_driver.cpp (CPU tier).
#ifndef VK_DEVBUF_H
#define VK_DEVBUF_H

#include <cstddef>
#include <cstdint>

// 0 and *p set, or the status of a reported error (VK_ERR_HIP through fail()) and *p untouched
int vk_devbuf_alloc(void **p, size_t bytes, bool pinned);
// hipFree, never an asynchronous free: it synchronises the device, and a workspace may still be read by the query before on the stream
void vk_devbuf_free(void *p, bool pinned);

template <typename T, bool Pinned = false>
class vk_devbuf {
	static_assert(16 % sizeof(T) == 0, "an empty request allocates 16 bytes: whole elements");
	T *p = nullptr;
	size_t cap = 0;            // elements
	int64_t *live = nullptr;   // the owner's count of live bytes (null: not counted)

public:
	vk_devbuf() = default;
	vk_devbuf(const vk_devbuf &) = delete;
	vk_devbuf &operator=(const vk_devbuf &) = delete;
	~vk_devbuf() { reset(); }

	operator T *() const { return p; }
	size_t capacity() const { return cap; }

	// Room for n elements; contents are not kept.  The old memory is freed BEFORE the new is asked for (a scratch area may be
	// gigabytes: the peak must not be both).  A failed allocation leaves the buffer empty.  n = 0: 16 bytes, so that a pointer exists.
	int reserve(size_t n, int64_t *live_bytes) {
		if (p && n <= cap) return 0;
		reset();
		if (n == 0) n = 16 / sizeof(T);
		void *q = nullptr;
		const int rc = vk_devbuf_alloc(&q, n * sizeof(T), Pinned);
		if (rc) return rc;
		p = (T *)q; cap = n; live = live_bytes;
		if (live) *live += (int64_t)(cap * sizeof(T));
		return 0;
	}

	void reset() {
		if (!p) return;
		vk_devbuf_free(p, Pinned);
		if (live) *live -= (int64_t)(cap * sizeof(T));
		p = nullptr; cap = 0;
	}
};

#endif
