// Driver of tests/test_devbuf.py: vk_devbuf.h (vectorian_amd/csrc) over a fake allocator.  The fake is malloc / free with a log of
// every call, a set of the blocks that are live (a block freed twice or never is reported, and AddressSanitizer aborts on it as well)
// and a switch that makes the n-th allocation from now fail, as hipMalloc does when the card is full.
#include "vk_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

static std::vector<std::string> g_log;
static std::map<void *, size_t> g_live;   // block -> bytes
static int g_fail_in = 0;                 // > 0: the g_fail_in-th allocation from now fails
static int g_double_free = 0;

int vk_devbuf_alloc(void **p, size_t bytes, bool pinned) {
	if (g_fail_in > 0 && --g_fail_in == 0) {
		g_log.push_back("alloc " + std::to_string(bytes) + " FAILED");
		return 3;   // VK_ERR_HIP
	}
	*p = malloc(bytes);
	g_live[*p] = bytes;
	g_log.push_back(std::string(pinned ? "alloc_pinned " : "alloc ") + std::to_string(bytes));
	return 0;
}

void vk_devbuf_free(void *p, bool pinned) {
	auto it = g_live.find(p);
	if (it == g_live.end()) g_double_free++;
	else {
		g_log.push_back(std::string(pinned ? "free_pinned " : "free ") + std::to_string(it->second));
		g_live.erase(it);
	}
	free(p);
}

static int64_t live_bytes() {
	int64_t b = 0;
	for (const auto &kv : g_live) b += (int64_t)kv.second;
	return b;
}

static void report(const char *name, const std::string &state) {
	printf("%s: %s |", name, state.c_str());
	for (const auto &s : g_log) printf(" [%s]", s.c_str());
	printf("\n");
	g_log.clear();
}

template <typename B> static std::string state_of(const B &b, int rc, int64_t counted) {
	const bool consistent = ((float *)b != nullptr) == (b.capacity() != 0);
	return "rc=" + std::to_string(rc) + " ptr=" + ((float *)b ? "set" : "null") + " cap=" + std::to_string(b.capacity()) +
		" counted=" + std::to_string(counted) + " live=" + std::to_string(live_bytes()) + (consistent ? "" : " INVARIANT BROKEN");
}

// what the call sites of the host units do with a workspace: each form once
struct Params { const float *table; float *out; void *scratch; };
static size_t takes_void(void *p, const void *q) { return (p != nullptr) + (q != nullptr); }

static int conversions() {
	int64_t counted = 0;
	vk_devbuf<float> a, b[2], c3[3];
	if (!a) { if (a.reserve(8, &counted)) return 1; } else return 2;   // `if (!c->d_x)`
	if (!a || a == nullptr) return 3;
	float *raw = a;                                                    // plain assignment
	if (a + 3 != raw + 3 || &a[3] != raw + 3) return 4;                 // pointer arithmetic, subscript
	Params p{};
	p.table = a; p.out = a + 1; p.scratch = a;                         // into kernel-parameter structs (const T *, T *, void *)
	if (p.table != raw || p.out != raw + 1 || p.scratch != (void *)raw) return 5;
	if ((void *)a != (void *)raw) return 6;                            // explicit cast
	if (takes_void(a, a) != 2) return 7;                               // a void * / const void * parameter (hipMemcpyAsync)
	const bool want = false;
	p.out = want ? (float *)a : nullptr;                               // against nullptr a conditional needs the pointer spelled out
	p.table = want ? a + 16 : nullptr;                                 // ... arithmetic already is one
	if (p.out) return 8;
	if (b[1].reserve(4, &counted)) return 9;
	int cur = 0;
	if (b[1 - cur] + 2 != (float *)b[1] + 2 || b[cur]) return 10;       // an array of buffers (d_keys[cur])
	for (int which = 0; which < 3; which++) {                          // a reference to one of three members (wide_order)
		vk_devbuf<float> &ord = which == 0 ? c3[0] : which == 1 ? c3[1] : c3[2];
		if (ord.reserve(2 + which, &counted)) return 11;
	}
	if (c3[2].capacity() != 4 || counted != live_bytes()) return 12;
	return 0;
}

int main() {
	int64_t counted = 0;
	{
		vk_devbuf<float> buf;
		report("fresh", state_of(buf, 0, counted));
		int rc = buf.reserve(100, &counted);
		report("first_reserve", state_of(buf, rc, counted));
		// steady state: what fits costs a comparison, no allocator call
		float *before = buf;
		rc = buf.reserve(100, &counted);
		if (!rc) rc = buf.reserve(7, &counted);
		if (!rc) rc = buf.reserve(0, &counted);
		report("steady_state", state_of(buf, rc ? rc : (before == (float *)buf ? 0 : 99), counted));
		// growth: the old memory goes before the new is asked for
		rc = buf.reserve(1000, &counted);
		report("grow", state_of(buf, rc, counted));
		// the allocation of a growth fails: the buffer is empty, nothing dangles
		g_fail_in = 1;
		rc = buf.reserve(5000, &counted);
		report("failed_grow", state_of(buf, rc, counted));
		// ... a request the old capacity would have held must allocate now
		rc = buf.reserve(50, &counted);
		report("reserve_after_failure", state_of(buf, rc, counted));
		buf.reset();
		report("reset", state_of(buf, 0, counted));
		buf.reset();
		report("reset_twice", state_of(buf, 0, counted));
		// an empty request still yields a pointer: 16 bytes
		rc = buf.reserve(0, &counted);
		report("empty_request", state_of(buf, rc, counted));
		rc = buf.reserve(2000, &counted);
		report("before_destruction", state_of(buf, rc, counted));
	}
	{
		vk_devbuf<float> gone;
		report("destroyed", state_of(gone, 0, counted));
	}
	{   // pinned host staging: the other allocator pair, outside the byte count
		vk_devbuf<float, true> pinned;
		int rc = pinned.reserve(64, nullptr);
		report("pinned", state_of(pinned, rc, counted));
		rc = pinned.reserve(128, nullptr);
		report("pinned_grow", state_of(pinned, rc, counted));
	}
	report("pinned_destroyed", "live=" + std::to_string(live_bytes()));
	{   // a group sized from one number (d_out_raw / d_out_sim / d_out_map): a failure in the middle leaves every member whole or empty
		vk_devbuf<float> raw, sim;
		vk_devbuf<int16_t> map;
		int rc = raw.reserve(10, &counted);
		if (!rc) rc = sim.reserve(640, &counted);
		if (!rc) rc = map.reserve(640, &counted);
		g_log.clear();
		g_fail_in = 2;
		rc = raw.reserve(20, &counted);
		if (!rc) rc = sim.reserve(1280, &counted);
		if (!rc) rc = map.reserve(1280, &counted);
		report("group_failure", "rc=" + std::to_string(rc) + " raw=" + std::to_string(raw.capacity()) + " sim=" + std::to_string(sim.capacity()) +
			" map=" + std::to_string(map.capacity()) + " counted=" + std::to_string(counted) + " live=" + std::to_string(live_bytes()));
	}
	const int conv = conversions();
	g_log.clear();
	report("conversions", "rc=" + std::to_string(conv));
	report("end", "counted=" + std::to_string(counted) + " live=" + std::to_string(live_bytes()) + " double_free=" + std::to_string(g_double_free));
	return 0;
}
