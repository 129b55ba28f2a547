// Driver of tests/test_longq_geometry_host.py: every shape of vk_host::longq_geometry_of (vectorian_amd/csrc/vk_longq_host.h) --
// query length 65 .. 512, longest slice 1 .. 512, gap mode, tracebacks, tag weights -- held against the limits of the device and, for
// slices of at most 64 tokens, against the formulas the kernel file had before the header existed (restated below).
#include "vk_longq_host.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace vk_host;

// ---- vk_longq.hip before the header: longq_stride, vk_longq_scratch_bytes, vk_longq_lds_bytes, vk_longq_hm_in_lds, the grid of vk_longq_blocks
static int old_stride(int max_len) { const int w = (max_len + 15) / 16 * 16; return w < 16 ? 16 : w > 64 ? 64 : w; }
static size_t old_scratch_bytes(int len_t, int gap_mode, bool flow, bool tagged) {
	const size_t lt_pad = (size_t)(len_t + 15) / 16 * 16;
	const size_t hm = gap_mode == 2 ? (size_t)(len_t + 1) * 64 * 4 : 0, dm = flow ? (size_t)(len_t + 1) * 64 * 2 : 0, su = (flow && tagged) ? lt_pad * 64 * 4 : 0;
	return (hm + dm + su + 255) / 256 * 256 + 256;
}
static size_t old_lds_bytes(int len_t, int max_len, bool flow) { return (size_t)((len_t + 15) / 16 * 16) * old_stride(max_len) * 4 + (flow ? 8192 : 0) + 64; }
static bool old_hm_in_lds(int len_t, int max_len) { return old_lds_bytes(len_t, max_len, false) + (size_t)(len_t + 1) * old_stride(max_len) * 4 <= 78 * 1024; }
static int old_grid(int cus, int len_t, int max_len, long long n_sent, bool hm_in_lds) {
	const size_t smem = old_lds_bytes(len_t, max_len, false) + (hm_in_lds ? (size_t)(len_t + 1) * old_stride(max_len) * 4 : 0);
	int per_cu = (int)((160 * 1024) / ((smem + 511) / 512 * 512 + 512));
	if (per_cu < 1) per_cu = 1;
	if (per_cu > 16) per_cu = 16;
	const long long want = (long long)cus * per_cu;
	return (int)(n_sent < want ? (n_sent < 1 ? 1 : n_sent) : want);
}

static long long violations = 0;
static void violated(const char *what, int len_t, int max_len, int gap, bool flow, bool tagged) {
	if (violations++ < 20) printf("VIOLATED %s: len_t %d max_len %d gap %d flow %d tagged %d\n", what, len_t, max_len, gap, (int)flow, (int)tagged);
}

int main(int argc, char **argv) {
	if (argc > 1 && !strcmp(argv[1], "worst")) {   // the largest launch and the largest region, for the record
		const longq_geometry g = longq_geometry_of(512, 512, 1, true, true), h = longq_geometry_of(512, 512, 2, true, true);
		printf("lds %zu scratch %zu\n", g.launch_lds_bytes, h.scratch_bytes);
		return 0;
	}
	long long points = 0;
	for (int len_t = 65; len_t <= 512; len_t++)
		for (int max_len = 1; max_len <= 512; max_len++)
			for (int gap = 0; gap < 3; gap++)
				for (int flow = 0; flow < 2; flow++)
					for (int tagged = 0; tagged < 2; tagged++) {
						const longq_geometry g = longq_geometry_of(len_t, max_len, gap, flow != 0, tagged != 0);
						points++;
#define CHECK(cond, what) do { if (!(cond)) violated(what, len_t, max_len, gap, flow != 0, tagged != 0); } while (0)
						// LDS: canon, strip, border columns, matrix -- in this order, none overlapping, all inside the launch, the launch inside a CU
						CHECK(g.launch_lds_bytes <= kLongqLdsLimit, "LDS demand beyond 160 KB");
						CHECK(g.canon_off == 0 && g.strip_off == g.canon_off + g.canon_bytes && g.col_off == g.strip_off + g.strip_bytes &&
							g.hm_lds_off == g.col_off + g.col_bytes && g.hm_lds_off + g.hm_lds_bytes <= g.launch_lds_bytes, "LDS parts overlap or leave the launch");
						CHECK(g.strip_bytes == (size_t)g.lt_pad * g.s_stride * 4 && g.lt_pad >= len_t && g.lt_pad % 16 == 0, "strip");
						CHECK(g.canon_bytes == (flow ? kLongqCanonLds : 0), "canon");
						CHECK(g.blocks == (max_len > 64), "form");
						if (g.blocks) {
							CHECK(g.s_stride == 64 && g.ls_pad >= max_len && g.ls_pad % 64 == 0 && g.ls_pad < max_len + 64, "block form strides");
							CHECK(g.col_bytes == 2 * (size_t)(gap == 1 ? 2 : 1) * (size_t)(len_t + 1) * 4 && !g.hm_in_lds, "border columns");
						} else CHECK(g.col_bytes == 0 && g.ls_pad == 64, "no border columns");
						// the scratch region: matrix, records, similarities -- sized for the longest slice, disjoint, inside the region
						const size_t need_hm = gap == 2 ? (size_t)(len_t + 1) * g.ls_pad * 4 : 0, need_dm = flow ? (size_t)(len_t + 1) * g.ls_pad * 2 : 0;
						const size_t need_su = (flow && (tagged || g.blocks)) ? (size_t)g.lt_pad * g.ls_pad * 4 : 0;
						CHECK(g.hm_bytes >= need_hm && g.dm_bytes >= need_dm && g.su_bytes >= need_su, "a part of the region is too small");
						CHECK(g.hm_off == 0 && g.dm_off >= g.hm_off + g.hm_bytes && g.su_off >= g.dm_off + g.dm_bytes && g.su_off + g.su_bytes <= g.scratch_bytes,
							"parts of the region overlap or leave it");
						CHECK(g.dm_off % 2 == 0 && g.su_off % 4 == 0, "alignment");
						for (long long n : {0ll, 1ll, 7ll, 300ll, 200000ll}) {
							const int grid = longq_grid(256, g.launch_lds_bytes, n);
							CHECK(grid >= 1 && (n < 1 || grid <= n) && grid <= 256 * 16, "grid");
							if (!g.blocks && !flow) CHECK(grid == old_grid(256, len_t, max_len, n, g.hm_in_lds), "grid differs from vk_longq_blocks");
						}
						for (int k : {1, 9, 256, 257, 1032}) {
							const int grid = longq_flow_grid(g.blocks, k);
							CHECK(grid >= 1 && grid <= k && (g.blocks ? grid <= kLongqFlowGrid : grid == k), "traceback grid");
						}
						if (!g.blocks) {   // the form that was: the values its callers had
							CHECK(g.s_stride == old_stride(max_len) && longq_stride(max_len) == old_stride(max_len), "stride differs");
							CHECK(g.scratch_bytes == old_scratch_bytes(len_t, gap, flow != 0, tagged != 0), "scratch bytes differ");
							CHECK(g.lds_bytes == old_lds_bytes(len_t, max_len, flow != 0), "LDS bytes differ");
							CHECK(longq_hm_in_lds(len_t, max_len) == old_hm_in_lds(len_t, max_len), "matrix-in-LDS rule differs");
							CHECK(g.hm_in_lds == (gap == 2 && !flow && old_hm_in_lds(len_t, max_len)), "matrix-in-LDS differs");
							CHECK(g.launch_lds_bytes == g.lds_bytes + (g.hm_in_lds ? (size_t)(len_t + 1) * old_stride(max_len) * 4 : 0), "launch LDS differs");
							CHECK(g.dm_off == (gap == 2 ? (size_t)(len_t + 1) * 64 * 4 : 0) && g.su_off == g.dm_off + (flow ? (size_t)(len_t + 1) * 64 * 2 : 0), "offsets differ from the kernel's");
						}
#undef CHECK
					}
	// (slices beyond 64 tokens clamp the old stride to 64: the pass over the short slices of a mixed corpus is sized by its own longest)
	printf("points %lld violations %lld\n", points, violations);
	return violations ? 1 : 0;
}
