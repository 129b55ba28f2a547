// vk_bound_host.h -- the bound pass where it needs no device: the format of a shadow, the quantizer of a row on either
// grid, the order of a tile, the query's bound tile with the constants of its cells, and the rule by which a handle stops trying.
// One definition each for the corpus's side (vk_shadow_kernel, vk_pack.hip, which compiles quantize_row for the device) and for the
// query's side (vk_pack_query): a bound holds because both sides are the same function.  No HIP types: tests/test_bound_pass_host.py
// and tests/test_bound6_host.py compile it with g++ under AddressSanitizer and UBSan and hold each rule against its statement in
// numpy (CPU tier); tests/test_gpu_shadow_bytes.py holds every byte the device writes against the same statements.
#ifndef VK_BOUND_HOST_H
#define VK_BOUND_HOST_H

#include "../../include/vectorian_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define VK_HOST_DEVICE __host__ __device__
#define VK_UNROLL _Pragma("unroll")
#else
#define VK_HOST_DEVICE
#define VK_UNROLL
#endif

namespace vk_host {

// ---- the format of a shadow.  A tile is 16 rows like a token tile: `steps` K-steps of the bound kernel's MFMA,
// then 16 x (s_x, e_x) as floats.  A K-step holds step_features features of every row in 64 lane operands, lane 16 g + i row i of
// quarter g; of the last K-step the kernel fetches `live` quarters, those that hold features, and the tile keeps `kept` of them.
//          MFMA                               step_features  bytes per K-step  steps  kept   tile_bytes            gamma_width
//   8 bit  v_mfma_i32_16x16x64_i8             64             1,024             5      4      5,248                 320   (289 .. 304 features)
//   8 bit                                     64             1,024             12     4      12,416                768   (753 .. 768)
//   6 bit  v_mfma_scale_f32_16x16x128_f8f6f4  128            1,536             3      live   3,200 + 384 live      320   (289 .. 304)
//   6 bit, compact             128            1,536; 576        3      2      3,712                 320   (289 .. 304)
// Compact: the last K-step is part P, 32 lanes x 12 bytes -- words 0 .. 2 of quarter 0 (lanes 0 .. 15) and of quarter 1 (16 .. 31),
// which are all of quarter 1's live words at every width up to 304 -- then part Q, 16 lanes x 12 bytes, words 3 .. 5 of quarter 0;
// behind it 16 x (s_x, e_x) as two bf16 in one word, s_x the low half (fp6c_meta), both rounded up (quantize_row, bf16_meta).
// The query's tile keeps every K-step whole (qtile_bytes; in LDS the cells' constants follow in VK_DEV_BOUND_CONST_BYTES, vk_device.h).
struct shadow_format {
	int bits = 0;            // 0: no shadow; 8: int8 codes (MODE 7); 6: E2M3 codes (MODE 8)
	int d = 0;               // features of a row
	int steps = 0, step_features = 0;
	int live = 0, kept = 0;  // quarters of the last K-step: fetched, stored (1 .. 4)
	int gamma_width = 0;     // the exact kernel's padded K, nk32 * 32: the d_pad of bound_cell_constants
	int compact = 0;         // 6 bit only: the compact last K-step (parts P and Q, 576 bytes) and 64 bytes of (s, e) as bf16 pairs
	constexpr int step_bytes() const { return step_features * bits * 2; }   // 16 rows of step_features codes
	constexpr int last_step_bytes() const { return compact ? 48 * 12 : kept * (step_bytes() / 4); }
	constexpr int meta_offset() const { return (steps - 1) * step_bytes() + last_step_bytes(); }   // where the 16 x (s, e) sit
	constexpr int tile_bytes() const { return meta_offset() + (compact ? 64 : 128); }
	constexpr int qtile_bytes() const { return steps * step_bytes(); }
	// features a tile has room for (compact: quarter 1 of the last K-step keeps three words, sixteen codes)
	constexpr int width() const { return (steps - 1) * step_features + (compact ? 48 : kept * (step_features / 4)); }
	constexpr int walk() const { return (width() + 31) / 32 * 32; }   // ... in whole lane operands of either grid: what quantize_row walks
};
constexpr int bits6_compact = 60;   // bits_wanted of shadow_format_of: six bits in the compact layout
// The format of the shadow of a corpus, or none (bits = 0): contextual bf16 rows whose exact kernel is one of the two compile-time
// forms that rescore the contenders -- nk32 = 10 with a half K-step (289 .. 304 features) or nk32 = 24 (753 .. 768).  Six bits exist
// for the first only; asked of the second they give its 8-bit form.  bits_wanted: 8, 6 or bits6_compact.
constexpr shadow_format shadow_format_of(int d, int nk32, int tail, int prec, int layout, int bits_wanted) {
	shadow_format f;
	const int steps8 = (nk32 == 10 && tail == 1) ? 5 : (nk32 == 24 && tail == 0) ? 12 : 0;
	if (layout != VK_LAYOUT_CONTEXTUAL || prec != 0 || steps8 == 0) return f;
	f.d = d; f.gamma_width = nk32 * 32;
	if (steps8 == 5 && bits_wanted == 6) {
		f.bits = 6; f.steps = 3; f.step_features = 128;
		f.live = f.kept = (d - 256 + 31) / 32;   // the quarters of 32 features that hold any: 2
	} else if (steps8 == 5 && bits_wanted == bits6_compact) {
		f.bits = 6; f.steps = 3; f.step_features = 128;
		f.live = f.kept = 2; f.compact = 1;      // d <= 304: quarter 1 holds at most 16 features, three words of a lane's six
	} else {
		f.bits = 8; f.steps = steps8; f.step_features = 64;
		f.live = (d - 64 * (steps8 - 1) + 15) / 16; f.kept = 4;   // the kernel steps over whole blocks
	}
	return f;
}

// ---- the quantizer of one row x (the bf16 values as stored, handed over as floats) on a grid of codes: s = max|x| / top, code k the
// grid value nearest to x[k] / s; e >= |x - s x^|, n >= |s x^|, a >= |x| with s x^ the row the codes stand for (Euclidean norms,
// summed in double in k order, then rounded UP to float: quant_up).  A row of zeros gives zeros throughout.
// bf16_meta (the compact shadow, which stores s and e as bf16): s is the least bf16 >= max|x| / top and the codes are computed with
// THAT s, so |x / s| <= top still holds and nothing new clips; e is the least bf16 >= quant_up(|x - s x^|); n is taken from the rows
// s x^ as quantized with that s.  The bound of DESIGN 11.2 holds for any s > 0 and any e at least the true error: it uses s only
// through the row s x^ that the codes stand for, and e only as an upper bound of |x - s x^|.
struct quant_meta { float s = 0.0f, e = 0.0f, n = 0.0f, a = 0.0f; };
// x (1 + 1e-6) as a float, then the next float up (nextafterf towards +inf; FLT_MAX and beyond give +inf)
VK_HOST_DEVICE inline float quant_up(double x) {
	if (!(x > 0.0)) return 0.0f;
	const float f = (float)(x * (1.0 + 1e-6));
	if (!(f < INFINITY)) return f;
	return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u);
}

// the least bf16 value >= f, as a float (f >= 0 or +inf; a NaN stays one)
VK_HOST_DEVICE inline float bf16_up(float f) {
	const uint32_t u = __builtin_bit_cast(uint32_t, f);
	return __builtin_bit_cast(float, (u & 0xffffu) ? (u | 0xffffu) + 1u : u);
}
// 16 x (s, e) of a compact tile: one word per token, s the low half, e the high half (both bf16 values already)
VK_HOST_DEVICE inline uint32_t fp6c_meta(float s, float e) {
	return (__builtin_bit_cast(uint32_t, s) >> 16) | (__builtin_bit_cast(uint32_t, e) & 0xffff0000u);
}

// The int8 grid: the integers -127 .. 127, ties to even (nearbyintf).  The code is the integer; sixteen of them are a lane's operand
// of v_mfma_i32_16x16x64_i8.
struct grid_i8 {
	static constexpr float top = 127.0f;
	static constexpr int lane_codes = 16;
	VK_HOST_DEVICE static int code_of(float x, float s, float *value) {
		*value = fminf(127.0f, fmaxf(-127.0f, nearbyintf(x / s)));
		return (int)*value;
	}
};

// The E2M3 grid: bit 5 the sign, bits 4 .. 0 the magnitude: 0 .. 1.875 in steps of 0.125 (codes 0 .. 15), 2 .. 3.75 in
// steps of 0.25 (16 .. 23), 4 .. 7.5 in steps of 0.5 (24 .. 31) -- the operand format of v_mfma_scale_f32_16x16x128_f8f6f4 with
// cbsz = blgp = 2; thirty-two codes are a lane's operand.  No code is an infinity or a NaN.
VK_HOST_DEVICE inline int e2m3_eighths(int code) {   // 8 x the value: an integer, |.| <= 60
	const int mag = code & 31, e = mag >> 3, f = mag & 7;
	const int n = e == 0 ? f : (8 + f) << (e - 1);
	return (code & 32) ? -n : n;
}
// the magnitude bits of the grid value n8 / 8 (n8 = 0 .. 15, an even number up to 30, a multiple of 4 up to 60)
VK_HOST_DEVICE inline int e2m3_mag_of_eighths(int n8) {
	return n8 < 16 ? n8 : n8 < 32 ? 16 + ((n8 - 16) >> 1) : 24 + ((n8 - 32) >> 2);
}
// a tie at the midpoint of a step goes to the even multiple of that step (nearbyintf), magnitudes clip to 7.5, no negative zero
struct grid_e2m3 {
	static constexpr float top = 7.5f;
	static constexpr int lane_codes = 32;
	VK_HOST_DEVICE static int code_of(float x, float s, float *value) {
		const float t = fminf(7.5f, fabsf(x / s));
		const float step = t < 2.0f ? 0.125f : t < 4.0f ? 0.25f : 0.5f;
		const float a = fminf(7.5f, nearbyintf(t / step) * step);
		const int mag = e2m3_mag_of_eighths((int)(a * 8.0f));
		*value = x < 0.0f ? -a : a;
		return mag | ((x < 0.0f && mag != 0) ? 32 : 0);
	}
};

// get(k): x[k] for k < d; put(k, code): every k < width in turn, zero codes from d on (width >= d: the features a tile has room for).
// Walks the row a lane's operand at a time, so that a put which collects one sees a constant k % lane_codes once the loop is unrolled.
template <typename Grid, typename Get, typename Put> VK_HOST_DEVICE inline quant_meta quantize_row(int d, int width, Get get, Put put, bool bf16_meta = false) {
	float m = 0.0f;
	for (int k = 0; k < d; k++) m = fmaxf(m, fabsf(get(k)));
	quant_meta r;
	r.s = m / Grid::top;
	if (bf16_meta) r.s = bf16_up(r.s);
	double e2 = 0.0, n2 = 0.0, a2 = 0.0;
	for (int k0 = 0; k0 < width; k0 += Grid::lane_codes) {
		VK_UNROLL
		for (int j = 0; j < Grid::lane_codes; j++) {
			const int k = k0 + j;
			if (k >= width) break;
			int code = 0;
			if (k < d) {
				const float x = get(k);
				float v = 0.0f;
				if (r.s > 0.0f) code = Grid::code_of(x, r.s, &v);
				const double xs = (double)r.s * (double)v, dd = (double)x - xs;
				e2 += dd * dd; n2 += xs * xs; a2 += (double)x * (double)x;
			}
			put(k, code);
		}
	}
	r.e = quant_up(sqrt(e2)); r.n = quant_up(sqrt(n2)); r.a = quant_up(sqrt(a2));
	if (bf16_meta) r.e = bf16_up(r.e);
	return r;
}
inline quant_meta quantize_row_i8(const float *x, int d, int8_t *xq) {
	return quantize_row<grid_i8>(d, d, [=](int k) { return x[k]; }, [=](int k, int code) { xq[k] = (int8_t)code; });
}
inline quant_meta quantize_row_e2m3(const float *x, int d, uint8_t *xq, bool bf16_meta = false) {
	return quantize_row<grid_e2m3>(d, d, [=](int k) { return x[k]; }, [=](int k, int code) { xq[k] = (uint8_t)code; }, bf16_meta);
}

// ---- the order of a tile.  int8: K-step k / 64, lane 16 ((k % 64) / 16) + i, byte k % 16 of the lane's 16.
VK_HOST_DEVICE inline size_t i8_offset(int i, int k) { return (size_t)(k >> 6) * 1024 + (size_t)(((k & 63) >> 4) * 16 + i) * 16 + (size_t)(k & 15); }
// one row's codes (d of them; the tile holds zeros beyond) into row i of a tile
inline void i8_put_row(uint8_t *tile, int i, const uint8_t *codes, int d) {
	for (int k = 0; k < d; k++) tile[i8_offset(i, k)] = codes[k];
}
// E2M3: a lane's operand of one K-step is 32 codes, code j at bits 6 j .. 6 j + 5 of 192 (six words).  Stored as the tile keeps a
// K-step of `quarters` 16-lane quarters: the first four words of lane l at 16 l, the last two behind all of those at 256 quarters + 8 l.
VK_HOST_DEVICE inline void fp6_pack32(const uint8_t *codes, uint32_t *w) {
	for (int i = 0; i < 6; i++) w[i] = 0u;
	for (int j = 0; j < 32; j++) {
		const int bit = 6 * j;
		w[bit >> 5] |= (uint32_t)(codes[j] & 63) << (bit & 31);
		if ((bit & 31) > 26) w[(bit >> 5) + 1] |= (uint32_t)(codes[j] & 63) >> (32 - (bit & 31));
	}
}
inline void fp6_store_lane(uint8_t *step, int quarters, int lane, const uint32_t *w) {
	memcpy(step + (size_t)lane * 16, w, 16);
	memcpy(step + (size_t)quarters * 256 + (size_t)lane * 8, w + 4, 8);
}
// one row's codes (d of them, zeros beyond) into row i of a tile whose last K-step keeps `kept` quarters (4: a query tile)
inline void fp6_put_row(uint8_t *tile, int kept, int i, const uint8_t *codes, int d) {
	uint8_t c32[32];
	uint32_t w[6];
	for (int t = 0; t < 3; t++)
		for (int g = 0; g < (t == 2 ? kept : 4); g++) {
			for (int j = 0; j < 32; j++) { const int k = 128 * t + 32 * g + j; c32[j] = k < d ? codes[k] : 0; }
			fp6_pack32(c32, w);
			fp6_store_lane(tile + (size_t)t * 1536, t == 2 ? kept : 4, 16 * g + i, w);
		}
}
// The last K-step of a compact tile: lane 16 g + i (g = 0, 1) stores words 0 .. 2 in part P at 12 lane, quarter 0 its words 3 .. 5 in
// part Q at 384 + 12 lane; quarter 1's words 3 .. 5 are features 304 .. 319, zero codes, and are not stored
VK_HOST_DEVICE inline void fp6c_store_lane(uint8_t *step, int lane, const uint32_t *w) {
	uint32_t *p = reinterpret_cast<uint32_t *>(step + (size_t)lane * 12);
	p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
	if (lane >= 16) return;
	uint32_t *q = reinterpret_cast<uint32_t *>(step + 384 + (size_t)lane * 12);
	q[0] = w[3]; q[1] = w[4]; q[2] = w[5];
}
// one row's codes (d <= 304 of them, zeros beyond) into row i of a compact tile
inline void fp6c_put_row(uint8_t *tile, int i, const uint8_t *codes, int d) {
	fp6_put_row(tile, 0, i, codes, d);   // the two whole K-steps
	uint8_t c32[32];
	uint32_t w[6];
	for (int g = 0; g < 2; g++) {
		for (int j = 0; j < 32; j++) { const int k = 256 + 32 * g + j; c32[j] = k < d ? codes[k] : 0; }
		fp6_pack32(c32, w);
		fp6c_store_lane(tile + 2 * 1536, 16 * g + i, w);
	}
}

// ---- the query's side.  The constants of query column j in a cell of the bound pass, ub = clip01((s_x cs) I + e_x ca + cb) (I the
// exact product of the codes): cs = s_q, ca = a_q, cb = e_q N + gamma, with N >= every |s_x xq| of the corpus and X >= every |x| of
// it.  gamma: twice d_pad 2^-24 a_q X for the fp32 accumulation of the exact kernel's MFMA cosine and the five
// roundings of the bound's own evaluation, plus 2e-6 absolute for the same roundings near zero.  Rounded up.
inline void bound_cell_constants(const quant_meta &q, float N, float X, int d_pad, float *cs, float *ca, float *cb) {
	const double gamma = 2.0 * (double)d_pad * std::ldexp(1.0, -24) * (double)q.a * (double)X + 2e-6;
	*cs = q.s; *ca = q.a;
	*cb = quant_up((double)q.e * (double)N + gamma);
}
// The query's bound tile: rows (len_t <= 16 of fmt.d floats: the query as stored, bf16-rounded) quantized like the shadow's and laid
// out like a shadow tile with every K-step whole, then cs[16], ca[16], cb[16] -- zeros for the rows past the query, so that their
// cells are the exact kernel's zeros.  False, and `out` as it was, when an element is not finite: no bound for this query.
inline bool pack_bound_query(const shadow_format &fmt, const float *rows, int len_t, float N, float X, std::vector<uint8_t> &out) {
	const int d = fmt.d;
	for (int k = 0; k < len_t * d; k++)
		if (!(fabsf(rows[k]) <= 3.4028234e38f)) return false;
	std::vector<uint8_t> t((size_t)fmt.qtile_bytes() + 3 * 16 * 4, 0), codes((size_t)d);
	float *cst = reinterpret_cast<float *>(t.data() + (size_t)fmt.qtile_bytes());
	for (int i = 0; i < len_t; i++) {
		const float *x = rows + (size_t)i * d;
		uint8_t *xq = codes.data();
		quant_meta m;
		if (fmt.bits == 8) { m = quantize_row_i8(x, d, reinterpret_cast<int8_t *>(xq)); i8_put_row(t.data(), i, xq, d); }
		else { m = quantize_row_e2m3(x, d, xq); fp6_put_row(t.data(), 4, i, xq, d); }
		bound_cell_constants(m, N, X, fmt.gamma_width, &cst[i], &cst[16 + i], &cst[32 + i]);
	}
	out.swap(t);
	return true;
}

// ---- when a handle stops trying the bound pass: after 5 fallbacks to the full pass among its last 8 bound passes the
// next 64 queries go without one.  A stream of queries whose bounds never separate thus pays at most 8 wasted bound passes per 72
// queries.  take(): does this query try the bound pass; record(): how the bound pass of a query that took it ended.
struct bound_backoff {
	uint32_t recent = 0;   // fallbacks among the last 8 bound passes, one bit each
	int skip = 0;          // queries still to go without a bound pass
	bool take() {
		if (skip > 0) { skip--; return false; }
		return true;
	}
	void record(bool fell_back) {
		recent = ((recent << 1) | (fell_back ? 1u : 0u)) & 0xffu;
		if (fell_back && __builtin_popcount(recent) >= 5) { skip = 64; recent = 0; }
	}
};

// ---- the flat tail of the slice-gap table: under general gaps the bound kernel may score under
//     w'(k) = w(k) for k <= K,   w'(k) = c_tail = min over K < j <= rows of w(j) for k > K         (rows: 32 or 64, the form's history)
// which is <= w entry by entry, so its scores bound those under w from above.  w[0 .. rows]; a minimum, not w[K + 1]: the table need
// not rise.  K >= rows: no entry is in the tail, +inf (the identity of the minimum; no row of the kernel reads it).
inline float bound_tail_cost(const float *w, int k, int rows) {
	float c = INFINITY;
	for (int j = k + 1; j <= rows; j++) c = w[j] < c ? w[j] : c;
	return c;
}
// VK_BOUND_TAIL as the environment holds it (null: unset) and VK_BOUND_PASS as bound_pass_mode reads it (-1 off, 0 by size, 1 force):
// "0" never, "1" use the tail, anything else the default -- on where the pass is switched on by size, off under force (the tests of
// the bound pass pin its bounds and the size of round 2 under force, as they pinned the 8-bit shadow: bound_bits_wanted)
inline bool bound_tail_choice(const char *env, int mode) {
	if (env && !strcmp(env, "0")) return false;
	if (env && !strcmp(env, "1")) return true;
	return mode == 0;
}

} // namespace vk_host

#endif
