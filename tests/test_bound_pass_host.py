"""CPU tier: the arithmetic of the 8-bit bound pass restated in numpy -- the quantizer of a row, the constants of a query
column, the cell of the bound kernel -- on random unit rows rounded to bf16 in 50, 300 and 768 dimensions, rows with one dominant
component and rows of zeros among them:
  * every cell of the bound is >= the float32 dot product of the bf16-rounded rows (what the exact kernel's cell approximates);
  * the host quantizer (vk_host::quantize_row_i8 and bound_cell_constants in vk_bound_host.h, the function both the query's tile
    and the shadow's kernel are made of), run through a g++ driver with AddressSanitizer and UBSan (the stand-alone program
    tests/bound_pass_driver.cpp), gives the restatement's numbers bit for bit;
  * the format of a shadow (vk_host::shadow_format_of) is the table written out here, at every width where it changes;
  * the query's 8-bit bound tile (vk_host::pack_bound_query) is the numpy packer's bytes, its constants constants()'s, and a query
    with an infinite element has none;
  * the rule by which a handle stops trying the bound pass (vk_host::bound_backoff) keeps its worst case."""

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import constants8 as constants, hexbits, quantize8 as quantize
from vectorian_amd import synth

F = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	return bc.build_driver(tmp_path_factory, "bound_pass_driver")


def rows_of(d, seed):
	rng = np.random.default_rng(seed)
	x = synth.normalize_rows(rng.standard_normal((40, d)).astype(F))
	x[3] = 0.0                                                   # a row of zeros
	x[4] = 0.0; x[4, d // 2] = 1.0                               # one component only
	x[5] = 1e-3 * x[5]; x[5, 1] = 0.9999                         # one dominant component: the others quantize to 0 or +-1
	x[6] = -x[7]                                                 # an opposite pair
	x[8] = 1e-30 * x[8]                                          # tiny throughout (a denormal scale)
	return synth.bf16_bits_to_f32(synth.to_bf16_bits(x))         # the rows as stored


@pytest.mark.parametrize("d", (50, 300, 768))
def test_every_cell_of_the_bound_is_above_the_dot_product(d, driver):
	X, Q = rows_of(d, 1), rows_of(d, 2)[:16]
	d_pad = (d + 63) // 64 * 64
	qx = [quantize(r) for r in X]
	qq = [quantize(r) for r in Q]
	N, Xmax = max(t[3] for t in qx), max(t[4] for t in qx)
	for j, (qh, s_q, e_q, n_q, a_q) in enumerate(qq):
		cs, ca, cb = constants(s_q, e_q, n_q, a_q, N, Xmax, d_pad)
		for i, (xh, s_x, e_x, n_x, a_x) in enumerate(qx):
			integer = int(qh.astype(np.int64) @ xh.astype(np.int64))
			assert abs(integer) < 2 ** 24
			ub = F(F(F(F(s_x * cs) * F(integer)) + F(e_x * ca)) + cb)   # the kernel's order of operations, float32 throughout
			ub = min(max(ub, F(0)), F(1))
			exact = min(max(F(np.dot(Q[j], X[i])), F(0)), F(1))
			exact64 = min(max(float(Q[j].astype(np.float64) @ X[i].astype(np.float64)), 0.0), 1.0)
			assert ub >= exact and float(ub) >= exact64, (d, i, j, ub, exact)
			if a_x > 0.5 and a_q > 0.5:
				assert float(ub) - exact64 < 0.05               # and it is a bound worth having
	# the host quantizer: the same numbers, bit for bit
	for rows, quant in ((X, qx), (Q, qq)):
		out = driver("quantize", len(rows), d, *[hexbits(v) for v in rows.reshape(-1)])
		for line, (xh, s, e, n, a) in zip(out, quant):
			f = line.split()
			assert f[:4] == [hexbits(s), hexbits(e), hexbits(n), hexbits(a)]
			assert [int(v) for v in f[4:]] == xh.tolist()
	args = []
	for _, s, e, n, a in qq:
		args += [hexbits(s), hexbits(e), hexbits(n), hexbits(a), hexbits(N), hexbits(Xmax), d_pad]
	out = driver("constants", len(qq), *args)
	for line, (_, s, e, n, a) in zip(out, qq):
		assert line.split() == [hexbits(v) for v in constants(s, e, n, a, N, Xmax, d_pad)]


# d -> live quarters of the last K-step; the 8-bit forms: (K-steps, bytes per tile, bytes of the query's tile, gamma's width)
LIVE8 = {289: 3, 300: 3, 303: 3, 304: 3, 753: 4, 768: 4}
FORM8 = {5: (5, 5248, 5120, 320), 12: (12, 12416, 12288, 768)}


def test_format_of_the_8bit_shadow(driver):
	"""the table of DESIGN 11.1; none beside the widths, for fp32 rows and for the static layout; six bits asked of 768-d rows: eight"""
	asked = [bc.factory_args(d, 8) for d in sorted(LIVE8)] + [bc.factory_args(d, 6) for d in (753, 768)]
	out = driver("format", len(asked), *sum(asked, []))
	for args, line in zip(asked, out):
		steps, tile, qtile, gamma = FORM8[5 if args[0] < 400 else 12]
		assert [int(v) for v in line.split()] == [8, steps, 64, LIVE8[args[0]], tile, tile - 128, qtile, gamma], (args, line)
	none = [bc.factory_args(d, b) for d in (288, 305, 752, 769, 50) for b in (8, 6)]
	none += [bc.factory_args(d, 8, prec=1) for d in (300, 768)] + [bc.factory_args(d, 8, layout=1) for d in (300, 768)]
	assert driver("format", len(none), *sum(none, [])) == ["none"] * len(none)


@pytest.mark.parametrize("d", (300, 768))
def test_query_tile_of_the_8bit_pass(d, driver):
	"""pack_bound_query for queries of 1, 10 and 16 rows: the codes in the block order, zeros past the query and past d, the constants
	with the exact kernel's padded K in gamma"""
	steps, _, qtile, gamma = FORM8[5 if d == 300 else 12]
	Q = rows_of(d, 5)[:16]
	N, X = F(1.0078125), F(1.015625)
	for len_t in (1, 10, 16):
		out = driver("query_tile", *bc.factory_args(d, 8), len_t, hexbits(N), hexbits(X), *[hexbits(v) for v in Q[:len_t].reshape(-1)])
		got = np.array([int(v) for v in out[0].split()], dtype=np.uint8)
		codes = np.zeros((16, 64 * steps), dtype=np.int8)
		want = [[hexbits(0)] * 16 for _ in range(3)]
		for i in range(len_t):
			xq, s, e, n, a = quantize(Q[i])
			codes[i, :d] = xq
			for j, v in enumerate(constants(s, e, n, a, N, X, gamma)):
				want[j][i] = hexbits(v)
		assert len(got) == qtile and (got == bc.pack_tile8(codes)).all()
		assert out[1].split() == sum(want, [])
	Q[3, 7] = np.inf
	assert driver("query_tile", *bc.factory_args(d, 8), 10, hexbits(N), hexbits(X), *[hexbits(v) for v in Q[:10].reshape(-1)]) == ["none"]


def test_back_off_after_repeated_fallbacks(driver):
	"""vk_host::bound_backoff: 5 fallbacks among the last 8 bound passes stop the handle's bound passes for 64 queries.  A stream whose
	bounds never separate wastes at most 8 bound passes per 72 queries; one that always separates never skips; four
	fallbacks in eight do not trip it."""
	def run(fell):
		out = driver("backoff", len(fell), *[int(f) for f in fell])
		return [int(x) for x in out]
	never = run([1] * 720)
	assert never[:5] == [1] * 5 and never[5:69] == [0] * 64 and never[69] == 1
	for start in range(0, 720 - 72):
		assert sum(never[start:start + 72]) <= 8
	assert run([0] * 300) == [1] * 300
	assert run([1, 0] * 150) == [1] * 300                        # 4 of every 8
	mixed = run([1, 1, 1, 0, 0, 0, 1, 1] + [0] * 100)
	assert mixed[:8] == [1] * 8 and mixed[8:72] == [0] * 64 and mixed[72:] == [1] * 36
