"""CPU tier: the host side of the 6-bit bound pass -- vk_host::quantize_row_e2m3, e2m3_eighths, the packer of a tile,
the format of the shadow and the query's bound tile in vk_bound_host.h, the functions both the query's tile and the shadow's kernel
are made of -- run through a g++ driver under AddressSanitizer and UBSan (the stand-alone program tests/bound6_driver.cpp) and held
against their statement in numpy (tests/bound6_cases.py):
  * every code decodes to a value of the grid, and the quantizer emits the nearest one, ties to the even multiple of the step;
  * the largest component of a row maps to +-7.5; e is at least the true norm of the residual in float64;
  * rows of zeros, one-hot rows, rows of 1e-30 and of 1e30;
  * the bytes of a packed tile are the layout the kernel reads;
  * the format of the 6-bit shadow is the table written out here at every width of the form, and the query's tile
    (vk_host::pack_bound_query) is pack_tile's bytes with constants()'s numbers behind them;
  * a cell of the bound is >= the float64 cosine of the stored rows for 10,000 random pairs at 289, 300 and 304 features -- and is
    not once e is taken for 0, so the test can tell."""

import numpy as np
import pytest

import bound6_cases as b6
import bound_cases as bc
from bound_cases import hexbits

F = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	return bc.build_driver(tmp_path_factory, "bound6_driver")


def quantize_by_driver(driver, rows):
	"""(codes, s, e, n, a) of float32 rows from the library's quantizer"""
	out = driver("quantize", len(rows), rows.shape[1], *[hexbits(v) for v in rows.reshape(-1)])
	assert len(out) == len(rows)
	f = [line.split() for line in out]
	meta = np.array([[int(w, 16) for w in t[:4]] for t in f], dtype=np.uint32).view(F)
	codes = np.array([[int(w) for w in t[4:]] for t in f], dtype=np.uint8).reshape(len(rows), rows.shape[1])
	return codes, meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]


def test_every_code_is_a_grid_value(driver):
	got = [int(v) for v in driver("decode")]
	assert got == b6.EIGHTHS.tolist()
	# sign, two exponent bits, three mantissa bits, bias 1, subnormals at exponent 0: the operand format of the scaled MFMA
	for code in range(64):
		e, m = (code >> 3) & 3, code & 7
		v = m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)
		assert got[code] == (-1 if code & 32 else 1) * v * 8


def test_ties_clip_and_special_rows(driver):
	# s = 7.5 / 7.5 = 1: the components are their own quotients.  Midpoints of every step go to the even multiple of the step.
	ties = np.array([[7.5, 0.0625, 0.1875, -0.3125, 1.9375, 2.125, 2.375, -3.875, 4.25, 4.75, 7.25, -7.5, 0.06, 0.07, 1.99, 3.9, 0.0]], dtype=F)
	want = np.array([7.5, 0.0, 0.25, -0.25, 2.0, 2.0, 2.5, -4.0, 4.0, 5.0, 7.0, -7.5, 0.0, 0.125, 2.0, 4.0, 0.0])
	codes, s, e, n, a = quantize_by_driver(driver, ties)
	assert s[0] == F(1)
	assert (b6.EIGHTHS[codes[0]] / 8 == want).all(), b6.EIGHTHS[codes[0]] / 8
	assert codes[0, 1] == 0 and codes[0, -1] == 0                 # no negative zero
	d = 300
	rng = np.random.default_rng(3)
	rows = b6.stored(rng.standard_normal((8, d)).astype(F))
	rows[0] = 0.0                                                # a row of zeros
	rows[1] = 0.0; rows[1, 17] = -1.0                            # one-hot
	rows[2] = F(1e-30) * rows[2]                                 # tiny throughout: s is a denormal-range quotient
	rows[3] = F(1e30) * rows[3]                                  # huge throughout
	rows[4] = 1e-3 * rows[4]; rows[4, 1] = 0.9999                # one dominant component
	codes, s, e, n, a = quantize_by_driver(driver, rows)
	rc, rs, re, rn, ra = b6.quantize6(rows)
	assert (codes == rc).all()
	for got, ref in ((s, rs), (e, re), (n, rn), (a, ra)):
		assert (got.view(np.uint32) == ref.view(np.uint32)).all(), (got, ref)
	assert (codes[0] == 0).all() and s[0] == 0 and e[0] == 0 and n[0] == 0 and a[0] == 0
	assert codes[1, 17] == 63 and (np.delete(codes[1], 17) == 0).all() and e[1] <= 1e-6
	for r in range(1, 8):
		k = int(np.argmax(np.abs(rows[r])))
		assert codes[r, k] == (63 if rows[r, k] < 0 else 31)       # the largest component is +-7.5
		true = np.sqrt(((rows[r].astype(np.float64) - b6.values(codes[r:r + 1], s[r:r + 1])[0]) ** 2).sum())
		assert float(e[r]) >= true and np.isfinite(e[r])
		assert float(e[r]) <= true * (1 + 1e-5) + 1e-45


@pytest.mark.parametrize("live6", (1, 2, 4))
def test_packed_tile_is_the_layout_the_kernel_reads(driver, live6):
	d = 256 + 32 * live6 - (5 if live6 == 2 else 0)              # 315 at live6 = 2: zero codes past d inside a live quarter
	rng = np.random.default_rng(live6)
	codes = np.zeros((16, 384), dtype=np.uint8)
	codes[:, :d] = rng.integers(0, 64, size=(16, d))
	out = driver("pack", live6, d, *codes[:, :d].reshape(-1).tolist())
	got = np.array([int(v) for v in out[0].split()], dtype=np.uint8)
	assert len(got) == 2 * 1536 + 384 * live6
	assert (got == b6.pack_tile(codes, live6)).all()


@pytest.mark.parametrize("d", (289, 300, 304))
def test_every_cell_of_the_bound_is_above_the_cosine(d, driver):
	rng = np.random.default_rng(d)
	X = b6.stored(rng.standard_normal((100, d)).astype(F))
	Q = b6.stored(rng.standard_normal((50, d)).astype(F) + 0.6 * X[:50])   # half of the queries near a corpus row: cosines up to ~0.5
	Q = np.concatenate([Q, b6.stored(rng.standard_normal((50, d)).astype(F))])
	xc, s_x, e_x, n_x, a_x = quantize_by_driver(driver, X)
	qc, s_q, e_q, n_q, a_q = quantize_by_driver(driver, Q)
	rc, rs, re, rn, ra = b6.quantize6(X)
	assert (xc == rc).all() and all((g.view(np.uint32) == r.view(np.uint32)).all() for g, r in ((s_x, rs), (e_x, re), (n_x, rn), (a_x, ra)))
	N, Xmax = n_x.max(), a_x.max()
	P = (b6.EIGHTHS[qc] @ b6.EIGHTHS[xc].T).astype(np.float64) / 64          # exact: multiples of 1 / 64 below 2^24 / 64
	assert (np.abs(P * 64) < 2 ** 21 + 1).all() and (P.astype(F).astype(np.float64) == P).all()
	exact = np.clip(Q.astype(np.float64) @ X.astype(np.float64).T, 0.0, 1.0)   # 10,000 pairs

	def cells(e_rows, e_query):
		cs, ca, cb = b6.constants(s_q, e_query, a_q, N, Xmax)
		ub = ((s_x[None, :] * cs[:, None]).astype(F) * P.astype(F)).astype(F)   # the kernel's order of operations, float32 throughout
		ub = ((ub + (e_rows[None, :] * ca[:, None]).astype(F)).astype(F) + cb[:, None]).astype(F)
		return np.clip(ub, F(0), F(1)).astype(np.float64)
	ub = cells(e_x, e_q)
	assert exact.size == 10_000 and (ub >= exact).all(), (ub - exact).min()
	assert (ub - exact).max() < 0.15                              # ... and a bound worth having
	# without the residual norms the same cells are no bound: the test can tell a bound from an estimate
	zero = np.zeros_like(e_x)
	assert (cells(zero, np.zeros_like(e_q)) < exact).any()


def test_format_of_the_6bit_shadow(driver):
	"""three K-steps of 128 features, 2 x 1536 + 384 live6 + 128 bytes per tile with live6 the quarters of 32 that hold features, a
	query tile of 4,608 bytes, gamma over the exact kernel's 320; none beside the widths"""
	widths = (289, 300, 303, 304)
	asked = [bc.factory_args(d, 6) for d in widths]
	out = driver("format", len(asked), *sum(asked, []))
	for d, line in zip(widths, out):
		live6 = -(-(d - 256) // 32)
		tile = 2 * 1536 + 384 * live6 + 128
		assert live6 == 2 and [int(v) for v in line.split()] == [6, 3, 128, live6, tile, tile - 128, 4608, 320], (d, line)
	none = [bc.factory_args(d, 6) for d in (288, 305, 752, 769)] + [bc.factory_args(300, 6, prec=1), bc.factory_args(300, 6, layout=1)]
	assert driver("format", len(none), *sum(none, [])) == ["none"] * len(none)


def test_query_tile_of_the_6bit_pass(driver):
	"""pack_bound_query at 300-d for queries of 1, 10 and 16 rows: every K-step whole, zeros past the query and past d, cs / ca / cb
	behind them; a query with an infinite element has no bound"""
	d = 300
	rng = np.random.default_rng(11)
	Q = b6.stored(rng.standard_normal((16, d)).astype(F))
	Q[2] = 0.0
	N, X = F(1.0078125), F(1.015625)
	for len_t in (1, 10, 16):
		out = driver("query_tile", *bc.factory_args(d, 6), len_t, hexbits(N), hexbits(X), *[hexbits(v) for v in Q[:len_t].reshape(-1)])
		got = np.array([int(v) for v in out[0].split()], dtype=np.uint8)
		codes = np.zeros((16, 384), dtype=np.uint8)
		cst = np.zeros((3, 16), dtype=F)
		qc, s, e, n, a = b6.quantize6(Q[:len_t])
		codes[:len_t, :d] = qc
		cst[:, :len_t] = b6.constants(s, e, a, N, X)
		assert len(got) == 4608 and (got == b6.pack_tile(codes, 4)).all()
		assert out[1].split() == [hexbits(v) for v in cst.reshape(-1)]
	Q[9, 299] = -np.inf
	assert driver("query_tile", *bc.factory_args(d, 6), 10, hexbits(N), hexbits(X), *[hexbits(v) for v in Q[:10].reshape(-1)]) == ["none"]
