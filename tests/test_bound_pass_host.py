"""CPU tier: the arithmetic of the 8-bit bound pass restated in numpy -- the quantizer of a row, the constants of a query
column, the cell of the bound kernel -- on random unit rows rounded to bf16 in 50, 300 and 768 dimensions, rows with one dominant
component and rows of zeros among them:
  * every cell of the bound is >= the float32 dot product of the bf16-rounded rows (what the exact kernel's cell approximates);
  * the host quantizer (vk_host::quantize_row_i8 and bound_cell_constants in vk_result_host.h, which vk_pack_query calls for the query's
    rows), run through a g++ driver with AddressSanitizer and UBSan, gives the restatement's numbers bit for bit;
  * the rule by which a handle stops trying the bound pass (vk_host::bound_backoff) keeps its worst case.
(The packing of the query's 8-bit tile in vk_pack_query is covered on the GPU only: bound >= exact score, tests/test_gpu_bound_pass.py.)"""

import os
import subprocess

import numpy as np
import pytest

from test_devbuf import CSRC, ROOT
from vectorian_amd import synth

F = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("bound_pass") / "bound_pass_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
		"-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "bound_pass_driver.cpp"), "-o", exe], check=True)

	def run(what, *numbers):
		out = subprocess.run([exe, what], input=" ".join(str(x) for x in numbers), check=True, capture_output=True, text=True)
		return out.stdout.split("\n")[:-1]
	return run


def hexbits(x):
	return "%08x" % int(np.asarray(x, dtype=F).view(np.uint32))


def up(v):
	"""a non-negative double rounded UP to float32 (quant_up)"""
	if not v > 0:
		return F(0)
	return np.nextafter(F(v * (1.0 + 1e-6)), F(np.inf))


def quantize(x):
	"""x: a float32 row.  Returns xq (int8), s, e >= |x - s xq|, n >= |s xq|, a >= |x| -- sums in double, in k order"""
	m = F(np.max(np.abs(x))) if len(x) else F(0)
	s = F(m / F(127))
	if s > 0:
		xq = np.clip(np.rint(x / s), -127, 127).astype(np.int8)
	else:
		xq = np.zeros(len(x), dtype=np.int8)
	xs = np.float64(s) * xq.astype(np.float64)
	dd = x.astype(np.float64) - xs
	seq = lambda t: float(np.cumsum(t)[-1]) if len(t) else 0.0   # sequential, as the C loop
	return xq, s, up(np.sqrt(seq(dd * dd))), up(np.sqrt(seq(xs * xs))), up(np.sqrt(seq(x.astype(np.float64) ** 2)))


def constants(s, e, n, a, N, X, d_pad):
	gamma = 2.0 * d_pad * 2.0 ** -24 * float(a) * float(X) + 2e-6
	return s, a, up(float(e) * float(N) + gamma)


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
