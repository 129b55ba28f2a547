"""Shared by the tests of both bound passes: the int8 quantizer of vk_host::quantize_row_i8 and the constants of a query
column restated in numpy, the block order of an int8 tile, the handle's shadow read back from the device, the build of the host
driver, and what the GPU modules of the pass have in common -- the environment of a block, a corpus with and without a shadow, the
counters of the last query, the comparison of two result sets.  The E2M3 side of the restatements is tests/bound6_cases.py."""

import ctypes as C
import os
import subprocess

import numpy as np

from bound6_cases import round2_limit as limit_of, stored, up   # noqa: F401 (the GPU modules take them from here)
from vectorian_amd import synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorian_amd", "csrc")


class Env:
	"""environment variables for the duration of a block (None: unset) -- VK_BOUND_PASS and VK_BOUND_BITS, which the library reads at
	finalize and per query"""

	def __init__(self, **values):
		self.values = values

	def __enter__(self):
		self.old = {k: os.environ.get(k) for k in self.values}
		self.set(self.values)

	def __exit__(self, *exc):
		self.set(self.old)

	@staticmethod
	def set(values):
		for k, v in values.items():
			if v is None:
				os.environ.pop(k, None)
			else:
				os.environ[k] = v


def build_driver(tmp_path_factory, name):
	"""tests/<name>.cpp (a stand-alone program over vk_bound_host.h and nothing else) built with g++ under AddressSanitizer and UBSan;
	returns run(command, *numbers) -> the lines it prints"""
	exe = str(tmp_path_factory.mktemp(name) / name)
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
		"-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)

	def run(what, *numbers):
		out = subprocess.run([exe, what], input=" ".join(str(x) for x in numbers), check=True, capture_output=True, text=True)
		return out.stdout.split("\n")[:-1]
	return run


def hexbits(x):
	return "%08x" % int(np.asarray(x, dtype=F).view(np.uint32))


def factory_args(d, bits, prec=0, layout=0):
	"""the arguments of vk_host::shadow_format_of for rows of d features: the exact kernel's nk32 and tail as vk_corpus_create derives
	them (d_pad a multiple of 16; bf16: K-steps of 32, the last one half filled; fp32: blocks of 16)"""
	d_pad = (d + 15) // 16 * 16
	nk32, tail = (d_pad // 16, 0) if prec else ((d_pad + 31) // 32, int(d_pad % 32 != 0))
	return [d, nk32, tail, prec, layout, bits]


def quantize8(x):
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
	return xq, s, F(up(np.sqrt(seq(dd * dd)))), F(up(np.sqrt(seq(xs * xs)))), F(up(np.sqrt(seq(x.astype(np.float64) ** 2))))


def constants8(s, e, n, a, N, X, d_pad):
	"""cs, ca, cb of a query column (vk_host::bound_cell_constants)"""
	gamma = 2.0 * d_pad * 2.0 ** -24 * float(a) * float(X) + 2e-6
	return s, a, F(up(float(e) * float(N) + gamma))


def pack_tile8(codes):
	"""codes: 16 rows x 64 nk64 int8 -> the bytes of the tile's blocks in the operand order of v_mfma_i32_16x16x64_i8: block k // 64 of
	1 KiB, in it lane 16 ((k % 64) // 16) + i holds row i, byte k % 16"""
	nk64 = codes.shape[1] // 64
	assert codes.shape == (16, 64 * nk64)
	return np.ascontiguousarray(codes.astype(np.int8).reshape(16, nk64, 4, 16).transpose(1, 2, 0, 3)).view(np.uint8).reshape(-1)


def shadow_of(hip, c, tile0=0, n=None):
	"""the handle's shadow as the device holds it: ({bits, steps, live, tile_bytes, tiles}, N, X, bytes [n, tile_bytes] of tiles
	tile0 .. tile0 + n - 1; all of them by default); no shadow: ({bits: 0, ...}, 0, 0, None)"""
	fn = hip.lib().vk_bound_pass_shadow
	fn.restype = C.c_int
	fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
	f = np.zeros(5, dtype=np.int64)
	nx = np.zeros(2, dtype=F)
	with c.lock:
		hip._check(fn(c._h, f.ctypes.data, nx.ctypes.data, 0, 0, None))
		fmt = dict(zip(("bits", "steps", "live", "tile_bytes", "tiles"), (int(v) for v in f)))
		if fmt["bits"] == 0:
			return fmt, nx[0], nx[1], None
		n = fmt["tiles"] - tile0 if n is None else n
		out = np.full((n, fmt["tile_bytes"]), 0xa5, dtype=np.uint8)
		hip._check(fn(c._h, f.ctypes.data, nx.ctypes.data, tile0, n, out.ctypes.data))
	return fmt, nx[0], nx[1], out


# ---- the GPU modules of the bound pass (test_gpu_bound_pass.py, test_gpu_bound_pass_768.py, test_gpu_bound6_pass.py)
V = 50_000


def corpus_of(hip, X, off):
	"""a finalized contextual corpus of the unit rows of X, rounded to bf16, in the slices off"""
	Xb = synth.to_bf16_bits(synth.normalize_rows(X))
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=Xb.shape[1], n_tokens=Xb.shape[0], n_sentences=len(off) - 1)
	c.append_vectors(Xb, normalize=False)
	c.set_sentences(off)
	c.finalize()
	return c


class Pair:
	"""the same vectors twice: `forced` has a shadow, `exact` has none.  env(mode): the environment of a block, the module's own"""

	def __init__(self, hip, env, corpus, X=None, off=None):
		self.corpus = corpus
		self.X = corpus["X"] if X is None else X
		self.off = np.asarray(corpus["sent_off"] if off is None else off, dtype=np.int64)
		self.n = len(self.off) - 1
		with env("off"):
			self.exact = corpus_of(hip, self.X, self.off)
		with env("force"):
			self.forced = corpus_of(hip, self.X, self.off)

	def close(self):
		self.forced.close()
		self.exact.close()


def state(hip, c, bounds=True):
	"""(bounds per slice or None, counters: ran, round 1, round 2, fell back, queries, fallbacks, survivors)"""
	lib = hip.lib()
	lib.vk_bound_pass_state.restype = C.c_int
	lib.vk_bound_pass_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
	cnt = np.zeros(7, dtype=np.int64)
	ub = np.empty(c.n_sentences, dtype=np.float32) if bounds else None
	with c.lock:
		hip._check(lib.vk_bound_pass_state(c._h, ub.ctypes.data if bounds else None, c.n_sentences, cnt.ctypes.data))
	return ub, cnt


def same_results(a, b):
	assert a.n == b.n
	n = a.n
	assert (a.score[:n].view(np.uint32) == b.score[:n].view(np.uint32)).all(), (a.score[:n], b.score[:n])
	assert (a.raw_score[:n].view(np.uint32) == b.raw_score[:n].view(np.uint32)).all()
	assert (a.sentence[:n] == b.sentence[:n]).all(), (a.sentence[:n], b.sentence[:n])
	assert (a.mapping[:n] == b.mapping[:n]).all()
	assert (a.edge_sim[:n].view(np.uint32) == b.edge_sim[:n].view(np.uint32)).all()


def ragged_with_empties(d, n, seed):
	"""n slices of 1..64 tokens, five of them emptied in place (first, inside a group, last)"""
	corpus = synth.make_contextual_corpus(n - 5, 1, 64, V, d, seed=seed)
	off = corpus["sent_off"]
	at = np.array([0, 7, (n - 5) // 2, n - 6, n - 5])
	corpus["sent_off"] = np.insert(off, at, off[at])
	assert len(corpus["sent_off"]) - 1 == n and (np.diff(corpus["sent_off"]) == 0).sum() == 5
	return corpus


def case_queries(corpus, len_t):
	"""The queries of a case: a noisy copy of len_t consecutive corpus tokens and len_t words drawn uniformly from the vocabulary
	(synth.make_queries' two kinds).  One token: the drawn word only -- a one-token query is a lookup of one word, the corpus draws its
	words from a Zipf law, and a copied token is a frequent word w.h.p.: hundreds to thousands of slices then hold that very word and tie
	within the quantization error (measured on the 4,000 x 32 shape: 3,523 .. 3,966 slices reach theta), which is the tie case that
	test_a_frequent_word_falls_back states on its own."""
	qs = synth.make_queries(corpus, 2, len_t, seed=100 + len_t)
	return [q["vectors"] for q in (qs[1:] if len_t == 1 else qs)]


def quantized8(x):
	"""the quantizer of vk_host::quantize_row_i8 over all rows at once: (e >= |x - s xq|, n >= |s xq|, a >= |x|) per row, each with a
	relative 1e-5 on top (the library rounds its double sums up by 1e-6)"""
	s = (np.abs(x).max(axis=1) / np.float32(127)).astype(np.float32)
	safe = np.where(s > 0, s, np.float32(1))
	xq = np.clip(np.rint(x / safe[:, None]), -127, 127) * (s > 0)[:, None]
	xs = s.astype(np.float64)[:, None] * xq
	norm = lambda t: np.sqrt((t * t).sum(axis=1)) * (1 + 1e-5)
	return norm(x.astype(np.float64) - xs), norm(xs), norm(x.astype(np.float64))


def round2_limit8(pair, qv, full, k, min_score, d_pad):
	"""(delta, the most slices round 2 can hold), from the exact scores `full` and the formats alone.  A cell of the bound exceeds the
	exact cosine by at most delta = 2 max (e_x a_q + e_q N) + gamma + 2e-5 (the Cauchy-Schwarz terms are added where the
	true quantization error may be as far below zero, at their largest over corpus and query; 2e-5 is the exact kernel's own rounding;
	gamma with the exact kernel's d_pad); a score is its at most len_t matched cells over len_t, so bound - exact <= delta per slice.
	Round 1 scores the M >= kk largest bounds: the kk-th largest bound is >= the kk-th best exact score s_kk, so theta >= s_kk - delta
	(or theta is the floor, when s_kk - delta is not above it or fewer than kk slices are).  A slice of round 2 has bound >= theta,
	hence exact >= theta - delta (bound6_cases.round2_limit counts them)."""
	if not hasattr(pair, "quant"):
		e, n, a = quantized8(stored(pair.X))
		pair.quant = (e.max(), n.max(), a.max())
	e_x, N, X = pair.quant
	e_q, _, a_q = quantized8(stored(qv))
	gamma = 2 * d_pad * 2.0 ** -24 * a_q * X + 2e-6
	delta = float((2 * (e_x * a_q + e_q * N) + gamma).max()) * (1 + 1e-5) + 2e-5
	return delta, limit_of(delta, full, k, pair.n, min_score)
