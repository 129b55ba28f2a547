"""The degenerate transport problems the LP tests share (test_transport_lp_host.py, test_gpu_transport_lp.py,
tools/make_transport_goldens.py): pure numpy, seeded, no GPU.

The exact stage of WRD and full WMD (vk_wrd_exact_kernel<1..4>, vk_wrd_exact_long_kernel<1|4>, vk_transport.hip) and the oracle's
vko_emd are the same successive-shortest-paths method, so the oracle cannot vouch for it where the method itself is at risk: under
ties.  Every family below is built from vectors (the library computes the similarities itself) and makes ties of one kind:

  types       six unit vectors drawn with repetition, rows scaled by 1, 2 or 4: bit-identical cost rows and columns, zero-length
              reduced-cost ties at every step, WRD masses that tie exactly; the static twin shares vocabulary ids between query and
              slice (sim[id][id] = 1: costs of exactly 0)
  axes        tokens +-e_i and (e_i + e_j) / sqrt 2: similarities on {<= 0 -> 0, 0.5, 0.707, 1}, costs full of exact 0s, exact 1s, ties
  assignment  continuous random unit vectors, len_t == len_s among the slices: with uniform masses every basic solution is degenerate
  skewed      continuous random similarities, row norms lognormal(0, 3): masses over five orders of magnitude (each at least 1e-6 of
              its side's total, so that the solvers' EPS = 1e-13 is not what the case measures)
  arc         points on an arc in two dimensions, the query's clustered and the slice's spread: nearly every unit of mass is rerouted
              through a chain of earlier shipments

A case: dict(name, family, layout, d, off, queries, search, and X (contextual: the token rows) or E + tok_id (static: vocabulary rows
and the tokens' ids)); a query: dict(vectors[, ids]).  Slices of no tokens are part of the short corpora."""

import hashlib

import numpy as np

# the four exact transports: name -> (algorithm, options common to the library's query() and the oracle's find())
MODES = {
	"wrd_norm": ("wrd", dict(wrd_normalize=True)),                        # balanced: the greedy start runs
	"wrd_raw": ("wrd", dict(wrd_normalize=False)),                        # raw magnitudes: unbalanced, no greedy start
	"nbow": ("wmd", dict(wmd_full=True, rwmd=(False, False, True))),      # masses 1 / len
	"bow": ("wmd", dict(wmd_full=True, rwmd=(False, False, False))),      # masses 1: unbalanced whenever len_t != len_s
}

FAMILIES = ("types", "axes", "assignment", "skewed", "arc")

# query lengths: 1, 2, 15, 16 take NQ = 1 (the register form), 17, 32 NQ = 2, 33, 48 NQ = 3, 49, 64 NQ = 4
SHORT_LEN_T = (1, 2, 15, 16, 17, 32, 33, 48, 49, 64)
# slices of at most 64 tokens (vk_wrd_exact_kernel), two of them empty
SHORT_LEN_S = (1, 2, 15, 0, 16, 17, 31, 32, 33, 63, 64, 0)
# long corpora: six slices of 65 .. 512 tokens (vk_wrd_exact_long_kernel) between short ones, so that launch_wrd_exact_both splits
# the candidates; queries of 16 tokens take the LDS form, 17, 40 and 64 the scratch form at nq 2, 3, 4
LONG_LEN_S = (65, 7, 127, 128, 33, 129, 511, 0, 512, 64)
LONG_LEN_T = (16, 17, 40, 64)
ASSIGNMENT_LEN = (16, 17, 32, 48, 64)


def _unit(x):
	return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _offsets(lens):
	return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


class _Family:
	"""rows(rng, n, query) -> float32 [n x d] token rows of one slice or one query"""

	def __init__(self, name, d, seed):
		self.name, self.d = name, d
		rng = np.random.default_rng(seed)
		if name == "types":
			self.types = _unit(rng.standard_normal((6, d)))
			self.scale = np.array([1, 2, 4, 1, 2, 4], dtype=np.float32)   # of a vocabulary entry (static twin)
		elif name == "axes":
			rows = [s * np.eye(d, dtype=np.float32)[i] for i in range(5) for s in (1.0, -1.0)]
			rows += [(np.eye(d)[i] + np.eye(d)[j]) / np.sqrt(2.0) for i in range(5) for j in range(i + 1, 5)]
			self.types = np.asarray(rows, dtype=np.float32)
		elif name in ("assignment", "skewed"):
			self.common = 0.7 * np.sqrt(d) * _unit(rng.standard_normal((1, d)))

	def ids(self, rng, n):
		return rng.integers(0, len(self.types), size=n).astype(np.int32)

	def rows(self, rng, n, query=False):
		d = self.d
		if self.name == "types":
			return self.types[self.ids(rng, n)] * rng.choice(np.array([1, 2, 4], dtype=np.float32), size=(n, 1))
		if self.name == "axes":
			return self.types[self.ids(rng, n)].copy()
		if self.name == "assignment":
			return _unit(rng.standard_normal((n, d)) + self.common)
		if self.name == "skewed":
			norm = rng.lognormal(0.0, 3.0, size=n)
			norm = np.maximum(norm, 4e-6 * norm.sum())   # every mass at least 1e-6 of the side's total (the floor moves the total by < n 4e-6)
			return (_unit(rng.standard_normal((n, d)) + self.common) * norm[:, None]).astype(np.float32)
		# arc: the query in a third of the quarter circle (query == "wide": over all of it), the slice over all of it; magnitudes 0.5 .. 2
		lo, hi = (0.55, 1.05) if query is True else (0.0, np.pi / 2)
		th = rng.uniform(lo, hi, size=n)
		x = np.zeros((n, d), dtype=np.float32)
		x[:, 0], x[:, 1] = np.cos(th), np.sin(th)
		return (x * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)


def _contextual(name, family, d, seed, len_s, len_t, search=False, per_mode=False):
	"""len_t: query lengths; (n, "wide"): a query drawn as the slices are.  per_mode: the GPU tier runs each mode as a test of its own"""
	fam = _Family(family, d, seed)
	rng = np.random.default_rng(seed + 1)
	X = np.concatenate([fam.rows(rng, int(n)) for n in len_s] + [np.zeros((0, d), np.float32)]).astype(np.float32)
	queries = [dict(vectors=fam.rows(rng, int(n[0]), query=n[1]) if isinstance(n, tuple) else fam.rows(rng, int(n), query=True)) for n in len_t]
	return dict(name=name, family=family, layout="contextual", d=d, X=X, off=_offsets(len_s), queries=queries, search=search, per_mode=per_mode)


def _static(name, family, d, seed, len_s, len_t, search=False):
	"""the vocabulary is the family's types (each with one magnitude); slices and queries are ids into it, shared between them"""
	fam = _Family(family, d, seed)
	rng = np.random.default_rng(seed + 1)
	E = (fam.types * fam.scale[:, None]).astype(np.float32)
	tok_id = np.concatenate([fam.ids(rng, int(n)) for n in len_s] + [np.zeros(0, np.int32)]).astype(np.int32)
	queries = []
	for n in len_t:
		ids = fam.ids(rng, int(n))
		queries.append(dict(vectors=E[ids], ids=ids))
	return dict(name=name, family=family, layout="static", d=d, E=E, tok_id=tok_id, off=_offsets(len_s), queries=queries, search=search, per_mode=False)


def _search_lens(seed, n):
	return np.random.default_rng(seed).integers(1, 41, size=n)


_CACHE = None


def cases():
	"""every case, built once"""
	global _CACHE
	if _CACHE is None:
		_CACHE = [
			_contextual("types_short", "types", 16, 100, SHORT_LEN_S, SHORT_LEN_T),
			_static("types_static_short", "types", 16, 100, SHORT_LEN_S, SHORT_LEN_T),
			_contextual("axes_short", "axes", 16, 200, SHORT_LEN_S, SHORT_LEN_T),
			_contextual("assignment", "assignment", 32, 300, ASSIGNMENT_LEN, ASSIGNMENT_LEN),
			_contextual("skewed_short", "skewed", 32, 400, SHORT_LEN_S, SHORT_LEN_T),
			_contextual("arc_short", "arc", 16, 500, SHORT_LEN_S, SHORT_LEN_T),
			_contextual("types_long", "types", 16, 110, LONG_LEN_S, LONG_LEN_T),
			_contextual("axes_long", "axes", 16, 210, LONG_LEN_S, LONG_LEN_T),
			# skewed: most supplies are used up early, so the long solver's scan runs over nearly every supply in every round -- 64 query
			# tokens against 511 or 512 slice tokens take it 3 to 4.5 s per mode (types: 0.16 s).  That cell is a case of one long slice,
			# each mode a test of its own
			_contextual("skewed_long", "skewed", 32, 410, (65, 7, 127, 128, 33, 129, 0, 64), LONG_LEN_T),
			_contextual("skewed_long_512", "skewed", 32, 430, (511, 13, 512), (16, 17, 40)),
			_contextual("skewed_512_nq4", "skewed", 32, 440, (13, 512), (64,), per_mode=True),
			# arc: the long solver is one untuned wave per candidate and the chains make it augment eight times as often as on the other
			# families (4,355 augmentations at 64 x 511) -- with every cell of LONG_LEN_S x LONG_LEN_T the case took 59 s on an MI355X,
			# nearly all of it at 40 and 64 query tokens against 511 and 512 slice tokens.  The family's long slices therefore come in
			# several cases: 65 .. 129 tokens at nq 1, 2, 3; 511 and 512 at nq 1; 65 .. 129 at nq 4; and ONE slice of 512 tokens at each of
			# nq 2, 3, 4 -- the slice count cut, not the shape --, the latter four with each mode a test of its own
			_contextual("arc_long", "arc", 16, 510, (65, 7, 127, 128, 0, 129, 64), (16, 17, 40)),
			_contextual("arc_long_512", "arc", 16, 530, (511, 13, 512), (16,)),
			_contextual("arc_long_nq4", "arc", 16, 540, (65, 9, 127, 128, 129), (64,), per_mode=True),
			_contextual("arc_512_nq2", "arc", 16, 550, (13, 512), (17,), per_mode=True),
			_contextual("arc_512_nq3", "arc", 16, 560, (13, 512), (40,), per_mode=True),
			_contextual("arc_512_nq4", "arc", 16, 570, (13, 512), (64,), per_mode=True),
			# the search route: more slices than the 512 candidates of round 1, so that round 2 has to run.  arc's second query is
			# spread as the slices are: every token has a near neighbour, the relaxation (the bound's kind) is near 1 for most slices
			# while the exact score is not, and more than 512 bounds lie above the 64th and the 10th best exact score
			_static("types_search", "types", 16, 120, _search_lens(121, 800), (12,), search=True),
			_contextual("arc_search", "arc", 16, 520, _search_lens(521, 800), (20, (20, "wide")), search=True),
		]
	return _CACHE


def case(name):
	return next(c for c in cases() if c["name"] == name)


def input_hash(c):
	"""sha256 over the case's input arrays (dtype, shape and bytes of each)"""
	h = hashlib.sha256()
	arrays = [c["off"]] + ([c["X"]] if c["layout"] == "contextual" else [c["E"], c["tok_id"]])
	for q in c["queries"]:
		arrays.append(q["vectors"])
		if "ids" in q:
			arrays.append(q["ids"])
	for a in arrays:
		a = np.ascontiguousarray(a)
		h.update(f"{a.dtype.str}{a.shape}".encode())
		h.update(a.tobytes())
	return h.hexdigest()


def nq_of(len_t):
	return (len_t + 15) // 16


def coverage():
	"""(family, mode, NQ, 'short' | 'long') -> slices checked against the LP (empty slices not counted)"""
	table = {}
	for c in cases():
		lens = np.diff(c["off"])
		for q in c["queries"]:
			for mode in MODES:
				for kind, cnt in (("short", int(((lens > 0) & (lens <= 64)).sum())), ("long", int((lens > 64).sum()))):
					if cnt:
						k = (c["family"], mode, nq_of(len(q["vectors"])), kind)
						table[k] = table.get(k, 0) + cnt
	return table


if __name__ == "__main__":
	for k, v in sorted(coverage().items()):
		print("%-11s %-9s NQ=%d %-5s %5d" % (*k, v))
