#!/usr/bin/env python3
"""CPU simulation of the bound pass under six quantizers of the shadow -- int8 (s = max|x| / 127), int6 (s = max|x| / 31),
E2M3 (s = max|x| / 7.5), E2M3 as the compact shadow stores it (e2m3c: s and e rounded UP to bf16, the codes computed with
that s) and the two 4-bit grids E2M1 (0, 0.5, 1, 1.5, 2, 3, 4, 6; s = max|x| / 6) and int4 (s = max|x| / 7) -- on a `synth` corpus of n slices x 32 tokens x 300-d, generated and scored one chunk at a
time.  No GPU: the exact scores are the oracle's (bf16 rows, `want_all_scores`), the bounds are the oracle's DP over a numpy
restatement of the bound cell (`S_rows`: ub = clip01((s_x s_q) q^ . x^ + e_x a_q + e_q N + gamma), float32 in the kernel's order), and
rounds 1 and 2 are taken as vk_query.cpp takes them (M = 64 largest bounds, theta = the kk-th best exact score among them, kk = 18;
round 2 = the slices whose bound reaches theta).  Per query and quantizer: bound - exact (max, mean) and the size of round 2.

Queries are built by the rule of bench.make_queries (even-numbered: a noisy copy of ten consecutive tokens of a slice, here of the
first chunk; odd-numbered: ten random words), with its seed; the benchmark's own corpus is drawn on the GPU, so these are queries
of the same kind, not the same vectors.  N and X, the corpus-wide constants of the bound, are the first chunk's maxima widened by
5e-3; the output says whether every later chunk stayed below them (`constants_hold`).

--tail K[,K...]: the E2M3 bounds once more per K under the slice-gap table made flat beyond K entries (w'(k) = w(k) for
k <= K, the minimum of w(K + 1 .. 32) beyond), which is what the flat-tailed bound kernels compute; per K the size of round 2 and
the largest (tail bound - full-table bound).

  python tools/sim_bound_bits.py --slices 1000000 --chunk 25000 --queries 16 --threads 16 --out profiles/bound_fp6_sim.json
  python tools/sim_bound_bits.py --slices 200000 --chunk 25000 --queries 16 --threads 16 --tail 3,4,6 --out profiles/bound_tail_sim.json
  python tools/sim_bound_bits.py --slices 200000 --chunk 25000 --queries 16 --threads 16 --out profiles/bound_compact_sim.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import vk_oracle as vo          # noqa: E402
from vectorian_amd import synth             # noqa: E402

F = np.float32
V, D, LEN_S, LEN_T, K, KK, M = 50_000, 300, 32, 10, 10, 18, 64
EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(F))


def up(v):
	v = np.asarray(v, dtype=np.float64)
	return np.where(v > 0, np.nextafter((v * (1.0 + 1e-6)).astype(F), F(np.inf)), F(0)).astype(F)


def grid_uniform(levels):
	def q(x):
		s = (np.abs(x).max(axis=1) / F(levels)).astype(F)
		safe = np.where(s > 0, s, F(1)).astype(F)
		return np.clip(np.rint(x / safe[:, None]), -levels, levels).astype(F) * (s > 0)[:, None], s
	return q


def grid_e2m3(x):
	s = (np.abs(x).max(axis=1) / F(7.5)).astype(F)
	safe = np.where(s > 0, s, F(1)).astype(F)
	t = np.minimum(F(7.5), np.abs(x / safe[:, None]))
	step = np.where(t < 2, F(0.125), np.where(t < 4, F(0.25), F(0.5))).astype(F)
	a = np.minimum(F(7.5), np.rint(t / step) * step).astype(F)
	return np.copysign(a, x) * (s > 0)[:, None], s


def bf16_up(v):
	"""the least bf16 value >= v (v >= 0), as float32"""
	u = np.ascontiguousarray(v, dtype=F).view(np.uint32).astype(np.uint64)
	return np.where(u & 0xffff, (u | 0xffff) + 1, u).astype(np.uint32).view(F)


def grid_e2m3_compact(x):
	"""vk_host::quantize_row<grid_e2m3> under bf16_meta: the scale rounded up to bf16 first, the codes computed with it"""
	s = bf16_up((np.abs(x).max(axis=1) / F(7.5)).astype(F))
	safe = np.where(s > 0, s, F(1)).astype(F)
	t = np.minimum(F(7.5), np.abs(x / safe[:, None]))
	step = np.where(t < 2, F(0.125), np.where(t < 4, F(0.25), F(0.5))).astype(F)
	a = np.minimum(F(7.5), np.rint(t / step) * step).astype(F)
	return np.copysign(a, x) * (s > 0)[:, None], s


E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=F)


def grid_e2m1(x):
	"""the nearest of the eight E2M1 magnitudes (a midpoint goes to the lower one)"""
	s = (np.abs(x).max(axis=1) / F(6)).astype(F)
	safe = np.where(s > 0, s, F(1)).astype(F)
	t = np.minimum(F(6), np.abs(x / safe[:, None]))
	mid = (E2M1[1:] + E2M1[:-1]) / 2
	a = E2M1[np.searchsorted(mid, t, side="left")]
	return np.copysign(a, x) * (s > 0)[:, None], s


QUANTIZERS = {"int8": grid_uniform(127), "int6": grid_uniform(31), "e2m3": grid_e2m3, "e2m3c": grid_e2m3_compact, "e2m1": grid_e2m1, "int4": grid_uniform(7)}


def quantize(name, x):
	"""x^ (float32, exact grid values), s, e >= |x - s x^|, n >= |s x^|, a >= |x|; e2m3c: e rounded up to bf16 as well"""
	xq, s = QUANTIZERS[name](x)
	xs = s.astype(np.float64)[:, None] * xq
	norm = lambda t: np.sqrt(np.einsum("ij,ij->i", t, t))
	e = up(norm(x.astype(np.float64) - xs))
	return xq, s, bf16_up(e) if name == "e2m3c" else e, up(norm(xs)), up(norm(x.astype(np.float64)))


def stored(x):
	return synth.bf16_bits_to_f32(synth.to_bf16_bits(synth.normalize_rows(x)))


def make_queries(corpus, n_queries, seed):
	"""bench.make_queries over the arrays of a synth corpus"""
	rng = np.random.default_rng(seed)
	E, ids, off = corpus["E"], corpus["tok_id"], corpus["sent_off"]
	qs = []
	for i in range(n_queries):
		qi = None
		if i % 2 == 0:
			s = int(rng.integers(0, len(off) - 1))
			st = int(off[s]) + int(rng.integers(0, LEN_S - LEN_T + 1))
			qi = ids[st:st + LEN_T].astype(np.int64)
		if qi is None:
			qi = rng.integers(0, V, size=LEN_T)
		qs.append(np.ascontiguousarray(E[qi] + 0.05 * rng.standard_normal((LEN_T, D)).astype(F), dtype=F))
	return qs


def flat_tailed(gap, k):
	"""the table flat beyond k entries: its tail costs the least of the entries k + 1 .. LEN_S (vk_host::bound_tail_cost)"""
	w = gap[1].copy()
	w[k + 1:] = w[k + 1:LEN_S + 1].min()
	return ("table", w)


def rounds(ub, ex, floor):
	"""(theta, size of round 2) as vk_query.cpp takes its rounds"""
	first = np.argsort(-ub, kind="stable")[:M]
	best = np.sort(ex[first][ex[first] > floor])[::-1]
	theta = float(best[KK - 1]) if len(best) >= KK else floor
	return theta, int((ub >= theta).sum() if len(best) >= KK else (ub > theta).sum())


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--slices", type=int, default=50_000)
	ap.add_argument("--chunk", type=int, default=25_000)
	ap.add_argument("--queries", type=int, default=8)
	ap.add_argument("--threads", type=int, default=16)
	ap.add_argument("--seed", type=int, default=3456, help="seed of the queries (bench.py draws its queries with 3456)")
	ap.add_argument("--tail", default="", help="K[,K...]: the E2M3 bounds again under the table flat beyond K entries")
	ap.add_argument("--quantizers", default=",".join(QUANTIZERS), help="which of " + ", ".join(QUANTIZERS))
	ap.add_argument("--out", default=None)
	a = ap.parse_args()
	tails = [int(x) for x in a.tail.split(",") if x]
	assert all(1 <= k < LEN_S for k in tails), tails
	t0 = time.time()
	n_chunks = (a.slices + a.chunk - 1) // a.chunk
	names = [q for q in a.quantizers.split(",") if q]
	assert all(q in QUANTIZERS for q in names) and (not tails or "e2m3" in names), names
	exact = np.empty((a.queries, a.slices), dtype=F)
	bound = {q: np.empty((a.queries, a.slices), dtype=F) for q in names}
	bound_tail = {k: np.empty((a.queries, a.slices), dtype=F) for k in tails}
	qs, qb, qq, const, holds = None, None, {}, {}, True
	for c in range(n_chunks):
		n = min(a.chunk, a.slices - c * a.chunk)
		corpus = synth.make_contextual_corpus(n, LEN_S, LEN_S, V, D, seed=synth.SEED_CORPUS + 17 * c)
		X = stored(corpus["X"])
		Xb = synth.to_bf16_bits(X)
		if c == 0:
			qs = [stored(q) for q in make_queries(corpus, a.queries, a.seed)]
			qb = [synth.to_bf16_bits(q) for q in qs]
		kw = dict(layout=vo.LAYOUT_CONTEXTUAL, d=D, sent_off=corpus["sent_off"], X=Xb, Qs=qb, locality=vo.LOCAL, gap_s=EXP5, gap_t=EXP5,
			max_matches=K, min_score=0.0, n_threads=a.threads, want_all_scores=True)
		lo = c * a.chunk
		for i, r in enumerate(vo.find_many(**kw)):
			exact[i, lo:lo + n] = r["all_scores"]
		for name in names:
			xq, s_x, e_x, n_x, a_x = quantize(name, X)
			if c == 0:
				const[name] = (F(n_x.max() * (1 + 5e-3)), F(a_x.max() * (1 + 5e-3)))
				qq[name] = [quantize("e2m3" if name == "e2m3c" else name, q) for q in qs]   # the query's tile is the same under either layout
			N, Xm = const[name]
			holds = holds and bool(n_x.max() <= N and a_x.max() <= Xm)
			P = xq @ np.concatenate([t[0] for t in qq[name]]).T          # exact in float32: see the module's text
			S = []
			for i, (_, s_q, e_q, _, a_q) in enumerate(qq[name]):
				gamma = 2.0 * 320 * 2.0 ** -24 * a_q.astype(np.float64) * float(Xm) + 2e-6
				cb = up(e_q.astype(np.float64) * float(N) + gamma)
				ub = ((s_x[:, None] * s_q[None, :]).astype(F) * P[:, i * LEN_T:(i + 1) * LEN_T]).astype(F)
				ub = ((ub + (e_x[:, None] * a_q[None, :]).astype(F)).astype(F) + cb[None, :]).astype(F)
				S.append(np.clip(ub, F(0), F(1)))
			for i, r in enumerate(vo.find_many(S_rows=S, **kw)):
				bound[name][i, lo:lo + n] = r["all_scores"]
			for k in tails if name == "e2m3" else ():
				for i, r in enumerate(vo.find_many(S_rows=S, **dict(kw, gap_s=flat_tailed(EXP5, k)))):
					bound_tail[k][i, lo:lo + n] = r["all_scores"]
		print(f"chunk {c + 1}/{n_chunks}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
	floor = -1e-5
	out = {"slices": a.slices, "tokens_per_slice": LEN_S, "d": D, "len_t": LEN_T, "k": K, "kk": KK, "round1": M, "gap": "exp5", "locality": "local",
		"query_seed": a.seed, "constants_hold": holds, "quantizers": {}}
	for name in names:
		rows = []
		for i in range(a.queries):
			ub, ex = bound[name][i], exact[i]
			assert (ub >= ex).all(), (name, i, float((ub - ex).min()))
			theta, round2 = rounds(ub, ex, floor)
			rows.append({"query": i, "planted": i % 2 == 0, "slack_max": round(float((ub - ex).max()), 5), "slack_mean": round(float((ub - ex).mean()), 5),
				"theta": round(theta, 5), "round2": round2})
		r2p = [r["round2"] for r in rows if r["planted"]]
		r2r = [r["round2"] for r in rows if not r["planted"]]
		out["quantizers"][name] = {"slack_max": max(r["slack_max"] for r in rows), "slack_mean": [min(r["slack_mean"] for r in rows), max(r["slack_mean"] for r in rows)],
			"round2_planted": [min(r2p), max(r2p)], "round2_random": [min(r2r), max(r2r)] if r2r else None,
			"round2_mean": round(float(np.mean(r2p + r2r)), 1), "round2_max": max(r2p + r2r), "fallback_line": max(a.slices // 16, 1024), "queries": rows}
		print(name, {k: v for k, v in out["quantizers"][name].items() if k != "queries"})
	if tails:
		out["tail"] = {"quantizer": "e2m3", "full_table_round2_mean": out["quantizers"]["e2m3"]["round2_mean"], "by_k": {}}
	for k in tails:
		rows = []
		for i in range(a.queries):
			ub, ex, ub_full = bound_tail[k][i], exact[i], bound["e2m3"][i]
			assert (ub >= ub_full).all(), (k, i, float((ub - ub_full).min()))   # a flat tail only raises a bound
			theta, round2 = rounds(ub, ex, floor)
			rows.append({"query": i, "planted": i % 2 == 0, "over_full_table_max": round(float((ub - ub_full).max()), 5), "theta": round(theta, 5), "round2": round2})
		r2p = [r["round2"] for r in rows if r["planted"]]
		r2r = [r["round2"] for r in rows if not r["planted"]]
		out["tail"]["by_k"][str(k)] = {"over_full_table_max": max(r["over_full_table_max"] for r in rows), "round2_planted": [min(r2p), max(r2p)],
			"round2_random": [min(r2r), max(r2r)] if r2r else None, "round2_mean": round(float(np.mean(r2p + r2r)), 1), "round2_max": max(r2p + r2r),
			"fallback_line": max(a.slices // 16, 1024), "queries": rows}
		print("tail", k, {key: v for key, v in out["tail"]["by_k"][str(k)].items() if key != "queries"})
	out["seconds"] = round(time.time() - t0)
	if a.out:
		with open(a.out, "w") as f:
			json.dump(out, f, indent=1)
			f.write("\n")


if __name__ == "__main__":
	main()
