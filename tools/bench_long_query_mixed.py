#!/usr/bin/env python3
"""Queries of 65 .. 512 tokens over a corpus of sentences that holds some long ones: time of one query at the C-ABI (vk_query: the
pass over the slices of at most 64 tokens, the block form's pass over the others, selection, tracebacks of the winners) for each query
length and gap family, over `--slices` slices of which `--long-share` have `--long-min` .. `--long-max` tokens -- and, on the same
tokens, over the same corpus with every long slice cut to 64 tokens (what the second pass costs).  One JSON line per case.

  python tools/bench_long_query_mixed.py --slices 200000 --long-share 0.02
  python tools/bench_long_query_mixed.py --cut-only --label parent      # a corpus without long slices: runs on any build of the library
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--slices", type=int, default=200000)
	ap.add_argument("--long-share", type=float, default=0.02)
	ap.add_argument("--long-min", type=int, default=65)
	ap.add_argument("--long-max", type=int, default=300)
	ap.add_argument("--d", type=int, default=300)
	ap.add_argument("--len-t", default="65,100,200,512")
	ap.add_argument("--gaps", default="linear,exp5")
	ap.add_argument("--reps", type=int, default=3)
	ap.add_argument("--cut-only", action="store_true", help="time the cut corpus only (no slice of more than 64 tokens)")
	ap.add_argument("--label", default="", help="copied into every line (which build of the library ran)")
	args = ap.parse_args()

	from vectorian_amd import core, synth
	core.init(0)
	rng = np.random.default_rng(4321)
	lens = rng.integers(4, 65, size=args.slices)
	long_at = rng.random(args.slices) < args.long_share
	lens[long_at] = rng.integers(args.long_min, args.long_max + 1, size=int(long_at.sum()))
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	T, d, V = int(off[-1]), args.d, 50000
	Eb = synth.to_bf16_bits(synth.normalize_rows(synth.make_vocab(V, d)))
	Xb = Eb[synth.zipf_ids(T, V, rng)]           # (a token is its word's vector: the times do not depend on the values)
	w = ("table", (1 - 2.0 ** (-np.arange(0, 513) / 5)).astype(np.float32))
	gaps = {"linear": dict(gap_s=0.1, gap_t=0.1), "exp5": dict(gap_s=w, gap_t=w)}
	s = int(np.argmax(lens))
	corpora = [("cut", off[:-1], np.minimum(off[1:], off[:-1] + 64))]
	if not args.cut_only:
		corpora.insert(0, ("mixed", off[:-1], off[1:]))
	for name, start, end in corpora:
		c = core.Corpus(layout=core.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=T, n_sentences=args.slices)
		c.append_vectors(Xb, normalize=False)
		c.set_slices(start, end)
		c.finalize()
		for len_t in [int(x) for x in args.len_t.split(",")]:
			toks = (int(off[s]) + np.arange(len_t)) % T   # quotes the longest slice from its first token on
			Q = synth.bf16_bits_to_f32(Xb[toks]) + 0.05 * rng.standard_normal((len_t, d)).astype(np.float32)
			Qb = synth.to_bf16_bits(synth.normalize_rows(Q))
			for gap in args.gaps.split(","):
				kw = dict(locality=0, max_matches=10, **gaps[gap])
				got = c.query(Qb, q_normalize=False, **kw)   # warm-up (buffers, work list)
				times, score_ms, flow_ms = [], [], []
				for _ in range(args.reps):
					t0 = time.perf_counter()
					got = c.query(Qb, q_normalize=False, **kw)
					times.append((time.perf_counter() - t0) * 1e3)
					tm = c.last_timings()
					score_ms.append(tm["score_ms"]); flow_ms.append(tm["flow_ms"])
				print(json.dumps({"corpus": name, "label": args.label, "slices": args.slices, "long_slices": int(((end - start) > 64).sum()), "longest": int((end - start).max()),
					"tokens": int((end - start).sum()), "d": d, "len_t": len_t, "gap": gap, "query_ms": round(float(np.median(times)), 3),
					"score_ms": round(float(np.median(score_ms)), 3), "flow_ms": round(float(np.median(flow_ms)), 3), "reps": args.reps,
					"top": [int(got.sentence[0]), round(float(got.score[0]), 6)], "quoted": s}), flush=True)
		c.close()


if __name__ == "__main__":
	main()
