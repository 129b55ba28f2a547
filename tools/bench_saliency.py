#!/usr/bin/env python3
"""The booster of a Saliency on the device, measured: `--sentences` slices of `--len` tokens over a static embedding
(`--vocab` words of `--d` features), `--keywords` keywords, one max-smoothed and one gauss-smoothed keyword signal, documents of
`--doc-sentences` slices.

  python tools/bench_saliency.py --out profiles/saliency.json

(a) compile: vk_signal_keywords / vk_signal_filter / vk_corpus_set_saliency on the resident corpus against the same arithmetic in
    numpy / scipy on the host (the reference's route: per document a filter call, one np.average) -- host clocks, every native call
    ends in a synchronise; medians of `--repeats` runs after `--warmup`.
(b) query: the headline query (`--len-t` tokens, local alignment, general gaps 1 - 2^(-k/5), top 10 with tracebacks) with the boost
    passed per query as an array (today's path: scanned, remapped and copied per query) against the resident booster (boost=None), on
    the same handle in one process: wall time of Corpus.query and the library's prepare_ms, median and range of `--queries` queries
    each after `--warmup` more.  The two result sets are compared bit for bit.

There is no gate: the figures are recorded."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_range(xs):
	return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def host_compile(ids, n, L, doc_off, kw_a, kw_b, width_a, pulse, weights):
	"""the booster in numpy / scipy, as the reference computes it per document"""
	import scipy.ndimage

	def keyword_signal(kw, max_count):
		counts = np.isin(ids, kw).reshape(n, L).sum(axis=1)
		return np.minimum(counts, max_count).astype(np.float32) / max_count
	a, b = keyword_signal(kw_a, 2), keyword_signal(kw_b, 1)
	sa, sb = np.empty(n, np.float32), np.empty(n, np.float32)
	for lo, hi in zip(doc_off[:-1], doc_off[1:]):
		sa[lo:hi] = scipy.ndimage.maximum_filter(a[lo:hi], size=width_a)
		x = b[lo:hi]
		sb[lo:hi] = np.convolve(x, pulse, mode="same") if len(pulse) <= len(x) else x
	return np.average([np.ones(n, np.float32), sa, sb], axis=0, weights=weights).astype(np.float32)


def device_compile(core, c, doc_off, kw_a, kw_b, width_a, pulse, weights):
	c.signal_keywords(0, kw_a, max_count=2)
	c.signal_filter(0, core.VK_SIGNAL_FILTER_MAX, width_a, doc_off)
	c.signal_keywords(1, kw_b, max_count=1)
	c.signal_filter(1, core.VK_SIGNAL_FILTER_CONV, len(pulse), doc_off, pulse=pulse)
	return c.set_saliency([0, 1], weights)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--sentences", type=int, default=1000000)
	ap.add_argument("--len", type=int, default=32)
	ap.add_argument("--d", type=int, default=300)
	ap.add_argument("--vocab", type=int, default=50000)
	ap.add_argument("--keywords", type=int, default=20)
	ap.add_argument("--doc-sentences", type=int, default=1000)
	ap.add_argument("--len-t", type=int, default=10)
	ap.add_argument("--queries", type=int, default=30)
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--warmup", type=int, default=3)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	n, L, d, V = args.sentences, args.len, args.d, args.vocab

	from vectorian_amd import core, synth
	from vectorian_amd.saliency import gauss_envelope
	core.init(0)
	rng = np.random.default_rng(18)
	E = synth.make_vocab(V, d).astype(np.float32)
	ids = synth.zipf_ids(n * L, V, rng).astype(np.int32)
	off = np.arange(n + 1, dtype=np.int64) * L
	doc_off = np.unique(np.concatenate((np.arange(0, n, args.doc_sentences), [n]))).astype(np.int64)
	kw = rng.choice(np.arange(20, min(V, 2000)), size=args.keywords, replace=False).astype(np.int32)   # words of middling frequency
	kw_a, kw_b = kw[:len(kw) // 2], kw[len(kw) // 2:]
	width_a = 5
	pulse = gauss_envelope(np.linspace(-1, 1, 7))
	pulse = pulse / np.sum(pulse)
	strength = 0.5
	weights = np.array([1 - strength] + (np.array([1.0, 1.0]) / 2.0 * strength).tolist())
	result = dict(tool="tools/bench_saliency.py", sentences=n, tokens_per_sentence=L, d=d, vocab=V, layout="static", keywords=len(kw),
		documents=len(doc_off) - 1, signals=["keywords max_count=2, MaxFilter(5)", "keywords max_count=1, GaussFilter(7)"], strength=strength,
		cpus_visible=len(os.sched_getaffinity(0)), omp_num_threads=os.environ.get("OMP_NUM_THREADS"))

	c = core.Corpus(layout=core.VK_LAYOUT_STATIC, d=d, n_tokens=n * L, n_sentences=n, vocab_size=V)
	c.append_vectors(E, normalize=True)
	c.set_token_ids(ids)
	c.set_sentences(off)
	c.finalize()

	# ---- (a) compile
	device_s, host_s = [], []
	for i in range(args.warmup + args.repeats):
		t0 = time.perf_counter()
		boost = device_compile(core, c, doc_off, kw_a, kw_b, width_a, pulse, weights)
		if i >= args.warmup:
			device_s.append(time.perf_counter() - t0)
	for i in range(1 + min(args.repeats, 3)):
		t0 = time.perf_counter()
		want = host_compile(ids, n, L, doc_off, kw_a, kw_b, width_a, pulse, weights)
		if i >= 1:
			host_s.append(time.perf_counter() - t0)
	ulps = np.abs(boost.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
	result["compile"] = dict(device_s=median_range(device_s), host_numpy_scipy_s=median_range(host_s),
		host_over_device=statistics.median(host_s) / statistics.median(device_s), largest_difference_ulps=int(ulps.max()),
		slices_that_differ=int((ulps > 0).sum()), distinct_boosts=int(len(np.unique(boost))),
		note="device: five native calls from Python, each ending in a synchronise, the booster copied back once; host: numpy / scipy, one filter call per document")
	print(json.dumps(dict(compile=result["compile"])), flush=True)

	# ---- (b) the headline query, boost per query against the resident booster
	corpus = dict(E=E, tok_id=ids, sent_off=off)
	w = (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(np.float32)
	options = dict(locality=core.Locality.LOCAL, gap_s=("table", w), gap_t=("table", w), q_normalize=True, max_matches=10, min_score=0.0, want_flow=True)
	queries = synth.make_queries(corpus, args.queries, args.len_t)
	per_query = np.ascontiguousarray(boost, dtype=np.float32)   # as the index keeps it: no conversion per query

	def run(boost_arg):
		wall, prepare, total, tops = [], [], [], []
		for i in range(-args.warmup, len(queries)):
			q = queries[i % len(queries)]
			t0 = time.perf_counter()
			top = c.query(q["vectors"], q_token_ids=q["ids"], boost=boost_arg, **options)
			t1 = time.perf_counter()
			if i >= 0:
				t = c.last_timings()
				wall.append((t1 - t0) * 1e3)
				prepare.append(t["prepare_ms"])
				total.append(t["total_ms"])
				tops.append(top)
		return dict(wall_ms=median_range(wall), prepare_ms=median_range(prepare), device_total_ms=median_range(total)), tops

	by_array, tops_a = run(per_query)
	resident, tops_r = run(None)
	by_array_again, _ = run(per_query)   # the order of the two blocks does not make the difference
	same = all(a.n == r.n and np.array_equal(a.score[:a.n].view(np.uint32), r.score[:r.n].view(np.uint32)) and np.array_equal(a.sentence[:a.n], r.sentence[:r.n])
		and np.array_equal(a.mapping[:a.n], r.mapping[:r.n]) for a, r in zip(tops_a, tops_r))
	c.clear_saliency()
	unboosted, _ = run(None)
	result["query"] = dict(len_t=args.len_t, boost_per_query=by_array, resident_booster=resident, boost_per_query_again=by_array_again, no_boost=unboosted,
		results_equal_bit_for_bit=bool(same), boost_bytes_per_query=int(n * 4),
		wall_ms_saved_per_query=by_array["wall_ms"]["median"] - resident["wall_ms"]["median"],
		prepare_ms_saved_per_query=by_array["prepare_ms"]["median"] - resident["prepare_ms"]["median"])
	print(json.dumps(dict(query=result["query"])), flush=True)
	c.close()
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(json.dumps(result, indent=1) + "\n")
	print(json.dumps(result))


if __name__ == "__main__":
	main()
