#!/usr/bin/env python3
"""Timing of the other BASELINE.json configurations / algorithms on one MI355X (not the
driver's bench: that is bench.py).  Prints one JSON line per run.

  python tools/bench_configs.py --alg rwmd --sentences 1000000
  python tools/bench_configs.py --alg wrd --d 768 --min-len 8 --max-len 64 --sentences 500000
  python tools/bench_configs.py --alg align --gap exp5 --locality global --d 768 --min-len 8 --max-len 64
  python tools/bench_configs.py --span-batch 256 --d 768          the span index's shape: 256 one-vector queries per vk_query_batch
  python tools/bench_configs.py --contextual-chain --d 300        the headline shape under operator chains on the cosine
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
	ap.add_argument("--alg", choices=["align", "rwmd", "wrd"], default="align")
	ap.add_argument("--gap", choices=["exp5", "linear", "affine", "lintable", "convex"], default="exp5", help="lintable: the linear cost 0.1 k handed over as a table (not strictly subadditive); convex: 0.02 k^2 capped at 1 (superadditive at short gaps)")
	ap.add_argument("--locality", choices=["local", "global", "semiglobal"], default="local")
	ap.add_argument("--d", type=int, default=300)
	ap.add_argument("--len-t", type=int, default=10)
	ap.add_argument("--min-len", type=int, default=32)
	ap.add_argument("--max-len", type=int, default=32)
	ap.add_argument("--sentences", type=int, default=1000000)
	ap.add_argument("--steps", type=int, default=10)
	ap.add_argument("--warmup", type=int, default=2)
	ap.add_argument("--k", type=int, default=10)
	ap.add_argument("--layout", choices=["contextual", "static"], default="contextual")
	ap.add_argument("--batch", type=int, default=0, help="queries per vk_query_batch call (config 4: 256)")
	ap.add_argument("--batch-flows", action="store_true", help="with --batch: flows asked for, so that every query's winners are restated from their "
		"similarity rows on the host (batch_winner_rows) instead of written from the scores of the pass")
	ap.add_argument("--precision", choices=["bf16", "f32"], default="bf16", help="how the unit rows are kept in HBM")
	ap.add_argument("--handles", type=int, default=1, help="queries in flight (vk_corpus_view handles, one host thread each), as bench.py keeps them")
	ap.add_argument("--filter", type=float, default=0.0, help="share of tokens a pos_filter drops: times vk_corpus_filter, then queries the filtered corpus")
	ap.add_argument("--sim-ops", type=int, default=0, help="static layout: after the plain run, the same queries under a chain of this many operators "
		"on the cosine (vk_corpus_set_sim_ops; Bias / Scale in turn), reported beside it as phases_ms_mean_sim_ops")
	ap.add_argument("--sim-source", action="append", default=[], metavar="KIND[:ARG]", help="static layout, may be repeated: after the plain run, the same "
		"queries under this source (vk_corpus_set_sim_source) -- pnorm:P under Scale(s), DistanceToSimilarity with the median cell at one half, "
		"sqrt-cosine bare -- reported beside the cosine as sim_sources: prepare_ms and the whole query's wall time, each query's")
	ap.add_argument("--sim-mix", action="store_true", help="static layout: after the plain run, the same queries on a second, mixed handle "
		"(vk_corpus_set_sim_mix): a two-operand AVERAGE, weights 2 : 1, of the cosine over this vocabulary and the cosine over a second one of "
		"the same width -- reported beside the cosine as sim_mix: prepare_ms and the whole query's wall time, each query's")
	ap.add_argument("--span-batch", type=int, default=0, metavar="B", help="the span-embedding index's shape (one vector per slice, as --len-t 1 "
		"--min-len 1 --max-len 1 --gap linear): times query_batch of B one-vector queries with HipSpanEncoderIndex's options; prints pairs/s and the route")
	ap.add_argument("--span-sim", action="append", default=[], metavar="KIND[:ARG]", help="the span-embedding index's shape, may be repeated: after the "
		"plain cosine, the same one-vector queries under this span similarity (vk_corpus_set_span_sim) -- pnorm:P under Scale(s), "
		"DistanceToSimilarity with the median distance at one half, sqrt-cosine bare, cosine under Bias(1), Scale(0.5) -- reported beside the "
		"cosine as span_sims: score_ms (device events) and the whole query's wall time, each query's, and the bytes the scoring pass reads")
	ap.add_argument("--contextual-chain", action="store_true", help="contextual layout: the same queries on one handle under the plain cosine, under "
		"[Bias(0)] (the generic tile form with a trivial chain and no bound pass) and under the chains (a), (d) and (e) of tests/sim_ops_cases.py "
		"(vk_corpus_set_contextual_sim_ops), the forms alternating within the process -- reported as contextual_chain: per form the score "
		"kernel's time from device events (every query's, median, spread), the algorithmic bf16 bytes over it, the route's plan, and the "
		"chain's own cost: the difference to [Bias(0)], not to the cosine")
	args = ap.parse_args()
	if args.span_batch > 0 or args.span_sim:
		args.alg, args.layout, args.len_t, args.min_len, args.max_len = "align", "contextual", 1, 1, 1

	import torch
	from vectorian_amd import core, synth
	core.init(0)
	device = torch.device("cuda", 0)
	V = 50000
	E = synth.make_vocab(V, args.d)
	rng = np.random.default_rng(1)
	lens = rng.integers(args.min_len, args.max_len + 1, size=args.sentences) if args.max_len > args.min_len else np.full(args.sentences, args.min_len)
	off = np.zeros(args.sentences + 1, dtype=np.int64)
	np.cumsum(lens, out=off[1:])
	n_tok = int(off[-1])
	ids = synth.zipf_ids(n_tok, V, rng)
	if args.layout == "static":
		# the reference's static-embedding layout: token ids + vocabulary table, per-query [V x |q|] table
		corpus = core.Corpus(layout=core.VK_LAYOUT_STATIC, d=args.d, n_tokens=n_tok, n_sentences=args.sentences, vocab_size=V)
		sources = []
		for text in args.sim_source:
			kind, _, arg = text.partition(":")
			sources.append((text, {"pnorm": core.VK_SIMSRC_PNORM, "sqrt-cosine": core.VK_SIMSRC_SQRT_COSINE}[kind], float(arg or 0)))
		if sources:   # the handle keeps the unmodified rows from its first append on, then goes back to the cosine for the plain run
			corpus.set_sim_source(sources[0][1], sources[0][2])
		corpus.append_vectors(E, normalize=True)
		corpus.set_sim_source(core.VK_SIMSRC_COSINE)
		corpus.set_token_ids(ids)
		corpus.set_sentences(off)
		corpus.finalize()
		w = (1 - 2.0 ** (-np.arange(0, max(65, args.len_t + 1)) / 5)).astype(np.float32)
		gap = {"exp5": ("table", w), "linear": 0.1, "affine": ("affine", 0.2, 0.05)}[args.gap]
		loc = {"local": 0, "global": 1, "semiglobal": 2}[args.locality]
		alg = {"align": core.VK_ALG_ALIGN, "rwmd": core.VK_ALG_RWMD, "wrd": core.VK_ALG_WRD}[args.alg]
		qs = []
		for i in range(args.steps + args.warmup):
			s_ = int(rng.integers(0, args.sentences)); st_ = int(off[s_])
			qi = ids[st_:st_ + args.len_t] if i % 2 == 0 else rng.integers(0, V, size=args.len_t)
			if len(qi) < args.len_t:
				qi = np.concatenate([qi, rng.integers(0, V, size=args.len_t - len(qi))])
			qs.append((np.ascontiguousarray(E[qi], dtype=np.float32), np.asarray(qi, dtype=np.int32)))
		def timed():
			for i in range(args.warmup):
				corpus.query(qs[i][0], q_token_ids=qs[i][1], algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, max_matches=args.k, want_flow=args.alg == "align")
			torch.cuda.synchronize()
			ph = []
			t0 = time.perf_counter()
			for i in range(args.steps):
				q = qs[args.warmup + i]
				corpus.query(q[0], q_token_ids=q[1], algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, max_matches=args.k, want_flow=args.alg == "align")
				ph.append(corpus.last_timings())
			return ph, time.perf_counter() - t0
		ph, el = timed()
		ph_ops = None
		if args.sim_ops > 0:
			# ((cos + 1/2) * 1/2 + 1/2) * 1/2 ...: stays inside [0, 1], so the scoring pass sees cells like the plain ones
			corpus.set_sim_ops([(core.VK_SIMOP_BIAS, 0.5) if i % 2 == 0 else (core.VK_SIMOP_SCALE, 0.5) for i in range(args.sim_ops)])
			ph_ops, _ = timed()
			corpus.set_sim_ops([])
		by_source = {}
		if sources:
			def each():
				"""prepare_ms and wall time of every query after the warm-up"""
				out = []
				for i in range(args.warmup + args.steps):
					q = qs[i]
					torch.cuda.synchronize()
					t0 = time.perf_counter()
					corpus.query(q[0], q_token_ids=q[1], algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, max_matches=args.k, want_flow=args.alg == "align")
					ms = (time.perf_counter() - t0) * 1e3
					if i >= args.warmup:
						out.append((corpus.last_timings()["prepare_ms"], ms))
				return {"prepare_ms_each": [a for a, _ in out], "query_ms_each": [b for _, b in out]}
			by_source["cosine"] = each()
			sample = E[rng.integers(0, V, size=256)]
			for text, kind, arg in sources:
				corpus.set_sim_source(kind, arg)
				if kind == core.VK_SIMSRC_PNORM:
					dist = (np.abs(sample[:128, None] - sample[None, 128:]) ** arg).sum(-1) ** (1 / arg)
					corpus.set_sim_ops([(core.VK_SIMOP_SCALE, 1 / (2 * float(np.median(dist)))), (core.VK_SIMOP_ONE_MINUS, 0.0)])
				by_source[text] = each()
				corpus.set_sim_ops([])
			corpus.set_sim_source(core.VK_SIMSRC_COSINE)
		by_mix = {}
		if args.sim_mix:
			def each_on(handle, operands):
				"""prepare_ms and wall time of every query after the warm-up"""
				out = []
				for i in range(args.warmup + args.steps):
					q = qs[i]
					more = dict(q_operand_vectors=[np.ascontiguousarray(E2[q[1]], dtype=np.float32)]) if operands else {}
					torch.cuda.synchronize()
					t0 = time.perf_counter()
					handle.query(q[0], q_token_ids=q[1], algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, max_matches=args.k, want_flow=args.alg == "align", **more)
					ms = (time.perf_counter() - t0) * 1e3
					if i >= args.warmup:
						out.append((handle.last_timings()["prepare_ms"], ms))
				return {"prepare_ms_each": [a for a, _ in out], "query_ms_each": [b for _, b in out]}
			E2 = np.random.default_rng(2).standard_normal((V, args.d)).astype(np.float32)
			mixed = core.Corpus(layout=core.VK_LAYOUT_STATIC, d=args.d, n_tokens=n_tok, n_sentences=args.sentences, vocab_size=V)
			mixed.set_sim_mix(core.VK_SIMMIX_AVERAGE, 2, [2, 1])
			mixed.set_sim_operand(1, args.d)
			mixed.append_operand_vectors(1, E2, normalize=True)
			mixed.append_vectors(E, normalize=True)
			mixed.set_token_ids(ids)
			mixed.set_sentences(off)
			mixed.finalize()
			by_mix["cosine"] = each_on(corpus, False)
			by_mix["average of two cosines"] = each_on(mixed, True)
			by_mix["cosine again"] = each_on(corpus, False)
			mixed.close()
		score_ms = float(np.mean([p["score_ms"] for p in ph]))
		cells = float(n_tok) * args.len_t
		print(json.dumps({"layout": "static", "alg": args.alg, "gap": args.gap, "d": args.d, "len_t": args.len_t, "len_s": [args.min_len, args.max_len],
			"sentences": args.sentences, "pairs_per_s": args.sentences * args.steps / el, "ms_per_query": el / args.steps * 1e3,
			"score_kernel_ms": score_ms, "GCUPS": cells / (score_ms * 1e-3) / 1e9,
			"token_id_GBps": n_tok * 4 / (score_ms * 1e-3) / 1e9,
			"phases_ms_mean": {k: float(np.mean([p[k] for p in ph])) for k in ph[0]},
			**({"sim_ops": args.sim_ops, "phases_ms_mean_sim_ops": {k: float(np.mean([p[k] for p in ph_ops])) for k in ph_ops[0]},
				"prepare_ms_each": [p["prepare_ms"] for p in ph], "prepare_ms_each_sim_ops": [p["prepare_ms"] for p in ph_ops]} if ph_ops else {}),
			**({"sim_sources": by_source} if by_source else {}), **({"sim_mix": by_mix} if by_mix else {})}))
		corpus.close()
		return
	corpus = core.Corpus(layout=core.VK_LAYOUT_CONTEXTUAL, d=args.d, n_tokens=n_tok, n_sentences=args.sentences,
		keep_magnitudes=args.alg == "wrd", precision=args.precision)
	span_sims = []
	for text in args.span_sim:
		kind, _, arg = text.partition(":")
		span_sims.append((text, {"cosine": core.VK_SIMSRC_COSINE, "pnorm": core.VK_SIMSRC_PNORM, "sqrt-cosine": core.VK_SIMSRC_SQRT_COSINE}[kind], float(arg or 0)))
	if any(kind != core.VK_SIMSRC_COSINE for _, kind, _ in span_sims):
		# the handle keeps the unmodified rows from its first append on, then goes back to the cosine for the plain run
		corpus.set_span_sim(next((kind, arg) for _, kind, arg in span_sims if kind != core.VK_SIMSRC_COSINE), [])
	E_dev = torch.from_numpy(E).to(device)
	gen = torch.Generator(device=device)
	gen.manual_seed(7)
	chunk = 1 << 19
	for a in range(0, n_tok, chunk):
		b = min(a + chunk, n_tok)
		idx = torch.from_numpy(ids[a:b].astype(np.int64)).to(device)
		x = E_dev[idx] + 0.3 * torch.randn((b - a, args.d), device=device, generator=gen)
		if args.alg == "wrd":
			x = x * torch.exp(0.25 * torch.randn((b - a, 1), device=device, generator=gen))
		x = x.contiguous()
		torch.cuda.synchronize()
		corpus.append_vectors_device(x.data_ptr(), b - a, core.VK_F32, normalize=True)
		del x, idx
	corpus.set_sentences(off)
	corpus.finalize()
	if span_sims:
		corpus.set_span_sim(None, [])

	filter_ms = None
	n_tok_scored = n_tok
	if args.filter > 0.0:
		source = corpus
		drop = (rng.random(n_tok) < args.filter).astype(np.int8)
		source.set_token_pos(drop)
		n_tok_scored = int(n_tok - drop.sum())   # the kernel streams the tokens that pass the filter: the roofline counts those
		source.filtered(pos_mask=2).close()   # warm-up (first use of the scan)
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		corpus = source.filtered(pos_mask=2)
		filter_ms = (time.perf_counter() - t0) * 1e3

	w = (1 - 2.0 ** (-np.arange(0, max(65, args.len_t + 1)) / 5)).astype(np.float32)
	gap = {"exp5": ("table", w), "linear": 0.1, "affine": ("affine", 0.2, 0.05),
		"lintable": ("table", (0.1 * np.arange(0, 65)).astype(np.float32)),
		"convex": ("table", np.minimum(0.02 * np.arange(0, 65) ** 2, 1.0).astype(np.float32))}[args.gap]
	loc = {"local": 0, "global": 1, "semiglobal": 2}[args.locality]
	alg = {"align": core.VK_ALG_ALIGN, "rwmd": core.VK_ALG_RWMD, "wrd": core.VK_ALG_WRD}[args.alg]
	qs = []
	for i in range(args.steps + args.warmup):
		if i % 2 == 0:
			s = int(rng.integers(0, args.sentences))
			st = int(off[s])
			qi = ids[st:st + args.len_t]
			if len(qi) < args.len_t:
				qi = np.concatenate([qi, rng.integers(0, V, size=args.len_t - len(qi))])
		else:
			qi = rng.integers(0, V, size=args.len_t)
		qs.append(np.ascontiguousarray(E[qi] + 0.05 * rng.standard_normal((args.len_t, args.d)).astype(np.float32), dtype=np.float32))

	def step(q):
		return corpus.query(q, algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, q_normalize=True, max_matches=args.k,
			min_score=0.0 if loc != 1 else -1e9, want_flow=args.alg == "align")

	if args.contextual_chain:
		import ctypes
		B, S, O, P, R = core.VK_SIMOP_BIAS, core.VK_SIMOP_SCALE, core.VK_SIMOP_ONE_MINUS, core.VK_SIMOP_POWER, core.VK_SIMOP_RADIAL_BASIS
		forms = [("cosine", []), ("[Bias(0)]", [(B, 0.0)]), ("(a) (x + 1) / 2", [(B, 1.0), (S, 0.5)]),
			("(d) eight exactly rounded operators", [(B, 1.0), (S, 0.5), (B, -0.125), (S, 1.25), (O, 0.0), (O, 0.0), (B, 0.0625), (S, 0.9)]),
			("(e) powf", [(P, 2.5)])]
		core.lib().vk_query_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
		plans = ("LISTED", "SPAN", "FUSED", "BOUNDED", "MULTI_BLOCK", "DOCW_ALL", "DOCG_ALL", "WIDE_ALL")   # route_plan, vk_route_host.h
		runs = {name: {"score_ms_each": [], "query_ms_each": [], "plans": set()} for name, _ in forms}
		rounds = 3
		for rnd in range(rounds):   # the forms alternate: a drift of the device's clocks falls on all of them
			for name, ops in forms:
				corpus.set_contextual_sim_ops(ops)
				for i in range(args.warmup):
					step(qs[i])
				for i in range(args.steps):
					torch.cuda.synchronize()
					t0 = time.perf_counter()
					step(qs[args.warmup + i])
					runs[name]["query_ms_each"].append((time.perf_counter() - t0) * 1e3)
					runs[name]["score_ms_each"].append(corpus.last_timings()["score_ms"])
					state = np.zeros(16, dtype=np.int64)
					core._check(core.lib().vk_query_route(corpus._h, state.ctypes.data))
					runs[name]["plans"].add(plans[int(state[0])])
		corpus.set_contextual_sim_ops([])
		bytes_alg = n_tok * args.d * 2
		for r in runs.values():
			ms = np.array(r["score_ms_each"])
			r.update(plans=sorted(r["plans"]), score_ms_median=float(np.median(ms)), score_ms_min=float(ms.min()), score_ms_max=float(ms.max()),
				query_ms_median=float(np.median(r["query_ms_each"])), algorithmic_bf16_TB_per_s=bytes_alg / (float(np.median(ms)) * 1e-3) / 1e12)
		base = runs["[Bias(0)]"]["score_ms_median"]
		for name, r in runs.items():
			r["score_ms_over_bias0"] = r["score_ms_median"] - base   # the chain's own cost (the cosine: the price of the generic form and of the bound pass, negated)
		print(json.dumps({"contextual_chain": runs, "d": args.d, "precision": args.precision, "gap": args.gap, "locality": args.locality, "len_t": args.len_t,
			"len_s": [args.min_len, args.max_len], "sentences": args.sentences, "tokens": n_tok, "k": args.k, "steps_per_round": args.steps, "rounds": rounds,
			"algorithmic_bf16_bytes": bytes_alg, "note": "score_ms: the scoring pass between device events (under the cosine: the bound pass and its rounds)"}))
		corpus.close()
		return

	if span_sims:
		def each():
			"""score_ms and wall time of every query after the warm-up"""
			out = []
			for i in range(args.warmup + args.steps):
				torch.cuda.synchronize()
				t0 = time.perf_counter()
				top = corpus.query(qs[i], q_normalize=True, locality=0, gap_s=0.0, gap_t=0.0, max_matches=args.k, min_score=0.0, want_flow=False)
				ms = (time.perf_counter() - t0) * 1e3
				if i >= args.warmup:
					out.append((corpus.last_timings()["score_ms"], ms, top.n))
			return {"score_ms_each": [a for a, _, _ in out], "query_ms_each": [b for _, b, _ in out], "score_ms_median": float(np.median([a for a, _, _ in out])),
				"query_ms_median": float(np.median([b for _, b, _ in out])), "matches_min": int(min(n for _, _, n in out))}
		unit_bytes = args.sentences * ((args.d + 31) // 32 * 32) * (4 if args.precision == "f32" else 2)
		raw_bytes = args.sentences * ((args.d + 15) // 16 * 16) * 4
		by_sim = {"cosine (plain)": dict(each(), bytes_read=unit_bytes)}
		for text, kind, arg in span_sims:
			ops = []
			if kind == core.VK_SIMSRC_PNORM:
				sample = E[rng.integers(0, V, size=256)]
				dist = (np.abs(sample[:128, None] - sample[None, 128:]) ** arg).sum(-1) ** (1 / arg)
				ops = [(core.VK_SIMOP_SCALE, 1 / (2 * float(np.median(dist)))), (core.VK_SIMOP_ONE_MINUS, 0.0)]
			elif kind == core.VK_SIMSRC_COSINE:
				ops = [(core.VK_SIMOP_BIAS, 1.0), (core.VK_SIMOP_SCALE, 0.5)]
			corpus.set_span_sim(None if kind == core.VK_SIMSRC_COSINE else (kind, arg), ops)
			by_sim[text] = dict(each(), bytes_read=unit_bytes if kind == core.VK_SIMSRC_COSINE else raw_bytes)
		for r in by_sim.values():
			r["TB_per_s"] = r["bytes_read"] / (r["score_ms_median"] * 1e-3) / 1e12
		print(json.dumps({"span_sims": by_sim, "d": args.d, "precision": args.precision, "spans": args.sentences, "k": args.k, "steps": args.steps,
			"device_bytes": corpus.device_bytes}))
		corpus.close()
		return

	if args.span_batch > 0:
		import ctypes
		bq = [np.ascontiguousarray(E[rng.integers(0, V, size=1)] + 0.05 * rng.standard_normal((1, args.d)).astype(np.float32), dtype=np.float32)
			for _ in range(args.span_batch)]
		def sstep():
			return corpus.query_batch(bq, q_normalize=True, locality=0, gap_s=0.0, gap_t=0.0, max_matches=args.k, min_score=0.0, want_flow=False)
		for i in range(args.warmup):
			sstep()
		torch.cuda.synchronize()
		ph = []
		t0 = time.perf_counter()
		for i in range(args.steps):
			outs = sstep()
			ph.append(corpus.last_timings())
		el = time.perf_counter() - t0
		state = np.zeros(16, dtype=np.int64)   # vk_batch_state (internal export): entry 0 is the route -- 1 query by query, 2 the shared pass, 4 the span pass
		core.lib().vk_batch_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
		core._check(core.lib().vk_batch_state(corpus._h, state.ctypes.data))
		score_ms = float(np.mean([p["score_ms"] for p in ph]))
		print(json.dumps({
			"span_batch": args.span_batch, "d": args.d, "precision": args.precision, "spans": args.sentences, "k": args.k, "route": int(state[0]),
			"pairs_per_s": args.sentences * args.span_batch * args.steps / el, "ms_per_batch": el / args.steps * 1e3,
			"score_kernels_ms": score_ms, "select_ms": float(np.mean([p["topk_ms"] for p in ph])), "total_device_ms": float(np.mean([p["total_ms"] for p in ph])),
			"matrix_GB": args.sentences * args.span_batch * 4 / 1e9, "corpus_GB": args.sentences * args.d * (4 if args.precision == "f32" else 2) / 1e9,
			"top_score_q0": float(outs[0].score[0]) if outs[0].n else None}))
		corpus.close()
		return

	if args.batch > 0:
		# BASELINE config 4: a batch of queries per call
		bq = [np.ascontiguousarray(E[rng.integers(0, V, size=args.len_t)] + 0.05 * rng.standard_normal((args.len_t, args.d)).astype(np.float32), dtype=np.float32)
			for _ in range(args.batch)]
		for i in range(0, len(bq), 2):    # half of them planted
			s_ = int(rng.integers(0, args.sentences)); st_ = int(off[s_])
			qi = ids[st_:st_ + args.len_t]
			if len(qi) == args.len_t:
				bq[i] = np.ascontiguousarray(E[qi] + 0.05 * rng.standard_normal((args.len_t, args.d)).astype(np.float32), dtype=np.float32)
		def bstep():
			return corpus.query_batch(bq, algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, q_normalize=True, max_matches=args.k,
				min_score=0.0 if loc != 1 else -1e9, want_flow=args.batch_flows)
		for i in range(args.warmup):
			bstep()
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		ph = []
		for i in range(args.steps):
			outs = bstep()
			ph.append(corpus.last_timings())
		el = time.perf_counter() - t0
		score_ms = float(np.mean([p["score_ms"] for p in ph]))
		flops = 2.0 * n_tok * args.batch * args.len_t * args.d
		if args.min_len == 32 and args.max_len == 32:   # vk_rwmd_batch32_kernel: 3 (len_t <= 10) or 2 queries per 32-row tile, K padded to 16
			qpt = 3 if args.len_t <= 10 else 2
			flops_padded = 2.0 * n_tok * ((args.batch + qpt - 1) // qpt) * 32 * ((args.d + 15) // 16 * 16)
		elif args.max_len > args.min_len and args.d <= 320:   # ragged: sentences padded to 32 / 64 tokens on the 32x32x16 kernels, 16 queries per 5 tiles
			padded = float(np.sum((lens + 31) // 32 * 32))
			flops_padded = 2.0 * padded * ((args.batch + 15) // 16 * 5) * 32 * ((args.d + 15) // 16 * 16)
		else:
			padded = float(np.sum((lens + 15) // 16 * 16))
			flops_padded = 2.0 * padded * args.batch * 16 * ((args.d + 31) // 32 * 32)
		print(json.dumps({
			"alg": args.alg, "batch": args.batch, "flows": args.batch_flows, "d": args.d, "len_t": args.len_t, "len_s": [args.min_len, args.max_len],
			"sentences": args.sentences, "pairs_per_s": args.sentences * args.batch * args.steps / el,
			"ms_per_batch": el / args.steps * 1e3, "gemm_kernel_ms": score_ms,
			"algorithmic_TFLOPs": flops / (score_ms * 1e-3) / 1e12, "issued_mfma_TFLOPs": flops_padded / (score_ms * 1e-3) / 1e12,
			"frac_of_2.5PF_algorithmic": flops / (score_ms * 1e-3) / 2.5e15,
			"phases_ms_mean": {k: float(np.mean([p[k] for p in ph])) for k in ph[0]},
			"top_score_q0": float(outs[0].score[0]) if outs[0].n else None}))
		corpus.close()
		return

	for i in range(args.warmup):
		step(qs[i])
	torch.cuda.synchronize()
	phases = []
	if args.handles > 1:
		# several queries in flight: the selection / exact stage / traceback of one query beside the scoring kernel of the next
		from concurrent.futures import ThreadPoolExecutor
		handles = [corpus] + [corpus.view() for _ in range(args.handles - 1)]

		def run(h, q):
			r = h.query(q, algorithm=alg, locality=loc, gap_s=gap, gap_t=gap, q_normalize=True, max_matches=args.k,
				min_score=0.0 if loc != 1 else -1e9, want_flow=args.alg == "align")
			return r, h.last_timings()
		with ThreadPoolExecutor(max_workers=len(handles)) as pool:
			for h in handles:
				run(h, qs[0])          # one at a time first: a handle's kernel queues behind its peer's from the second query on
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			futs = []
			for i in range(args.steps):
				if len(futs) >= len(handles):
					top, ph = futs.pop(0).result()
					phases.append(ph)
				futs.append(pool.submit(run, handles[i % len(handles)], qs[args.warmup + i]))
			for f in futs:
				top, ph = f.result()
				phases.append(ph)
			el = time.perf_counter() - t0
		for h in handles[1:]:
			h.close()
	else:
		t0 = time.perf_counter()
		for i in range(args.steps):
			top = step(qs[args.warmup + i])
			phases.append(corpus.last_timings())
		el = time.perf_counter() - t0
	score_ms = float(np.mean([p["score_ms"] for p in phases]))
	bytes_alg = n_tok_scored * args.d * 2   # (round 2 counted the unfiltered tokens: "hbm_frac_of_8TBps: 1.044" with --filter)
	print(json.dumps({
		"alg": args.alg, "gap": args.gap, "locality": args.locality, "d": args.d, "len_t": args.len_t,
		"len_s": [args.min_len, args.max_len], "sentences": args.sentences, "tokens": n_tok, "tokens_scored": n_tok_scored,
		"pairs_per_s": args.sentences * args.steps / el, "ms_per_query": el / args.steps * 1e3,
		"score_kernel_ms": score_ms, "score_kernel_GBps": bytes_alg / (score_ms * 1e-3) / 1e9,
		"hbm_frac_of_8TBps": bytes_alg / (score_ms * 1e-3) / 8e12,
		"phases_ms_mean": {k: float(np.mean([p[k] for p in phases])) for k in phases[0]},
		"top_score": float(top.score[0]) if top.n else None, "filter_build_ms": filter_ms, "handles": args.handles}))
	corpus.close()


if __name__ == "__main__":
	main()
