#!/usr/bin/env python3
"""Index build of a span corpus from pooled token vectors: `--sentences` sentences of `--len` tokens at `--d` features,
mean pooling, over a static embedding (a vocabulary of `--vocab` rows and token ids: one vk_corpus_append_pooled) and over a
contextual one (documents of `--doc-sentences` sentences: one call per document), each beside the host route -- the reference's
loop, one numpy call per span, then the vectors appended as rows -- timed in the same process.

  hipcc --offload-arch=gfx950 -O3 -o tools/probe/read_bw tools/probe/read_bw.hip      (optional: the read-only ceiling beside it)
  python tools/bench_pooled_spans.py --out profiles/pooled_spans.json

Every build is a host clock around work that ends in a synchronise (every native call drains the handle's stream); the kernel alone
is timed with device events around vk_launch_pool_spans on rows that are resident, apart from the copies.  Medians of `--repeats`
runs after `--warmup`.  There is no gate: the figures are recorded."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_range(xs):
	return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=len(xs))


def read_bw_probe(gb):
	"""tools/probe/read_bw in a process of its own: TB/s of read-only kernels, per pattern"""
	exe = os.path.join(ROOT, "tools", "probe", "read_bw")
	if not os.path.exists(exe):
		return dict(note="tools/probe/read_bw is not built: not measured")
	p = subprocess.run([exe, str(gb), "1"], capture_output=True, text=True, timeout=300)
	if p.returncode != 0:
		return dict(note=f"tools/probe/read_bw exited with {p.returncode}: not measured")
	rates = json.loads(p.stdout.strip().splitlines()[-1])["TBps"]
	# a wave owns a contiguous run and keeps 4 / 8 loads of 1 KiB in flight: the pooling kernel's pattern over rows as they are
	keep = {k: v for k, v in rates.items() if k.startswith(("runs_u4_nt", "runs_u8_nt", "runs_u8_w", "stride_u4_w"))}
	return dict(GB=gb, TBps=keep, best_TBps=max(rates.values()))


def finish(c, n):
	c.set_sentences(np.arange(n + 1, dtype=np.int64))
	c.finalize()


def span_corpus(core, d, n):
	return core.Corpus(layout=core.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n)


def kernel_ms(core, torch, rows, ids, start, end, d, repeats, warmup):
	"""vk_launch_pool_spans alone, on resident arrays, between device events"""
	lib = core.lib()
	fn = lib.vk_launch_pool_spans
	fn.restype = C.c_int
	fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
	n = start.shape[0]
	out = torch.empty((n, d), dtype=torch.float32, device=rows.device)
	times = []
	for i in range(warmup + repeats):
		a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		a.record()
		rc = fn(rows.data_ptr(), 0, None if ids is None else ids.data_ptr(), start.data_ptr(), end.data_ptr(), n, d, core.VK_POOL_MEAN, out.data_ptr(), None)
		b.record()
		torch.cuda.synchronize()
		if rc != 0:
			raise RuntimeError(f"vk_launch_pool_spans: hipError {rc}")
		if i >= warmup:
			times.append(a.elapsed_time(b))
	return times, out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--sentences", type=int, default=1000000)
	ap.add_argument("--len", type=int, default=32)
	ap.add_argument("--d", type=int, default=300)
	ap.add_argument("--vocab", type=int, default=50000)
	ap.add_argument("--doc-sentences", type=int, default=1000)
	ap.add_argument("--repeats", type=int, default=5)
	ap.add_argument("--warmup", type=int, default=1)
	ap.add_argument("--host-repeats", type=int, default=1, help="the host route takes seconds per run")
	ap.add_argument("--read-bw-gb", type=float, default=19.2)
	ap.add_argument("--out", default=None)
	args = ap.parse_args()
	n, L, d, V = args.sentences, args.len, args.d, args.vocab
	result = dict(tool="tools/bench_pooled_spans.py", sentences=n, tokens_per_sentence=L, d=d, vocab=V, agg="mean", cpus_visible=len(os.sched_getaffinity(0)), omp_num_threads=os.environ.get("OMP_NUM_THREADS"),
		host_route="one numpy call per span in one Python process (the reference's loop), then append_vectors")
	result["read_bw_probe"] = read_bw_probe(args.read_bw_gb)

	import torch
	from vectorian_amd import core, synth
	core.init(0)
	dev = torch.device("cuda", 0)
	rng = np.random.default_rng(16)
	start = np.arange(n, dtype=np.int64) * L
	end = start + L
	check = rng.choice(n, size=min(n, 2000), replace=False)

	# ---- static: the vocabulary and the token ids
	E = synth.make_vocab(V, d).astype(np.float32)
	ids = synth.zipf_ids(n * L, V, rng).astype(np.int32)
	device_s, pool_s = [], []
	for i in range(args.warmup + args.repeats):
		t0 = time.perf_counter()
		c = span_corpus(core, d, n)
		t1 = time.perf_counter()
		c.append_pooled(E, start, end, np.mean, ids=ids, normalize=True)
		t2 = time.perf_counter()
		finish(c, n)
		t3 = time.perf_counter()
		c.close()
		if i >= args.warmup:
			device_s.append(t3 - t0)
			pool_s.append(t2 - t1)
	host_s, loop_s = [], []
	for _ in range(args.host_repeats):
		t0 = time.perf_counter()
		vectors = np.empty((n, d), np.float32)
		for s in range(n):
			vectors[s] = np.mean(E[ids[s * L:(s + 1) * L]], axis=0)
		t1 = time.perf_counter()
		c = span_corpus(core, d, n)
		c.append_vectors(vectors, normalize=True)
		finish(c, n)
		t2 = time.perf_counter()
		c.close()
		host_s.append(t2 - t0)
		loop_s.append(t1 - t0)
	with span_corpus(core, d, len(check)) as c:   # the same aggregates, bit for bit
		got = c.append_pooled(E, start[check], end[check], np.mean, ids=ids, want_pooled=True)
	same = bool(np.array_equal(got.view(np.uint32), vectors[check].view(np.uint32)))
	t_ids, t_start, t_end = (torch.from_numpy(a).to(dev) for a in (ids, start, end))
	times, _ = kernel_ms(core, torch, torch.from_numpy(E).to(dev), t_ids, t_start, t_end, d, max(10, args.repeats), 3)
	bytes_read = n * L * (d * 4 + 4) + n * 16
	bytes_written = n * d * 4
	k = median_range(times)
	result["static"] = dict(
		device_build_s=median_range(device_s), append_pooled_s=median_range(pool_s), host_build_s=median_range(host_s), host_loop_s=median_range(loop_s),
		host_over_device=statistics.median(host_s) / statistics.median(device_s), aggregates_equal_bit_for_bit=same,
		kernel_ms=k, kernel_bytes=dict(rows_and_ids_read=bytes_read, written=bytes_written, vocabulary=V * d * 4),
		kernel_effective_TBps=(bytes_read + bytes_written) / (k["median"] * 1e-3) / 1e12,
		note="the gathered rows come from a vocabulary of %.0f MB that stays in L2 / Infinity Cache: the effective rate is not an HBM rate" % (V * d * 4 / 1e6))
	print(json.dumps(dict(static=result["static"])), flush=True)
	del vectors, t_ids

	# ---- contextual: token vectors, document by document (a few distinct documents, taken in turn)
	per = args.doc_sentences
	n_docs = (n + per - 1) // per
	docs = [rng.standard_normal((per * L, d)).astype(np.float32) for _ in range(min(8, n_docs))]
	d_start = np.arange(per, dtype=np.int64) * L
	d_end = d_start + L
	sizes = [min(per, n - i * per) for i in range(n_docs)]
	device_s = []
	for i in range(args.warmup + min(args.repeats, 3)):
		t0 = time.perf_counter()
		c = span_corpus(core, d, n)
		for j, m in enumerate(sizes):
			c.append_pooled(docs[j % len(docs)][:m * L], d_start[:m], d_end[:m], np.mean, normalize=True)
		finish(c, n)
		t1 = time.perf_counter()
		c.close()
		if i >= args.warmup:
			device_s.append(t1 - t0)
	# the same calls over rows that are resident already (mem = device): what a call costs without the copy of its rows
	resident = [torch.from_numpy(x).to(dev) for x in docs]
	torch.cuda.synchronize()
	resident_s = []
	for i in range(args.warmup + min(args.repeats, 3)):
		t0 = time.perf_counter()
		c = span_corpus(core, d, n)
		for j, m in enumerate(sizes):
			c.append_pooled_device(resident[j % len(docs)].data_ptr(), m * L, core.VK_F32, d_start[:m], d_end[:m], np.mean, normalize=True)
		finish(c, n)
		t1 = time.perf_counter()
		c.close()
		if i >= args.warmup:
			resident_s.append(t1 - t0)
	del resident
	host_s, loop_s = [], []
	for _ in range(args.host_repeats):
		t0 = time.perf_counter()
		vectors = np.empty((n, d), np.float32)
		at = 0
		for j, m in enumerate(sizes):
			X = docs[j % len(docs)]
			for s in range(m):
				vectors[at + s] = np.mean(X[s * L:(s + 1) * L], axis=0)
			at += m
		t1 = time.perf_counter()
		c = span_corpus(core, d, n)
		c.append_vectors(vectors, normalize=True)
		finish(c, n)
		t2 = time.perf_counter()
		c.close()
		host_s.append(t2 - t0)
		loop_s.append(t1 - t0)
	with span_corpus(core, d, per) as c:
		got = c.append_pooled(docs[0], d_start, d_end, np.mean, want_pooled=True)
	same = bool(np.array_equal(got.view(np.uint32), vectors[:per].view(np.uint32)))
	del vectors
	# the copy of one document's rows alone through torch, for comparison (append_pooled copies from pageable memory with hipMemcpyAsync)
	copy_s = []
	for i in range(2 + 5):
		t0 = time.perf_counter()
		x = torch.from_numpy(docs[i % len(docs)]).to(dev)
		torch.cuda.synchronize()
		if i >= 2:
			copy_s.append(time.perf_counter() - t0)
		del x
	doc_bytes = per * L * d * 4
	h2d_GBps = doc_bytes / statistics.median(copy_s) / 1e9
	# the kernel over all the rows, resident (n x L x d fp32)
	X = torch.empty((n * L, d), dtype=torch.float32, device=dev)
	for a in range(0, n * L, 1 << 22):
		X[a:a + (1 << 22)].normal_()
	times, _ = kernel_ms(core, torch, X, None, t_start, t_end, d, max(10, args.repeats), 3)
	del X
	bytes_read = n * L * d * 4 + n * 16
	k = median_range(times)
	total_bytes = n * L * d * 4
	result["contextual"] = dict(
		documents=n_docs, sentences_per_document=per, device_build_s=median_range(device_s), device_build_rows_resident_s=median_range(resident_s),
		host_build_s=median_range(host_s), host_loop_s=median_range(loop_s),
		host_over_device=statistics.median(host_s) / statistics.median(device_s), aggregates_equal_bit_for_bit=same,
		rows_copy_share_of_device_build=1.0 - statistics.median(resident_s) / statistics.median(device_s),
		h2d_copy=dict(bytes_per_document=doc_bytes, GBps=h2d_GBps, seconds_for_all_rows=total_bytes / (h2d_GBps * 1e9)),
		kernel_ms=k, kernel_bytes=dict(rows_read=bytes_read, written=bytes_written),
		kernel_effective_TBps=(bytes_read + bytes_written) / (k["median"] * 1e-3) / 1e12)
	print(json.dumps(dict(contextual=result["contextual"])), flush=True)
	line = json.dumps(result)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(json.dumps(result, indent=1) + "\n")
	print(line)


if __name__ == "__main__":
	main()
