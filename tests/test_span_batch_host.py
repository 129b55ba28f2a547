"""CPU tier: the host side of the batched span pass.  The carve-up (vectorian_amd/csrc/vk_span_batch_host.h) is host-only:
a g++ driver with its own main (tests/span_batch_driver.cpp), built plain and with AddressSanitizer / UBSan and run as a stand-alone
program, walks a table of (tile_bytes, spans, queries) -- every width of test_gpu_span_batch.py, 1 .. 2^27 spans, 2 .. 5,000 queries
-- and the truth table of the qualification.  HipSpanEncoderIndex.find_many is held against a recording double of core.Corpus: how
it cuts a call into chunks, what it asks the backend, in which order the results come back."""

import os
import re
import subprocess

import numpy as np
import pytest

from fake_backend import OracleCorpus
from test_devbuf import CSRC, ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	exe = str(tmp_path_factory.mktemp("span_batch_" + request.param) / "span_batch_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (SANITIZE if request.param == "sanitized" else []) +
		["-I", CSRC, os.path.join(ROOT, "tests", "span_batch_driver.cpp"), "-o", exe], check=True)
	return lambda *args: subprocess.run([exe, *args], capture_output=True, text=True)


def test_every_shape_holds_its_invariants(driver):
	r = driver()
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0 and not [line for line in out if line.startswith("VIOLATED")], (out[:10], r.stderr[-2000:])
	points, table, violations = [int(x) for x in re.fullmatch(r"points (\d+) table (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and points == 14 * 11 * 11 and table == 25


def test_queries_per_lds_fill(driver):
	"""one workgroup per CU stages query tiles in the CU's 160 KiB: eight tiles of 304-d bf16 rows, six of 768-d, four of 1,024-d; two
	of 1,024-d fp32 rows -- never none up to 1,024 features"""
	fill = lambda tile_bytes: int(driver("fill", str(tile_bytes)).stdout)
	assert [fill(d * 32) for d in (16, 304, 384, 768, 1024)] == [128, 128, 128, 96, 64]
	assert [fill(d * 64) for d in (16, 304, 1024)] == [128, 128, 32]
	assert fill(160 * 1024) == 16 and fill(160 * 1024 + 512) == 0


def test_the_route_and_the_kernel_read_the_header():
	"""one place computes these numbers"""
	batch, kernel, internal = [open(os.path.join(CSRC, name)).read() for name in ("vk_batch.cpp", "vk_span_batch.hip", "vk_internal.h")]
	assert '#include "vk_span_batch_host.h"' in kernel and '#include "vk_span_batch_host.h"' in internal
	for name in ("span_batch_corpus_ok(", "span_batch_query_ok(", "span_batch_fill_tiles(", "span_batch_chunk("):
		assert "vk_host::" + name in batch, name
	assert "vk_host::span_batch_grid(" in kernel and "160 * 1024" not in kernel
	# VK_BS_COUNT has not grown: tests/test_gpu_batch_every_slice.py hands vk_batch_state a 16-element array
	names = re.search(r"enum vk_batch_state_index \{(.*?)VK_BS_COUNT", internal, re.S).group(1)
	assert len(re.findall(r"VK_BS_[A-Z0-9_]+", names)) == 16


class Recording(OracleCorpus):
	"""core.Corpus's interface on the oracle, with a log of the calls an index makes"""
	log = None

	def query(self, q_vectors, **options):
		if not getattr(self, "_in_batch", False):
			Recording.log.append(("query", 1, options))
		return super().query(q_vectors, **options)

	def query_batch(self, queries, token_ids=None, **options):
		Recording.log.append(("query_batch", len(queries), options))
		assert all(np.asarray(q).shape == (1, self.d) for q in queries)
		self._in_batch = True
		try:
			return super().query_batch(queries, token_ids=token_ids, **options)
		finally:
			self._in_batch = False


def test_find_many_cuts_a_call_into_chunks():
	from test_host_api import Document, Session
	from vectorian_amd import core
	from vectorian_amd.sim import EmbeddedSpanSim, SpanEmbedding
	rng = np.random.default_rng(15)
	n, d = 90, 24
	vectors = rng.standard_normal((n, d)).astype(np.float32)
	docs = [Document([[f"s{i}"] for i in range(30)]) for _ in range(3)]
	session = Session(docs, embeddings=[])
	texts = [f"text {i}" for i in range(600)]
	target = {t: int(rng.integers(0, n)) for t in texts}
	encodes = []

	def encode(ts):
		encodes.append(len(ts))
		return np.stack([vectors[target[t]] + 0.05 * np.random.default_rng(target[t]).standard_normal(d).astype(np.float32) for t in ts])

	Recording.log = []
	index = session.partition("sentence").index(EmbeddedSpanSim(SpanEmbedding("enc", d, encode)), vectors=vectors, corpus_factory=Recording)
	encodes.clear()
	done = []
	results = index.find_many(texts, n=3, min_score=0.1, batch=256, progress=done.append)
	assert encodes == [256, 256, 88]
	assert [(name, count) for name, count, _ in Recording.log] == [("query_batch", 256), ("query_batch", 256), ("query_batch", 88)]
	for _, _, options in Recording.log:   # find's own options
		assert options == dict(q_normalize=True, locality=core.Locality.LOCAL, gap_s=0.0, gap_t=0.0, max_matches=3, min_score=0.1, want_flow=False)
	assert done == [256 / 600, 512 / 600, 1.0]
	assert len(results) == 600
	for t, r in zip(texts, results):   # in order: every text finds the span its vector was drawn from
		assert 1 <= len(r) <= 3 and docs.index(r[0].prepared_doc) * 30 + r[0].slice_id == target[t], t
		assert r[0].level == "span" and all(m.score > 0.1 for m in r)
	# the default chunk is 256 texts; in_flight is accepted
	Recording.log, encodes[:] = [], []
	assert len(index.find_many(texts[:300], n=3, in_flight=7)) == 300
	assert encodes == [256, 44] and [count for _, count, _ in Recording.log] == [256, 44]
	# find still makes a single query call, and returns what find_many returned for that text
	Recording.log, encodes[:] = [], []
	one = index.find(texts[5], n=3, min_score=0.1)
	assert [(name, count) for name, count, _ in Recording.log] == [("query", 1)] and encodes == [1]
	key = lambda r: [(docs.index(m.prepared_doc), m.slice_id, m.score) for m in r]
	assert key(one) == key(results[5])
	assert index.find_many([], n=3) == []
	with pytest.raises(TypeError):
		index.find_many(texts[:2], abort=[0])
	index.close()
