"""A recording double for the saliency tests: tests/fake_backend.OracleCorpus with the signal methods of core.Corpus.  It notes every
call the index makes with its payload, keeps the signals on the host in saliency_cases' arithmetic, and -- as the library does -- runs
a query without a boost under the booster set_saliency left."""

import numpy as np

import saliency_cases as sc
from fake_backend import OracleCorpus
from vectorian_amd import core


class RecordingSaliencyCorpus(OracleCorpus):
	def __init__(self, **kw):
		super().__init__(**kw)
		self.calls = []
		self._signals = {}
		self.resident = None

	def finalize(self):
		self.calls.append(("finalize",))
		super().finalize()

	def _slices(self):
		if self._end is None:   # set_sentences: CSR offsets
			return self._off[:-1], self._off[1:]
		return self._off, self._end

	def signal_keywords(self, slot, keyword_ids, max_count=1, token_ids=None, vocab_size=None):
		self.calls.append(("signal_keywords", slot, np.array(keyword_ids), max_count, None if token_ids is None else np.array(token_ids), vocab_size))
		ids = self._ids if token_ids is None else token_ids
		start, end = self._slices()
		self._signals[slot] = sc.keyword_signal(ids, start[:self.n_sentences], end[:self.n_sentences], keyword_ids, max_count)

	def signal_set(self, slot, values):
		self.calls.append(("signal_set", slot, np.array(values)))
		self._signals[slot] = np.asarray(values, dtype=np.float32)

	def signal_filter(self, slot, kind, width, doc_off, pulse=None):
		self.calls.append(("signal_filter", slot, kind, width, np.array(doc_off), None if pulse is None else np.array(pulse)))
		f = (lambda x: sc.max_filter(x, width)) if kind == core.VK_SIGNAL_FILTER_MAX else (lambda x: sc.conv_filter(x, pulse))
		self._signals[slot] = sc.per_document(f, self._signals[slot], doc_off)

	def set_saliency(self, slots, weights):
		self.calls.append(("set_saliency", np.array(slots), np.array(weights)))
		self.resident = sc.average([self._signals[int(s)] for s in slots], weights, self.n_sentences)
		self._signals = {}
		return self.resident.copy()

	def query(self, q_vectors, **options):
		boost = options.get("boost")
		self.calls.append(("query", None if boost is None else np.array(boost)))
		if boost is None and self.resident is not None:
			options = dict(options, boost=self.resident)
		return super().query(q_vectors, **options)
