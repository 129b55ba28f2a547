"""The reference's saliency arithmetic (vectorian/saliency.py; Document::count_keywords, core/cpp/document.h:276-315) restated with
numpy and scipy, and the cases the host tier (test_saliency_host.py) and the GPU tier (test_gpu_saliency.py) share.  scipy is needed
here, by the tests only: the package restates what it needs of it in numpy."""

import numpy as np
import scipy.ndimage
import scipy.signal

MAX_WIDTHS = (1, 2, 3, 4, 5, 8)
PULSE_TAPS = tuple(range(1, 10))


# ---- the restatement

def keyword_signal(ids, start, end, keyword_ids, max_count):
	"""_FastKeywordSignal: count_keywords per slice, np.minimum(counts, max_count).astype(float32) / max_count.  A keyword id < 0 (a
	keyword outside the vocabulary) is dropped as count_keywords drops it; a token id < 0 is in no set"""
	kw = np.asarray([k for k in keyword_ids if k >= 0], dtype=np.int64)
	hit = np.isin(np.asarray(ids, dtype=np.int64), kw)
	counts = np.array([int(hit[a:b].sum()) for a, b in zip(start, end)], dtype=np.int64)
	counts = np.minimum(counts, max_count)
	return counts.astype(np.float32) / max_count


def max_filter(x, width):
	return scipy.ndimage.maximum_filter(x, size=width)


def normalized(pulse):
	pulse = np.asarray(pulse, dtype=np.float64)
	return pulse / np.sum(pulse)


def conv_filter(x, pulse):
	"""ConvFilter.__call__ with the pulse already divided by its sum"""
	if pulse.shape[0] <= x.shape[0]:
		return np.convolve(x, pulse, mode="same")
	return x


def gauss_pulse(width, fc=1):
	t = np.linspace(-1, 1, width, endpoint=True)
	_, e = scipy.signal.gausspulse(t, fc=fc, retenv=True)
	return e


def per_document(f, x, doc_off):
	"""a filter over every document's segment of a signal; each result as float32, as Saliency.add_signal's astype leaves it"""
	out = np.empty(len(x), dtype=np.float32)
	for a, b in zip(doc_off[:-1], doc_off[1:]):
		out[a:b] = np.asarray(f(x[a:b])).astype(np.float32)
	return out


def saliency_weights(user_weights, strength):
	if len(user_weights) == 0:
		return [1]
	normal_w = np.array(user_weights) / np.sum(user_weights)
	return [1 - strength] + (normal_w * strength).tolist()


def average(signals, weights, n):
	"""Saliency.compile: np.average over [ones, s_1 ..] in float64; Booster holds floats"""
	stack = [np.ones((n,), dtype=np.float32)] + [np.asarray(s, dtype=np.float32) for s in signals]
	return np.average(stack, axis=0, weights=weights).astype(np.float32)


def ulps(a, b):
	"""distance of two float32 arrays of finite values of one sign, in units of the last place"""
	a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
	return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the cases

def doc_lengths(width):
	"""documents of 1, 2, width - 1, width and width + 1 slices, one without slices in between, and a long one"""
	return [1, 2, max(width - 1, 1), 0, width, width + 1, 37]


def offsets(lengths):
	return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def signal_values(n, seed):
	"""a signal as keyword counts leave it -- multiples of 1 / 3 in [0, 1], many of them 0 -- with a few arbitrary values between"""
	rng = np.random.default_rng(seed)
	x = (np.minimum(rng.integers(0, 6, n), 3).astype(np.float32) / 3) * (rng.random(n) < 0.6)
	odd = rng.random(n) < 0.2
	x[odd] = rng.random(int(odd.sum())).astype(np.float32)
	return x.astype(np.float32)


def pulse_of(taps, seed=0):
	rng = np.random.default_rng(100 + taps + seed)
	return normalized(rng.random(taps) + 0.05)


def filter_cases(total=None):
	"""(name, kind, width, pulse or None, doc_off, x, expected): every filter case of the issue -- the max filter for widths 1, 2, 3,
	4, 5, 8 and the `same` convolution for pulses of 1 .. 9 taps (and two Gauss pulses), each over documents shorter than, as long as
	and longer than the window.  kind: 0 max, 1 convolution (VK_SIGNAL_FILTER_*).  total: every case over this many slices -- one more
	document takes the rest -- for a handle of that size"""
	def lengths(width):
		ls = doc_lengths(width)
		return ls if total is None else ls + [total - sum(ls)]
	cases = []
	for w in MAX_WIDTHS:
		off = offsets(lengths(w))
		x = signal_values(int(off[-1]), w)
		cases.append((f"max{w}", 0, w, None, off, x, per_document(lambda seg: max_filter(seg, w), x, off)))
	pulses = [(f"conv{m}", pulse_of(m)) for m in PULSE_TAPS] + [(f"gauss{m}", normalized(gauss_pulse(m))) for m in (4, 7)]
	for name, pulse in pulses:
		off = offsets(lengths(len(pulse)))
		x = signal_values(int(off[-1]), 50 + len(pulse))
		cases.append((name, 1, len(pulse), pulse, off, x, per_document(lambda seg: conv_filter(seg, pulse), x, off)))
	return cases


def assert_filtered(got, case):
	"""the max filter == scipy's; the convolution within one float32 ulp of np.convolve's rounded result (numpy does not specify the
	order of its sum), and == x where a document is shorter than the pulse"""
	name, kind, width, pulse, off, x, want = case
	got = np.asarray(got, dtype=np.float32)
	assert got.shape == want.shape, name
	if kind == 0:
		assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, got, want)
		return
	assert int(ulps(got, want).max(initial=0)) <= 1, (name, got, want)
	for a, b in zip(off[:-1], off[1:]):
		if b - a < width:
			assert np.array_equal(got[a:b].view(np.uint32), x[a:b].view(np.uint32)), (name, "pass-through", a, b)
