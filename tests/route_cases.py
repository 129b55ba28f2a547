"""The named single-query cases of the routing tests: five tiny corpora and one query per route of vk_query.  Shared by
tools/route_cases.py (parent against branch: kernel trace and result sets), tests/test_gpu_query_route.py (the route of each case from
vk_query_route, the result set against the oracle) and tests/test_route_host.py (the same routes from vk_host::route_query, CPU tier).

ROUTES was written from the kernel trace of the commit BEFORE vk_route_host.h existed (profiles/route_cases_trace_parent.txt): which
kernels served each case there is what the route has to say."""

import numpy as np

from vectorian_amd import synth

AFF = ("affine", 0.2, 0.05)
AFF_NEG = ("affine", -0.05, 0.1)   # a_t < 0: the prefix-scan form of the multi-block kernel does not take it
LIN = 0.1


def exp5(n):
	"""1 - 2^(-k/5): 1.0 in float32 from k = 125 on (ws_tail 125 over a corpus whose longest slice has more than 125 tokens)"""
	return ("table", (1 - 2.0 ** (-np.arange(0, n + 1) / 5)).astype(np.float32))


def rising(n):
	"""a table that never saturates (ws_tail 0)"""
	return ("table", (0.002 * np.arange(0, n + 1)).astype(np.float32))


# slices per corpus: A 40 of 3 .. 64 tokens; B: A and six of 65 .. 200; C: B and one of 600; D: one token each; E: B, static layout
def lengths(name):
	rng = np.random.default_rng(7)
	lens = rng.integers(3, 65, size=40)
	lens[5], lens[11] = 64, 3
	if name == "D":
		return np.ones(48, dtype=np.int64)
	if name in ("B", "C", "E"):
		lens = np.concatenate((lens, [65, 200, 129, 97, 160, 128]))
		lens = lens[np.random.default_rng(8).permutation(len(lens))]
	if name == "C":
		lens = np.insert(lens, 20, 600)
	return lens.astype(np.int64)


def build(hip, name, d):
	"""-> dict(c=handle, off, X (float rows or None), Xb (stored rows), static fields)"""
	lens = lengths(name)
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	rng = np.random.default_rng(100 + d + ord(name))
	n_tok = int(off[-1])
	pos_s = rng.integers(0, 6, size=n_tok).astype(np.int8)
	if name == "E":
		E = rng.standard_normal((500, d)).astype(np.float32)
		Eb = synth.to_bf16_bits(synth.normalize_rows(E))
		tok = rng.integers(0, 500, size=n_tok).astype(np.int32)
		c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=n_tok, n_sentences=len(lens), vocab_size=500)
		c.append_vectors(Eb, normalize=False)
		c.set_token_ids(tok)
		c.set_token_pos(pos_s)
		c.set_sentences(off)
		c.finalize()
		return dict(c=c, off=off, Eb=Eb, tok=tok, pos_s=pos_s, static=True, d=d)
	X = rng.standard_normal((n_tok, d)).astype(np.float32)
	Xb = synth.to_bf16_bits(synth.normalize_rows(X))
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n_tok, n_sentences=len(lens), keep_magnitudes=True)
	c.append_vectors(Xb, normalize=False)
	c.set_token_pos(pos_s)
	c.set_sentences(off)
	c.finalize()
	return dict(c=c, off=off, X=X, Xb=Xb, pos_s=pos_s, static=False, d=d)


def query_of(w, sent, len_t, seed):
	"""noisy copies of tokens of one slice (static layout: its token ids), random tokens behind them where the slice is shorter"""
	rng = np.random.default_rng(seed)
	a, b = int(w["off"][sent]), int(w["off"][sent + 1])
	idx = np.sort(rng.choice(np.arange(a, b), size=min(len_t, b - a), replace=False))
	if w["static"]:
		ids = w["tok"][idx].astype(np.int32)
		if len(ids) < len_t:
			ids = np.concatenate((ids, rng.integers(0, 500, size=len_t - len(ids)).astype(np.int32)))
		return w["Eb"][ids], ids
	q = w["X"][idx] + 0.05 * rng.standard_normal((len(idx), w["d"])).astype(np.float32)
	if len(q) < len_t:
		q = np.concatenate((q, rng.standard_normal((len_t - len(q), w["d"])).astype(np.float32)))
	return synth.to_bf16_bits(synth.normalize_rows(q)), None


ALIGN, RWMD, WRD = 0, 1, 2   # vk_algorithm
R11, R1N = (True, True, True), (False, False, True)   # relaxed WMD: (injective, symmetric, normalize_bow)

# name -> (corpus, d, len_t, options of Corpus.query / oracle.find, environment switches)
CASES = {
	"A64_linear_8": ("A", 64, 8, dict(gap=(LIN, LIN)), {}),
	"A64_affine_8": ("A", 64, 8, dict(gap=(AFF, AFF), locality=2), {}),
	"A64_table_8": ("A", 64, 8, dict(gap=("exp5", "exp5"), locality=1), {}),
	"A300_linear_8": ("A", 300, 8, dict(gap=(LIN, LIN)), {}),
	"A300_table_16": ("A", 300, 16, dict(gap=("exp5", "exp5")), {}),
	"A64_linear_20": ("A", 64, 20, dict(gap=(LIN, LIN)), {}),
	"A64_linear_40": ("A", 64, 40, dict(gap=(LIN, LIN), locality=1), {}),
	"A64_table_20": ("A", 64, 20, dict(gap=("exp5", "exp5")), {}),
	"A300_table_33": ("A", 300, 33, dict(gap=("exp5", "exp5")), {}),
	"A64_affine_neg_20": ("A", 64, 20, dict(gap=(AFF, AFF_NEG)), {}),
	"A64_linear_20_no_score32": ("A", 64, 20, dict(gap=(LIN, LIN)), {"VK_NO_SCORE32": "1"}),
	"A64_submatch_8": ("A", 64, 8, dict(gap=(LIN, LIN), submatch_weight=0.5), {}),
	"A64_tagged_8": ("A", 64, 8, dict(gap=(LIN, LIN), tagged=True), {}),
	"A64_rwmd11_8": ("A", 64, 8, dict(algorithm=RWMD, rwmd=R11), {}),
	"A64_rwmd1n_8": ("A", 64, 8, dict(algorithm=RWMD, rwmd=R1N), {}),
	"A64_rwmd1n_20": ("A", 64, 20, dict(algorithm=RWMD, rwmd=R1N), {}),
	"A64_wmd_8": ("A", 64, 8, dict(algorithm=RWMD, rwmd=R1N, wmd_full=True), {}),
	"A64_wrd_20": ("A", 64, 20, dict(algorithm=WRD), {}),
	"B64_linear_8": ("B", 64, 8, dict(gap=(LIN, LIN)), {}),
	"B64_linear_8_long_pass": ("B", 64, 8, dict(gap=(LIN, LIN)), {"VK_LONG_PASS": "1"}),
	"B64_exp5_8": ("B", 64, 8, dict(gap=("exp5", "exp5")), {}),
	"B64_rising_8": ("B", 64, 8, dict(gap=("rising", "rising")), {}),
	"B64_linear_20": ("B", 64, 20, dict(gap=(LIN, LIN)), {}),
	"B300_exp5_20": ("B", 300, 20, dict(gap=("exp5", "exp5")), {}),
	"B64_rising_20": ("B", 64, 20, dict(gap=("rising", "rising")), {}),
	"B64_linear_20_no_apart": ("B", 64, 20, dict(gap=(LIN, LIN)), {"VK_NO_APART": "1"}),
	"B64_rwmd11_8": ("B", 64, 8, dict(algorithm=RWMD, rwmd=R11), {}),
	"B64_rwmd11_20": ("B", 64, 20, dict(algorithm=RWMD, rwmd=R11), {}),
	"B64_rwmd1n_8": ("B", 64, 8, dict(algorithm=RWMD, rwmd=R1N), {}),
	"B64_rwmd1n_20": ("B", 64, 20, dict(algorithm=RWMD, rwmd=R1N), {}),
	"B64_wrd_20": ("B", 64, 20, dict(algorithm=WRD), {}),
	"B64_only_8": ("B", 64, 8, dict(gap=(LIN, LIN), only=(3, 41, 17)), {}),
	"C64_linear_8": ("C", 64, 8, dict(gap=(LIN, LIN)), {}),
	"C64_exp5_40": ("C", 64, 40, dict(gap=("exp5", "exp5")), {}),
	"C64_linear_20": ("C", 64, 20, dict(gap=(AFF, LIN)), {}),
	"C64_rwmd11_8": ("C", 64, 8, dict(algorithm=RWMD, rwmd=R11), {}),
	"D64_span_1": ("D", 64, 1, dict(gap=(LIN, LIN)), {}),
	"E64_linear_8": ("E", 64, 8, dict(gap=(LIN, LIN)), {}),
	"E64_rwmd1n_20": ("E", 64, 20, dict(algorithm=RWMD, rwmd=R1N), {}),
}

SWITCHES = sorted({k for case in CASES.values() for k in case[4]})


def options(w, name):
	"""-> (query rows, keyword arguments common to Corpus.query and oracle.find, those of Corpus.query alone, of oracle.find alone)"""
	corpus, d, len_t, opt, env = CASES[name]
	seed = sorted(CASES).index(name)
	n = len(w["off"]) - 1
	Qb, ids = query_of(w, (7 * seed + 3) % n, len_t, 500 + seed)
	longest = int(np.diff(w["off"]).max())
	table = {"exp5": exp5(max(512, longest)), "rising": rising(max(512, longest))}
	both = dict(max_matches=6, min_score=-1e9 if opt.get("locality", 0) else 0.0, locality=opt.get("locality", 0))
	if "gap" in opt:
		both["gap_s"], both["gap_t"] = [table.get(g, g) if isinstance(g, str) else g for g in opt["gap"]]
	for k in ("algorithm", "rwmd", "wmd_full", "submatch_weight"):
		if k in opt:
			both[k] = opt[k]
	if both.get("algorithm", ALIGN) != ALIGN:
		both["min_score"] = -1.0
	hip_kw, ref_kw = dict(q_normalize=False), {}
	if ids is not None:
		hip_kw["q_token_ids"], ref_kw["q_ids"] = ids, ids
	if opt.get("tagged"):
		rng = np.random.default_rng(900 + seed)
		both.update(tag_weights=rng.uniform(0.3, 1.0, size=len_t).astype(np.float32), q_pos=rng.integers(0, 6, size=len_t).astype(np.int8),
			pos_mismatch_penalty=0.4, similarity_threshold=0.15)
		ref_kw["pos_s"] = w["pos_s"]
	if "only" in opt:
		hip_kw["only_slices"] = np.asarray(opt["only"], dtype=np.int64)
	return Qb, both, hip_kw, ref_kw


def run(w, name, setenv, delenv):
	"""the case on the handle of its corpus, under its switches (setenv / delenv: os.environ's or monkeypatch's)"""
	for k in SWITCHES:
		delenv(k)
	for k, v in CASES[name][4].items():
		setenv(k, v)
	Qb, both, hip_kw, _ = options(w, name)
	try:
		return w["c"].query(Qb, **both, **hip_kw)
	finally:
		for k in CASES[name][4]:
			delenv(k)


# ---- the routes.  The enums of vectorian_amd/csrc/vk_route_host.h and the order of vk_query_route_index (vk_internal.h), by name
PLAN = ("LISTED", "SPAN", "FUSED", "BOUNDED", "MULTI_BLOCK", "DOCW_ALL", "DOCG_ALL", "WIDE_ALL")
PASS = ("NONE", "SPAN", "FUSED", "FUSED_LONG", "SCORE32", "LONG_RWMD_FILL", "LONG_BOUND", "DOC", "DOCW", "DOCG", "WIDE")
LIST = ("NONE", "ALL", "APART", "XLONG")
FLOW = ("NARROW", "WIDE", "DOC", "DOCW", "DOCG")
STATE = ("plan", "gap_mode", "wide_gap_mode", "score32_gap_mode", "wave_tiles", "pass_short", "pass_mid", "pass_xlong", "list", "ring_rows",
	"flow", "ostride", "raw", "span_skip_raw")

# name -> (plan, the gap mode of the plan's kernel -- vk_score_kernel's, vk_score32_kernel's, else the one-wave-per-slice family's --,
# pass of the slices of at most 64 tokens, of 65 .. 512, beyond, work list, traceback kernel or None where the case launches none).
# Read off the parent's kernel trace: vk_score_kernel<., ., ., MODE, .> FUSED (a second launch: FUSED_LONG), vk_score32_kernel<MODE, ...>
# MULTI_BLOCK, vk_doc / vk_docw / vk_docg / vk_wide_kernel<false, ...> the pass over a list (after vk_score32 / vk_score) or over every
# row, <true, ...> and vk_flow_kernel the traceback.
ROUTES = {
	"A300_linear_8": ("FUSED", 0, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A300_table_16": ("FUSED", 6, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A300_table_33": ("MULTI_BLOCK", 6, "SCORE32", "NONE", "NONE", "NONE", "WIDE"),
	"A64_affine_8": ("FUSED", 1, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A64_affine_neg_20": ("DOCW_ALL", 1, "DOCW", "NONE", "NONE", "ALL", "DOCW"),
	"A64_linear_20": ("MULTI_BLOCK", 0, "SCORE32", "NONE", "NONE", "NONE", "DOCW"),
	"A64_linear_20_no_score32": ("DOCW_ALL", 0, "DOCW", "NONE", "NONE", "ALL", "DOCW"),
	"A64_linear_40": ("MULTI_BLOCK", 0, "SCORE32", "NONE", "NONE", "NONE", "DOCW"),
	"A64_linear_8": ("FUSED", 0, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A64_rwmd11_8": ("FUSED", 4, "FUSED", "NONE", "NONE", "NONE", None),
	"A64_rwmd1n_20": ("MULTI_BLOCK", 7, "SCORE32", "NONE", "NONE", "NONE", None),
	"A64_rwmd1n_8": ("FUSED", 7, "FUSED", "NONE", "NONE", "NONE", None),
	"A64_submatch_8": ("FUSED", 0, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A64_table_20": ("MULTI_BLOCK", 6, "SCORE32", "NONE", "NONE", "NONE", "WIDE"),
	"A64_table_8": ("FUSED", 6, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A64_tagged_8": ("FUSED", 0, "FUSED", "NONE", "NONE", "NONE", "NARROW"),
	"A64_wmd_8": ("FUSED", 4, "FUSED", "NONE", "NONE", "NONE", None),
	"A64_wrd_20": ("MULTI_BLOCK", 5, "SCORE32", "NONE", "NONE", "NONE", None),
	"B300_exp5_20": ("MULTI_BLOCK", 6, "SCORE32", "DOCG", "NONE", "APART", "DOCG"),
	"B64_exp5_8": ("FUSED", 6, "FUSED", "DOC", "NONE", "APART", "DOC"),
	"B64_linear_20": ("MULTI_BLOCK", 0, "SCORE32", "DOCW", "NONE", "APART", "DOCW"),
	"B64_linear_20_no_apart": ("DOCW_ALL", 0, "DOCW", "DOCW", "NONE", "ALL", "DOCW"),
	"B64_linear_8": ("FUSED", 0, "FUSED", "DOC", "NONE", "APART", "DOC"),
	"B64_linear_8_long_pass": ("FUSED", 0, "FUSED", "FUSED_LONG", "NONE", "NONE", "DOC"),
	"B64_only_8": ("LISTED", 0, "NONE", "NONE", "NONE", "NONE", "DOC"),
	"B64_rising_20": ("MULTI_BLOCK", 6, "SCORE32", "WIDE", "NONE", "APART", "WIDE"),
	"B64_rising_8": ("FUSED", 6, "FUSED", "WIDE", "NONE", "APART", "WIDE"),
	"B64_rwmd11_20": ("MULTI_BLOCK", 4, "SCORE32", "DOCW", "NONE", "APART", None),
	"B64_rwmd11_8": ("FUSED", 4, "FUSED", "DOC", "NONE", "APART", None),
	"B64_rwmd1n_20": ("MULTI_BLOCK", 7, "SCORE32", "LONG_RWMD_FILL", "NONE", "NONE", None),
	"B64_rwmd1n_8": ("FUSED", 7, "FUSED", "FUSED_LONG", "NONE", "NONE", None),
	"B64_wrd_20": ("MULTI_BLOCK", 5, "SCORE32", "LONG_BOUND", "NONE", "NONE", None),
	"C64_exp5_40": ("MULTI_BLOCK", 6, "SCORE32", "WIDE", "WIDE", "APART", "WIDE"),
	"C64_linear_20": ("MULTI_BLOCK", 1, "SCORE32", "DOCW", "DOCW", "APART", "DOCW"),
	"C64_linear_8": ("FUSED", 0, "FUSED", "DOC", "DOC", "APART", "DOC"),
	"C64_rwmd11_8": ("FUSED", 4, "FUSED", "FUSED_LONG", "DOC", "XLONG", None),
	"D64_span_1": ("SPAN", 0, "SPAN", "NONE", "NONE", "NONE", "NARROW"),
	"E64_linear_8": ("FUSED", 0, "FUSED", "DOC", "NONE", "APART", "DOC"),
	"E64_rwmd1n_20": ("MULTI_BLOCK", 7, "SCORE32", "LONG_RWMD_FILL", "NONE", "NONE", None),
}


def check_route(name, state):
	"""state: dict by STATE (vk_query_route, or the CPU driver's line)"""
	plan, mode, short, mid, xlong, lst, flow = ROUTES[name]
	got = (PLAN[state["plan"]], PASS[state["pass_short"]], PASS[state["pass_mid"]], PASS[state["pass_xlong"]], LIST[state["list"]])
	assert got == (plan, short, mid, xlong, lst), (name, got, ROUTES[name])
	key = "score32_gap_mode" if plan == "MULTI_BLOCK" else "gap_mode" if plan in ("FUSED", "BOUNDED", "SPAN", "LISTED") else "wide_gap_mode"
	assert state[key] == mode, (name, key, state[key], mode)
	if flow is not None:
		assert FLOW[state["flow"]] == flow and state["ostride"] == (16 if flow == "NARROW" else 64), (name, state["flow"], state["ostride"], flow)
