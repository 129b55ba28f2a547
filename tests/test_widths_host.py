"""The inputs of the width sweep (test_gpu_widths.py) can fail: on the oracle alone, a corpus whose rows lost their last live
feature, or whose last block of 16 features is counted twice, scores differently on more than half of its slices -- by more than
twice the width's tolerance -- and returns other winners.  No GPU: this is the argument that a kernel with a dropped or doubled
tail feature cannot pass the sweep."""

import numpy as np
import pytest

import width_cases as wc

CASES = [(layout, d) for layout, table in wc.TABLES.items() for d in table]


def stored_rows(oracle, case):
	return oracle.normalize_rows(case.raw) if case.layout == "f32" else oracle.normalize_rows_bf16(case.raw)[0]


def stored_query(oracle, case, q):
	return oracle.normalize_rows(q) if case.layout == "f32" else oracle.normalize_rows_bf16(q)[0]


def all_scores(oracle, case, rows, Q, q_ids, **kw):
	if case.layout == "static":
		return oracle.find(layout=oracle.LAYOUT_STATIC, d=case.d, sent_off=case.off, tok_id=case.tok_id, E=rows, Q=Q, q_ids=q_ids,
			max_matches=10, want_all_scores=True, n_threads=4, **kw)
	return oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=case.d, sent_off=case.off, X=rows, Q=Q, max_matches=10, want_all_scores=True,
		n_threads=4, **kw)


@pytest.mark.parametrize("layout,d", CASES)
def test_a_lost_or_doubled_tail_feature_shows(oracle, layout, d):
	case = wc.Case(layout, d)
	rows = stored_rows(oracle, case)
	live = case.lens > 0
	if layout == "static":
		q_ids = case.static_ids(7)
		qv = case.query(7)
		Q = stored_query(oracle, case, qv)
		Q[q_ids >= 0] = rows[q_ids[q_ids >= 0]]
	else:
		q_ids, Q = None, stored_query(oracle, case, case.query(7))
	routes = (
		(1e-4, dict(locality=0, gap_s=0.1, gap_t=0.1, min_score=0.0)),
		(2e-5, dict(algorithm=oracle.ALG_RWMD, rwmd=(True, True, True), min_score=-10.0)),
	)
	for project, kw in routes:
		t = wc.tol(d, project)
		ref = all_scores(oracle, case, rows, Q, q_ids, **kw)
		assert len(ref["sentence"]) == 10
		for kind in ("zero", "double"):
			bad = all_scores(oracle, case, wc.mutate(rows, d, kind), Q, q_ids, **kw)
			moved = np.abs(bad["all_scores"][live] - ref["all_scores"][live]) > 2 * t
			print(f"{layout} d {d} {kind} {'rwmd' if 'algorithm' in kw else 'align'}: {moved.mean():.3f} of {live.sum()} slices moved by more than {2 * t:.2e}")
			assert moved.mean() > 0.5, (kind, kw, moved.mean())
			assert set(bad["sentence"].tolist()) != set(ref["sentence"].tolist()), (kind, kw)
