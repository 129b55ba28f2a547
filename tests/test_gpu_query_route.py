"""-m gpu: the route of a single query (vectorian_amd/csrc/vk_route_host.h).  Each named case of route_cases.py runs once
on its tiny corpus; vk_query_route, an internal export of the library as vk_batch_state is, says which kernels served it, and that is
held against the table written from the kernel trace of the commit before the route existed (route_cases.ROUTES).  The result set of
each case against the oracle, as the neighbouring tests do: alignments with their tracebacks and the relaxed WMD bit for bit, the
exact transports within 1e-4."""

import ctypes as C

import numpy as np
import pytest

import route_cases as rc
from helpers import assert_same_results

pytestmark = pytest.mark.gpu

WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def worlds():
	yield
	for w in WORLDS.values():
		w["c"].close()
	WORLDS.clear()


def query_route(hip, c):
	lib = hip.lib()
	lib.vk_query_route.restype = C.c_int
	lib.vk_query_route.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(len(rc.STATE), dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_query_route(c._h, st.ctypes.data))
	return dict(zip(rc.STATE, st.tolist()))


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_route_and_result_of_a_case(hip, oracle, monkeypatch, name):
	corpus, d = rc.CASES[name][:2]
	if (corpus, d) not in WORLDS:
		WORLDS[(corpus, d)] = rc.build(hip, corpus, d)
	w = WORLDS[(corpus, d)]
	got = rc.run(w, name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
	rc.check_route(name, query_route(hip, w["c"]))
	Qb, both, hip_kw, ref_kw = rc.options(w, name)
	if w["static"]:
		ref_kw.update(layout=oracle.LAYOUT_STATIC, tok_id=w["tok"], E=w["Eb"])
	else:
		ref_kw.update(layout=oracle.LAYOUT_CONTEXTUAL, X=w["Xb"])
	only = hip_kw.get("only_slices")
	if only is not None:
		both = dict(both, max_matches=len(w["off"]) - 1, min_score=-1e9)   # every slice, then the listed ones
	ref = oracle.find(d=d, sent_off=w["off"], Q=Qb, **both, **ref_kw)
	algorithm = both.get("algorithm", rc.ALIGN)
	if only is not None:
		by_slice = {int(s): i for i, s in enumerate(ref["sentence"])}
		idx = [by_slice[int(s)] for s in only]
		ref = {k: np.asarray(ref[k])[idx] for k in ("score", "sentence", "mapping")}
		assert_same_results(got.trimmed(), ref)
	elif algorithm == rc.ALIGN:
		assert_same_results(got.trimmed(), ref)
	elif algorithm == rc.RWMD and not both.get("wmd_full"):
		assert_same_results(got.trimmed(), ref, check_mapping=False, exact=True)
	else:
		assert_same_results(got.trimmed(), ref, check_mapping=False)
