"""CPU tier: the route of a query on a contextual handle under an operator chain (route_facts::chained, vk_route_host.h).
A g++ driver with its own main (once plain, once under AddressSanitizer and UBSan) enumerates the facts tests/route_driver.cpp
enumerates, every switch on its own, and holds three rules:
  - the plan is never PLAN_BOUNDED (the shadow bounds the clipped cosine) and never PLAN_SPAN;
  - the query is refused -- VK_ERR_UNSUPPORTED, a message that names the chain -- exactly when a class of slices the corpus holds
    would be scored by a pass that is neither vk_score_kernel nor vk_score32_kernel (read off the unchained route of the same facts
    with only_slices aside), or the unchained route refuses it too;
  - otherwise every field is the unchained answer's, but for the plan (and the span kernel's pass) where bound or span was dropped."""

import os
import subprocess

import pytest

from test_devbuf import CSRC, ROOT


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def enumerated(request, tmp_path_factory):
	extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
	exe = str(tmp_path_factory.mktemp("route_chain_" + request.param) / "route_chain_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
		os.path.join(ROOT, "tests", "route_chain_driver.cpp"), "-o", exe], check=True)
	return subprocess.run([exe, "enumerate"], check=True, capture_output=True, text=True).stdout.splitlines()


def test_no_rule_is_violated(enumerated):
	assert not [line for line in enumerated if line.startswith("VIOLATED")], enumerated[:10]
	words = enumerated[-1].split()
	counts = dict(zip(words[0::2], map(int, words[1::2])))
	assert counts["violations"] == 0
	# the grid reaches every case the rules speak of
	assert counts["points"] > 100000 and counts["refused"] > 0 and counts["fused"] > 0 and counts["multi_block"] > 0
	assert counts["dropped_bound"] > 0 and counts["dropped_span"] > 0
	assert counts["refused"] + counts["fused"] + counts["multi_block"] <= counts["points"]
