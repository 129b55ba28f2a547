"""CPU tier: the host side of the bound pass's flat tail -- vk_host::bound_tail_cost and vk_host::bound_tail_choice of
vk_bound_host.h through a stand-alone g++ driver (AddressSanitizer, UBSan; tests/bound_tail_driver.cpp), and where the switch is read."""

import os
import re

import numpy as np
import pytest

import bound_cases as bc

F = np.float32
KS = np.arange(0, 65)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	return bc.build_driver(tmp_path_factory, "bound_tail_driver")


def cost(driver, w, k, rows):
	line = driver("cost", k, rows, len(w), *["%.9g" % x for x in w])
	assert len(line) == 1
	return np.array([int(line[0], 16)], dtype=np.uint32).view(F)[0]


def test_the_tail_cost_is_a_minimum_not_the_next_entry(driver):
	dips = (np.where(KS == 20, 0.12, np.where(KS == 40, 0.07, 0.15 + 0.02 * np.minimum(KS, 12) + 0.05 * np.cos(KS))) * (KS > 0)).astype(F)
	for k in (1, 3, 4, 6, 19):
		assert cost(driver, dips, k, 32) == dips[20] and cost(driver, dips, k, 64) == dips[40]
	assert cost(driver, dips, 20, 32) == dips[21:33].min() and cost(driver, dips, 20, 32) > dips[20]   # an entry at or below K is no part of the tail
	assert cost(driver, dips, 40, 64) == dips[41:].min()
	exp5 = (1 - 2.0 ** (-KS / 5)).astype(F)
	for k in (3, 4, 6):
		assert cost(driver, exp5, k, 32) == exp5[k + 1] and cost(driver, exp5, k, 64) == exp5[k + 1]   # a rising table: the next entry
	falling = (1.0 / (1 + KS)).astype(F)
	assert cost(driver, falling, 4, 32) == falling[32] and cost(driver, falling, 4, 64) == falling[64]


def test_k_at_and_beyond_the_tables_useful_length(driver):
	w = (0.1 * KS).astype(F)
	assert cost(driver, w, 31, 32) == w[32] and cost(driver, w, 63, 64) == w[64]        # one entry in the tail
	for k, rows in ((32, 32), (33, 32), (64, 64), (100, 64)):
		assert np.isposinf(cost(driver, w, k, rows))                                     # none: the identity of the minimum
	# a table shorter than the form's history reads as +inf beyond its end (vk_host::gap_cost): the tail's minimum is over what it holds
	assert cost(driver, w[:10], 4, 32) == w[5] and np.isposinf(cost(driver, w[:5], 4, 32)) and np.isposinf(cost(driver, w[:3], 4, 64))


def test_the_switch_by_value_and_mode(driver):
	rows = [(env, mode) for env in ("0", "1", "x", "-") for mode in (-1, 0, 1)]
	out = driver("choice", *[x for row in rows for x in row])
	got = {row: int(v) for row, v in zip(rows, out)}
	for mode in (-1, 0, 1):
		assert got[("0", mode)] == 0 and got[("1", mode)] == 1
		assert got[("-", mode)] == got[("x", mode)] == int(mode == 0)   # unset, or any other value: on where the pass is on by size


def test_the_switch_is_read_beside_bound_bits_wanted():
	internal = open(os.path.join(bc.CSRC, "vk_internal.h")).read()
	assert re.search(r"inline bool bound_tail_wanted\(int mode\) \{ return vk_host::bound_tail_choice\(getenv\(\"VK_BOUND_TAIL\"\), mode\); \}", internal)
	assert internal.index("inline int bound_bits_wanted") < internal.index("inline bool bound_tail_wanted")
	query = open(os.path.join(bc.CSRC, "vk_query.cpp")).read()
	assert "getenv" not in query and query.count("bound_tail_wanted(") == 1
	assert "getenv" not in open(os.path.join(bc.CSRC, "vk_bound_host.h")).read()
