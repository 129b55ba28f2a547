"""CPU tier: the vector similarities beside the cosine (vectorian_amd/csrc/vk_sim_src_host.h).  The header is the one
definition the table kernel compiles for the device; here a g++ driver (once plain, once under AddressSanitizer and UBSan, run as a
stand-alone program) holds its cell
  * against the numpy restatement of its stated order (vector_sim_cases.source_matrix) bit for bit, for the forms made of exactly
    rounded operations -- p = 1, p = 2, the sqrt-cosine -- at every width where a partial sum changes length, with zero rows and equal
    rows among the inputs;
  * against the reference's own outputs (tests/golden/vector_sims_reference.npz, tools/make_goldens.py) for every form.  The reference
    sums in float32 pairwise, the header in double in its fixed order: they differ by summation-order noise.  MEASURED is the largest
    relative deviation of the header's cell from the golden over all its shapes and sources; the bound asserted is 4 x that (the noise
    varies with the input; a wrong term is off by orders of magnitude more).
Then the Python classes: compute() against the golden under the same bound, and the reference's name strings."""

import os
import subprocess

import numpy as np
import pytest

import vector_sim_cases as vc
from test_devbuf import CSRC, ROOT

from vectorian_amd import core
from vectorian_amd.embedding import Vectors
from vectorian_amd.sim import EuclideanDistance, ImprovedSqrtCosineSim, ModifiedVectorSim, PNormDistance, Scale, DistanceToSimilarity

# max |header - golden| / |golden| over the golden file (p = 0.5, 1, 2, 3 and the sqrt-cosine; d = 8, 300, 768): 2.813e-7, at the
# sqrt-cosine of the 768-d shape (p = 0.5: 2.62e-7; p = 1, 2, 3: at most 1.1e-7)
MEASURED = 2.82e-7
BOUND = 4 * MEASURED

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "vector_sims_reference.npz"))
SOURCES = {"pnorm_0.5": (core.VK_SIMSRC_PNORM, 0.5), "pnorm_1": (core.VK_SIMSRC_PNORM, 1.0), "pnorm_2": (core.VK_SIMSRC_PNORM, 2.0),
	"pnorm_3": (core.VK_SIMSRC_PNORM, 3.0), "sqrt_cosine": (core.VK_SIMSRC_SQRT_COSINE, 0.0)}
EXACT = ("pnorm_1", "pnorm_2", "sqrt_cosine")


def _build(tmp, extra):
	exe = str(tmp / "vector_sim_driver")
	subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", *extra, "-I", CSRC,
		os.path.join(ROOT, "tests", "vector_sim_driver.cpp"), "-o", exe], check=True)
	return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
	exe = _build(tmp_path_factory.mktemp("vector_sim_" + request.param), extra)

	def run(what, text):
		return subprocess.run([exe, what], input=text, check=True, capture_output=True, text=True).stdout.split()
	return run


def _bits(x):
	return int(np.float32(x).view(np.uint32))


def _cells(driver, source, A, B):
	A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
	head = f"{source[0]} {_bits(source[1]):x} {A.shape[1]} {len(A)} {len(B)}\n"
	body = "\n".join(f"{int(u):x}" for u in np.concatenate([A.ravel(), B.ravel()]).view(np.uint32))
	out = driver("cells", head + body + "\n")
	return np.array([int(w, 16) for w in out], dtype=np.uint32).view(np.float32).reshape(len(A), len(B))


def _inputs(d, seed):
	"""six rows against five: raw normal rows, a zero row on either side, a pair of equal rows (distance exactly 0)"""
	rng = np.random.default_rng(seed)
	A, B = rng.standard_normal((6, d)).astype(np.float32), rng.standard_normal((5, d)).astype(np.float32)
	A[1] = 0
	B[2] = 0
	B[3] = A[4]
	return A, B


# every width of the issue, and the widths around which a partial sum of the order changes length (d mod 4) or the table kernel's
# 16-feature block count changes (d mod 16)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 64, 67, 100, 300, 768)


@pytest.mark.parametrize("name", EXACT)
def test_the_exactly_rounded_forms_are_the_stated_order_bit_for_bit(driver, name):
	source = SOURCES[name]
	for d in WIDTHS:
		A, B = _inputs(d, 100 + d)
		got, ref = _cells(driver, source, A, B), vc.source_matrix(A, B, source)
		differ = got.view(np.uint32) != ref.view(np.uint32)
		assert not differ.any(), (name, d, got[differ][:5], ref[differ][:5])
		if name == "sqrt_cosine":
			assert (got[1] == 0).all() and (got[:, 2] == 0).all() and got[4, 3] > 0.99   # 0 / 0 is 0; equal rows: 1 up to the roundings
		else:
			assert got[4, 3] == 0 and (got[[0, 2, 3, 5]] > 0).all()


def _deviation(got, ref):
	with np.errstate(divide="ignore", invalid="ignore"):
		rel = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.abs(ref.astype(np.float64))
	return float(np.nanmax(np.where(ref == 0, np.where(got == 0, 0.0, np.inf), rel)))


def test_the_header_against_the_golden(driver):
	worst = {}
	for shape in ("small", "wide", "tiny"):
		A, B = GOLDEN[shape + "_a"], GOLDEN[shape + "_b"]
		for name, source in SOURCES.items():
			worst[shape, name] = _deviation(_cells(driver, source, A, B), GOLDEN[f"{shape}_{name}"])
	print({k: f"{v:.3g}" for k, v in worst.items()})
	print("max relative deviation from the golden:", max(worst.values()), "bound:", BOUND)
	assert max(worst.values()) <= BOUND, worst


def test_the_numpy_restatement_against_the_golden():
	"""what the GPU tier builds its reference tables from"""
	for shape in ("small", "wide", "tiny"):
		for name, source in SOURCES.items():
			assert _deviation(vc.source_matrix(GOLDEN[shape + "_a"], GOLDEN[shape + "_b"], source), GOLDEN[f"{shape}_{name}"]) <= BOUND, (shape, name)


def test_check_refuses_what_the_entry_point_refuses(driver):
	def status(kind, arg):
		return driver("check", f"{kind} {_bits(arg):x}\n")
	assert status(core.VK_SIMSRC_COSINE, 0.0) == ["0"] and status(core.VK_SIMSRC_SQRT_COSINE, 0.0) == ["0"]
	assert status(core.VK_SIMSRC_PNORM, 2.0) == ["0"] and status(core.VK_SIMSRC_PNORM, 0.5) == ["0"]
	for kind, arg in ((3, 1.0), (-1, 1.0), (core.VK_SIMSRC_PNORM, 0.0), (core.VK_SIMSRC_PNORM, -2.0), (core.VK_SIMSRC_PNORM, np.inf),
			(core.VK_SIMSRC_PNORM, np.nan)):
		assert status(kind, arg) == [str(core.VK_ERR_INVALID)], (kind, arg)


# ---- the Python classes (vectorian/sim/vector.py)

def test_the_classes_compute_the_golden():
	sims = {"pnorm_0.5": PNormDistance(0.5), "pnorm_1": PNormDistance(1), "pnorm_2": PNormDistance(2), "pnorm_3": PNormDistance(3),
		"sqrt_cosine": ImprovedSqrtCosineSim()}
	for shape in ("small", "wide", "tiny"):
		a, b = Vectors(GOLDEN[shape + "_a"]), Vectors(GOLDEN[shape + "_b"])
		for name, sim in sims.items():
			out = np.full((len(GOLDEN[shape + "_a"]), len(GOLDEN[shape + "_b"])), np.nan, np.float32)
			sim(a, b, out)
			assert _deviation(out, GOLDEN[f"{shape}_{name}"]) <= BOUND, (shape, name)
		out = np.empty((len(GOLDEN[shape + "_a"]), len(GOLDEN[shape + "_b"])), np.float32)
		EuclideanDistance()(a, b, out)
		assert _deviation(out, GOLDEN[shape + "_pnorm_2"]) <= BOUND
	assert GOLDEN["small_pnorm_2"][0, 0] == 0 and (GOLDEN["tiny_sqrt_cosine"][1] == 0).all()   # equal rows; the zero row


def test_names_and_sources():
	assert PNormDistance(2).name == "p-norm(2)" and PNormDistance().name == "p-norm(2)" and PNormDistance(0.5).name == "p-norm(0.5)"
	assert EuclideanDistance().name == "p-norm(2)" and ImprovedSqrtCosineSim().name == "improved-sqrt-cosine"
	assert PNormDistance(3).sim_source == (core.VK_SIMSRC_PNORM, np.float32(3)) and isinstance(PNormDistance(3).sim_source[1], np.float32)
	assert EuclideanDistance().sim_source == (core.VK_SIMSRC_PNORM, np.float32(2))
	assert ImprovedSqrtCosineSim().sim_source == (core.VK_SIMSRC_SQRT_COSINE, np.float32(0))
	assert ModifiedVectorSim(PNormDistance(2), Scale(0.25), DistanceToSimilarity()).name == "(1 - (p-norm(2) * 0.25))"
	with pytest.raises(TypeError):
		EuclideanDistance(2)   # (upstream's takes a scale its base class refuses; this one takes nothing)
	header = open(os.path.join(ROOT, "include", "vectorian_hip.h")).read()
	assert "VK_SIMSRC_COSINE = 0, VK_SIMSRC_PNORM = 1, VK_SIMSRC_SQRT_COSINE = 2" in header
	assert (core.VK_SIMSRC_COSINE, core.VK_SIMSRC_PNORM, core.VK_SIMSRC_SQRT_COSINE) == (0, 1, 2)
