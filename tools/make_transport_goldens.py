"""Writes tests/golden/transport_lp.npz: `python tools/make_transport_goldens.py`.

Per case of tests/transport_cases.py an array [queries x modes x slices] of the float64 LP score of every slice (tests/transport_lp.py: scipy's HiGHS;
NaN for an empty slice), and per case a sha256 over its input arrays.  Needs scipy and the oracle (for the bf16 rows, magnitudes
and similarities the problems are stated from); the GPU tier needs neither scipy nor this tool, only the file."""

import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
	from oracle import vk_oracle as vo
	import transport_lp
	out = transport_lp.all_scores(vo)
	np.savez_compressed(transport_lp.GOLDEN, **out)
	n = sum(int(np.isfinite(v).sum()) for k, v in out.items() if not k.endswith("/sha256"))
	print("wrote", transport_lp.GOLDEN, f"{len(out)} arrays, {n} LP scores, {os.path.getsize(transport_lp.GOLDEN)} bytes")


if __name__ == "__main__":
	main()
