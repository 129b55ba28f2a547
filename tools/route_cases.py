"""The named single-query cases of tests/route_cases.py, once each on one GPU: for comparing two commits that must route alike.

  python tools/route_cases.py run RESULTS.txt [INFO.txt]
      runs every case; RESULTS.txt: the result sets (slice ids, score / aligner-score / edge-similarity bit patterns, mappings);
      INFO.txt: per case vk_timings.prepare_ms and, where the library exports vk_query_route, the route.  Between two cases the
      library's one-tile probe kernel (vk_i8_probe_kernel) runs once: the separator `trace` splits a kernel trace by.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_cases.py run RESULTS.txt
  python tools/route_cases.py trace KERNEL_TRACE.csv OUT.txt
      the trace as one line per launch, in order of start, under the name of its case: kernel name with template arguments, grid,
      workgroup, LDS bytes.  Two commits route alike when their OUT.txt and RESULTS.txt are equal byte for byte."""

import csv
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SEPARATOR = "vk_i8_probe"


def run(results_path, info_path=None):
	import route_cases as rc
	from vectorian_amd import core as hip
	hip.init(0)
	lib = hip.lib()
	lib.vk_i8_tile_probe.restype = C.c_int
	lib.vk_i8_tile_probe.argtypes = [C.c_void_p] * 3
	zeros, out = np.zeros((16, 64), np.int8), np.zeros(256, np.int32)
	have_route = hasattr(lib, "vk_query_route")
	worlds = {}
	res, info = [], []
	for name in sorted(rc.CASES):   # (every corpus first: finalize launches kernels of its own)
		if rc.CASES[name][:2] not in worlds:
			worlds[rc.CASES[name][:2]] = rc.build(hip, *rc.CASES[name][:2])
	for name in sorted(rc.CASES):
		w = worlds[rc.CASES[name][:2]]
		hip._check(lib.vk_i8_tile_probe(zeros.ctypes.data, zeros.ctypes.data, out.ctypes.data))
		got = rc.run(w, name, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
		t = got.trimmed()
		res.append("== %s n %d" % (name, got.n))
		for i in range(got.n):
			res.append("%d %08x %08x %s %s" % (t["sentence"][i], t["score"][i:i + 1].view(np.uint32)[0], t["raw_score"][i:i + 1].view(np.uint32)[0],
				",".join(str(int(m)) for m in t["mapping"][i]), ",".join("%08x" % x for x in t["edge_sim"][i].view(np.uint32))))
		line = "%s prepare_ms %.4f" % (name, w["c"].last_timings()["prepare_ms"])
		if have_route:
			import test_gpu_query_route as tq
			line += " route " + " ".join("%s=%d" % kv for kv in tq.query_route(hip, w["c"]).items())
		info.append(line)
	hip._check(lib.vk_i8_tile_probe(zeros.ctypes.data, zeros.ctypes.data, out.ctypes.data))
	for w in worlds.values():
		w["c"].close()
	open(results_path, "w").write("\n".join(res) + "\n")
	if info_path:
		open(info_path, "w").write("\n".join(info) + "\n")


def trace(csv_path, out_path):
	import route_cases as rc
	rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
	names = iter(sorted(rc.CASES))
	lines, started = [], False
	for r in rows:
		if SEPARATOR in r["Kernel_Name"]:
			name = next(names, None)
			started = name is not None
			if started:
				lines.append("== " + name)
			continue
		if started:
			lines.append(r["Kernel_Name"] + "".join(" %s %s" % (k, r[k]) for k in r if k.startswith(("Grid_Size", "Workgroup_Size", "LDS_"))))
	open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
	if len(sys.argv) >= 3 and sys.argv[1] == "run":
		run(*sys.argv[2:4])
	elif len(sys.argv) == 4 and sys.argv[1] == "trace":
		trace(sys.argv[2], sys.argv[3])
	else:
		sys.exit(__doc__)
