"""CPU tier: the owning buffer of a handle's workspaces (vectorian_amd/csrc/vk_devbuf.h) -- the pointer is non-null exactly when the
capacity is non-zero, after failed allocations too.  The header is host-only; a g++ driver runs it over a fake allocator that logs
every call and can be told to fail, under AddressSanitizer with leak detection (a block freed twice or never aborts the driver).
Allocation failure is never provoked on a GPU: this test is where that path is exercised."""

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vectorian_amd", "csrc")
HOST_UNITS = ("vk_internal.h", "vk_corpus.cpp", "vk_query.cpp", "vk_batch.cpp", "vk_longq_host.cpp")


def test_devbuf_keeps_pointer_and_capacity_together(tmp_path):
	exe = str(tmp_path / "devbuf_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address", "-fno-omit-frame-pointer",
		"-I", CSRC, os.path.join(ROOT, "tests", "devbuf_driver.cpp"), "-o", exe], check=True)
	out = subprocess.run([exe], check=True, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
	lines = {}
	for l in out.stdout.strip().split("\n"):
		name, rest = l.split(": ", 1)
		state, calls = rest.split(" |", 1)
		lines[name] = (state, calls.strip())
	assert "INVARIANT BROKEN" not in out.stdout
	assert lines["fresh"] == ("rc=0 ptr=null cap=0 counted=0 live=0", "")
	assert lines["first_reserve"] == ("rc=0 ptr=set cap=100 counted=400 live=400", "[alloc 400]")
	# what fits (the same size, a smaller one, an empty request) performs no allocator call and keeps the pointer
	assert lines["steady_state"] == ("rc=0 ptr=set cap=100 counted=400 live=400", "")
	# growth frees BEFORE it allocates: the peak is never old + new
	assert lines["grow"] == ("rc=0 ptr=set cap=1000 counted=4000 live=4000", "[free 400] [alloc 4000]")
	# a failed allocation: the status comes back, the buffer is empty (null / 0), the counter follows
	assert lines["failed_grow"] == ("rc=3 ptr=null cap=0 counted=0 live=0", "[free 4000] [alloc 20000 FAILED]")
	# ... and a later request that the lost capacity would have held allocates
	assert lines["reserve_after_failure"] == ("rc=0 ptr=set cap=50 counted=200 live=200", "[alloc 200]")
	# the byte counter equals the live bytes after grow - fail - grow - reset
	assert lines["reset"] == ("rc=0 ptr=null cap=0 counted=0 live=0", "[free 200]")
	assert lines["reset_twice"] == ("rc=0 ptr=null cap=0 counted=0 live=0", "")
	# an empty request allocates 16 bytes, so that a pointer exists
	assert lines["empty_request"] == ("rc=0 ptr=set cap=4 counted=16 live=16", "[alloc 16]")
	# destruction frees
	assert lines["before_destruction"] == ("rc=0 ptr=set cap=2000 counted=8000 live=8000", "[free 16] [alloc 8000]")
	assert lines["destroyed"] == ("rc=0 ptr=null cap=0 counted=0 live=0", "[free 8000]")
	# pinned host staging: its own allocator pair, outside the byte count
	assert lines["pinned"] == ("rc=0 ptr=set cap=64 counted=0 live=256", "[alloc_pinned 256]")
	assert lines["pinned_grow"] == ("rc=0 ptr=set cap=128 counted=0 live=512", "[free_pinned 256] [alloc_pinned 512]")
	assert lines["pinned_destroyed"] == ("live=0", "[free_pinned 512]")
	# three arrays sized from one number, the second allocation fails: the first has grown, the second is empty, the third is
	# untouched -- each names exactly the memory it holds
	assert lines["group_failure"] == ("rc=3 raw=20 sim=0 map=640 counted=1360 live=1360", "[free 40] [alloc 80] [free 2560] [alloc 5120 FAILED]")
	# every form in which the host units read a workspace compiles and means the raw pointer
	assert lines["conversions"] == ("rc=0", "")
	assert lines["end"] == ("counted=0 live=0 double_free=0", "")


def _enclosing_functions(text, pattern):
	"""the top-level definitions (a line at column 0 with a parameter list that opens a body) around every match of `pattern`"""
	found = []
	current = None
	for line in text.split("\n"):
		if line and not line[0].isspace() and line[0] not in "}#/" and "(" in line and line.rstrip().endswith("{"):
			current = re.findall(r"([\w:~]+)\(", line)[0]
		if re.search(pattern, line):
			found.append((current, line.strip()))
	return found


def test_workspaces_are_allocated_and_freed_by_the_buffer_type_alone():
	"""no host unit frees a handle's array or keeps a capacity by hand: device and pinned memory are allocated and freed only in the
	functions named here"""
	allowed = {
		"vk_devbuf_alloc", "vk_devbuf_free",                  # the allocator pair of vk_devbuf.h (vk_corpus.cpp)
		"vk_devblock::release", "vk_devblock::~vk_devblock",  # the refcounted block of the arrays several handles read
		"alloc_shared",                                       # ... and its allocations
		"vk_corpus_filter",                                   # temporaries of one call (keep flags, scan, maps), freed before it returns
	}
	seen = set()
	for name in HOST_UNITS:
		text = open(os.path.join(CSRC, name)).read()
		assert "hipFree(c->" not in text and "hipHostFree(c->" not in text, name
		for fn, line in _enclosing_functions(text, r"\bhip(?:Host)?(?:Malloc|Free)\w*\("):
			assert fn in allowed, (name, fn, line)
			seen.add(fn)
		# no capacity kept beside a pointer: neither a member of the handle nor a use of one
		assert not re.findall(r"\b\w+_cap\b", text), (name, re.findall(r"\b\w+_cap\b", text))
	assert seen == allowed   # (the scan sees what it is meant to see)
	internal = open(os.path.join(CSRC, "vk_internal.h")).read()
	struct = internal[internal.index("struct vk_corpus"):]
	# every array of the handle's own is a buffer; the raw device pointers left are the aliases into the shared block
	raw = set(re.findall(r"\*\s*(d_\w+)", struct[:struct.index("// units")]))
	assert raw == {"d_tiles", "d_mag", "d_tok_id", "d_pos", "d_tag", "d_sent_start", "d_sent_end", "d_long_groups"}, raw
