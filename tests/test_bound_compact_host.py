"""CPU tier: the host side of the compact 6-bit shadow -- the format vk_host::shadow_format_of gives it, the quantizer
under bf16_meta (s and e rounded up to bf16, the codes computed with that s) and the packer of a compact tile in vk_bound_host.h --
run through the stand-alone program tests/bound6c_driver.cpp, built twice with g++ (plain, and under AddressSanitizer and UBSan;
both must print the same), and held against the statement in numpy (tests/bound6c_cases.py):
  * the format's numbers: 6 bits, three K-steps, tiles of 3,712 bytes with the (s, e) words at 3,648, a query tile of 4,608;
  * every byte of a packed tile at 289, 300, 303 and 304 features, s and e as bf16 among them, and N and X;
  * a row of zeros; a row whose largest element is a bf16 multiple of 7.5 (s = max / 7.5 exactly: nothing to round); a row with one
    large component;
  * e is at least the true error of the row in float64, for every row, and |x / s| <= 7.5: nothing clips;
  * shadow_format_of with the arguments it had before answers what it answered before."""

import os
import subprocess

import numpy as np
import pytest

import bound6_cases as b6
import bound6c_cases as b6c
import bound_cases as bc
from bound_cases import hexbits

F = np.float32
WIDTHS = (289, 300, 303, 304)
COMPACT = 60   # vk_host::bits6_compact


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
	"""run(command, *numbers) -> the lines the program prints, the same from the plain and from the sanitized build"""
	src = os.path.join(bc.ROOT, "tests", "bound6c_driver.cpp")
	tmp = tmp_path_factory.mktemp("bound6c_driver")
	exes = []
	for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])):
		exe = str(tmp / name)
		subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, "-I", bc.CSRC, src, "-o", exe], check=True)
		exes.append(exe)

	def run(what, *numbers):
		text = " ".join(str(x) for x in numbers)
		outs = [subprocess.run([exe, what], input=text, check=True, capture_output=True, text=True).stdout for exe in exes]
		assert outs[0] == outs[1]
		return outs[0].split("\n")[:-1]
	return run


def rows_of(d, seed=0):
	"""sixteen rows as a corpus stores them (bf16 values), the special ones of the module's text among them"""
	rng = np.random.default_rng(1000 + d + seed)
	x = b6.stored(rng.standard_normal((16, d)).astype(F))
	x[3] = 0.0                                                    # a row of zeros
	x[6, d - 1] = F(0.9375)                                       # the largest element: 7.5 / 8, so s = 0.125, a bf16 value as it is
	x[6] = np.clip(x[6], -0.9375, 0.9375)
	x[11] = b6.stored(F(1e-3) * x[11][None, :])[0]; x[11, d // 2] = F(-0.99609375)   # one large component
	assert (b6.synth.bf16_bits_to_f32(b6.synth.to_bf16_bits(x)) == x).all()
	return np.ascontiguousarray(x, dtype=F)


def quantize_by_driver(driver, rows):
	out = driver("quantize", len(rows), rows.shape[1], *[hexbits(v) for v in rows.reshape(-1)])
	f = [line.split() for line in out]
	meta = np.array([[int(w, 16) for w in t[:4]] for t in f], dtype=np.uint32).view(F)
	codes = np.array([[int(w) for w in t[4:]] for t in f], dtype=np.uint8).reshape(len(rows), rows.shape[1])
	return codes, meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]


def test_format_of_the_compact_shadow(driver):
	asked = [bc.factory_args(d, COMPACT) for d in WIDTHS]
	out = driver("format", len(asked), *sum(asked, []))
	for d, line in zip(WIDTHS, out):
		# bits steps step_features live tile_bytes meta_offset qtile_bytes gamma_width
		assert [int(v) for v in line.split()] == [6, 3, 128, 2, 3712, 3648, 4608, 320], (d, line)
	assert 3712 == 29 * 128 == 2 * 1536 + 32 * 12 + 16 * 12 + 16 * 4
	# beside the widths, fp32 rows, the static layout: none; 768-d rows: the 8-bit form, as for 6
	none = [bc.factory_args(d, COMPACT) for d in (288, 305, 752, 769)] + [bc.factory_args(300, COMPACT, prec=1), bc.factory_args(300, COMPACT, layout=1)]
	assert driver("format", len(none), *sum(none, [])) == ["none"] * len(none)
	assert [int(v) for v in driver("format", 1, *bc.factory_args(768, COMPACT))[0].split()] == [8, 12, 64, 4, 12416, 12288, 12288, 768]


def test_todays_arguments_give_todays_formats(driver):
	"""the table of DESIGN 11.1 as it stood: 8 and 6 bits at 300-d, 8 bits at 768-d whatever is asked"""
	asked = [bc.factory_args(300, 8), bc.factory_args(300, 6), bc.factory_args(289, 6), bc.factory_args(304, 8), bc.factory_args(768, 8), bc.factory_args(768, 6),
		bc.factory_args(753, 8), bc.factory_args(300, 0), bc.factory_args(300, 7)]
	got = [[int(v) for v in line.split()] for line in driver("format", len(asked), *sum(asked, []))]
	six, eight, wide = [6, 3, 128, 2, 3968, 3840, 4608, 320], [8, 5, 64, 3, 5248, 5120, 5120, 320], [8, 12, 64, 4, 12416, 12288, 12288, 768]
	assert got == [eight, six, six, eight, wide, wide, wide, eight, eight], got


@pytest.mark.parametrize("d", WIDTHS)
def test_quantizer_rounds_s_and_e_up_to_bf16(driver, d):
	x = rows_of(d)
	codes, s, e, n, a = quantize_by_driver(driver, x)
	rc, rs, re, rn, ra = b6c.quantize6c(x)
	assert (codes == rc).all()
	for got, ref in ((s, rs), (e, re), (n, rn), (a, ra)):
		assert (got.view(np.uint32) == ref.view(np.uint32)).all(), (got, ref)
	assert not (s.view(np.uint32) & 0xffff).any() and not (e.view(np.uint32) & 0xffff).any()          # bf16 values
	m = np.abs(x).max(axis=1)
	assert (s.astype(np.float64) * 7.5 >= m).all()                                                     # s >= max|x| / 7.5: nothing clips
	assert (s.astype(np.float64) <= (m / F(7.5)).astype(F).astype(np.float64) * (1 + 2.0 ** -7)).all()   # ... and the least such bf16
	big = np.abs(x).argmax(axis=1)
	for r in range(16):
		if m[r] > 0:
			assert int(codes[r, big[r]] & 31) == 31                # the largest element is still +-7.5: s grew by less than 2^-7
	# e is an upper bound of the true error, in float64, and within the rounding of a bf16 of it
	true = np.sqrt(((x.astype(np.float64) - b6.values(codes, s)) ** 2).sum(axis=1))
	assert (e.astype(np.float64) >= true).all()
	assert (e.astype(np.float64) <= true * (1 + 1e-5) * (1 + 2.0 ** -7) + 1e-45).all()
	# the rows of the module's text
	assert not codes[3].any() and s[3] == 0 and e[3] == 0 and n[3] == 0 and a[3] == 0
	assert s[6] == F(0.125) and codes[6, d - 1] == 31
	assert codes[11, d // 2] == 63
	# the plain quantizer differs from this one: the test can tell them apart
	_, ps, pe, _, _ = b6.quantize6(x)
	assert (ps.view(np.uint32) != s.view(np.uint32)).any() and (pe.view(np.uint32) != e.view(np.uint32)).any()
	assert ps[6] == s[6]                                         # ... except where max / 7.5 is a bf16 value already


@pytest.mark.parametrize("d", WIDTHS)
def test_every_byte_of_a_compact_tile(driver, d):
	x = rows_of(d, seed=1)
	out = driver("tile", *bc.factory_args(d, COMPACT), *[hexbits(v) for v in x.reshape(-1)])
	got = np.array([int(v) for v in out[0].split()], dtype=np.uint8)
	rc, rs, re, rn, ra = b6c.quantize6c(x)
	codes = np.zeros((16, 384), dtype=np.uint8)
	codes[:, :d] = rc
	want = b6c.pack_tile_c(codes, rs, re)
	assert len(got) == b6c.TILE
	diff = np.flatnonzero(got != want)
	assert len(diff) == 0, (diff[:8], got[diff[:8]], want[diff[:8]])
	words = got[b6c.META:].view(np.uint32)
	assert ((words << 16).view(F) == rs).all() and ((words & 0xffff0000).view(F) == re).all()        # s and e as the kernel expands them
	assert out[1].split() == [hexbits(rn.max()), hexbits(ra.max())]
	if d < 304:
		# zero codes from d on: the last live lane's bits past feature d
		lane = b6c.lane_words(codes[0, 288:320])
		assert not lane[12:].any() and (codes[:, d:] == 0).all()
