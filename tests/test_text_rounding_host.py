"""CPU: the designed sets of text_rounding_cases.py hold their patterns on the oracle alone, the decimal expectation
agrees with Python's exact `%.12f`, and the two host formatters (cli::fmt_fixed12 behind `distance --host-selftest format`,
dst_format_distance = snprintf("%.12f")) print every exact tie of the 12th decimal, with integer parts of one to eight
digits and either sign, as the exact quotient rounded half to even (the ctypes leg is what reaches glibc's snprintf).
test_gpu_text_rounding.py runs the same sets through the device's put_fixed12 and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import oracle
import text_rounding_cases as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
THREADS = min(16, len(os.sched_getaffinity(0)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def test_expected_field_on_known_values():
    assert tr.expected_field(1, 8192) == "0.000122070312"          # 0.0001220703125: a tie, the even neighbour is below
    assert tr.expected_field(3, 8192) == "0.000366210938"          # 0.0003662109375: a tie, the even neighbour is above
    assert tr.expected_field(2, 16384) == "0.000122070312" and tr.expected_field(9, 24576) == "0.000366210938"
    assert tr.expected_field(1, 16384) == "0.000061035156"         # 0.00006103515625: below the tie
    assert tr.expected_field(0, 8192) == "0.000000000000" and tr.expected_field(8192, 8192) == "1.000000000000"
    assert tr.expected_field(0, 0) == "NaN"
    assert tr.is_tie(1, 8192) and not tr.rounds_up(1, 8192) and tr.rounds_up(3, 8192)
    assert not tr.is_tie(1, 16384) and not tr.is_tie(2, 8192) and not tr.is_tie(0, 8192)


def test_tie_set_holds_its_pattern_on_the_oracle():
    codes, cases, ids = tr.tie_alignment()
    assert codes.shape == (1 + len(cases), tr.TIE_L) and len(codes) >= 300    # a matrix row crosses the 256-cell chunk
    assert np.isin(codes[0], tr.KNOWN).all()
    tl = oracle.tallies_rect("raw", codes[:1], codes, threads=THREADS)[0]
    assert [tuple(int(x) for x in t) for t in tl[1:]] == cases
    assert tuple(int(x) for x in tl[0]) == (0, tr.TIE_L)
    for k, (n, d) in enumerate(cases[:40], start=1):                          # ... and by the per-pair entry point
        assert tuple(int(x) for x in oracle.tallies("raw", codes[0], codes[k])) == (n, d)
    # what the issue asks the set to hold
    in_8192 = {n for n, d in cases if d == tr.TIE_D}
    assert set(tr.FIXED_A) <= in_8192 and len([n for n in in_8192 if n % 2]) >= 208
    assert {(2, 16384), (6, 16384), (3, 24576), (9, 24576), (1, 16384), (0, 8192), (8192, 8192)} <= set(cases)
    assert all((a - 1, 8192) in cases and (a + 1, 8192) in cases for a in (1, 3, 4095, 8191))
    assert len([c for c in cases if c[1] == 16384 and tr.is_tie(*c)]) >= 24
    assert len([c for c in cases if c[1] == 24576 and tr.is_tie(*c)]) >= 24
    ties = [c for c in cases if tr.is_tie(*c)]
    up = [c for c in ties if tr.rounds_up(*c)]
    assert len(up) >= 80 and len(ties) - len(up) >= 80, (len(ties), len(up))
    for n, d in ties:                                                         # the last digit says which way it went
        kept = int(tr.expected_field(n, d)[-1])
        assert kept % 2 == 0 and (n * 10 ** 12 // d + (1 if (n, d) in up else 0)) % 10 == kept
    # ids: every length from 0 to 22, exactly one empty
    assert {len(i) for i in ids} == set(range(23)) and ids.count("") == 1 and len(set(ids)) == len(ids)
    sub = tr.cli_subset(cases)
    assert sub[0] == 0 and 200 <= len(sub) <= 260 and all(cases[k - 1][1] == tr.TIE_D for k in sub[1:])
    assert len([k for k in sub[1:] if tr.rounds_up(*cases[k - 1])]) >= 80


def test_long_set_holds_its_pattern_on_the_oracle():
    codes, cases, ids = tr.long_jc69_alignment()
    assert codes.shape == (5, tr.LONG_L) and tr.LONG_L > 65535                # the 32-bit tally form
    tl = oracle.tallies_rect("jc69", codes[:1], codes, threads=THREADS)[0]
    assert [tuple(int(x) for x in t) for t in tl[1:]] == cases
    v = oracle.all_pairs_square("jc69", codes, pair_range=(0, 4))
    text = ["%.12f" % x for x in v]
    assert text[0].startswith("10.18") and len(text[0]) == 15                 # one character more than any other test prints
    assert text[1].startswith("8.97") and len(text[1]) == 14
    assert np.isnan(v[2]) and text[3] == "0.000003814722"   # p + 2/3 p^2 at p = 1 / 262,143
    assert [da.format_distance("jc69", da.finalize("jc69", t)) for t in tl[1:]] == [oracle.format_distance(float(x)) for x in v]


def test_decimal_expectation_is_exact_percent_formatting():
    """expected_field against Python's "%.12f" (correctly rounded from the exact binary value) of the double n / d on
    every designed case and every value of the formatter test"""
    _, cases, _ = tr.tie_alignment()
    for n, d in cases:
        assert tr.expected_field(n, d) == "%.12f" % (n / d), (n, d)
    for s, k, a in tr.format_values():
        assert tr.expected_format(s, k, a) == "%.12f" % tr.format_value(s, k, a), (s, k, a)


def test_both_host_formatters_on_every_exact_tie():
    cases = tr.format_values()
    assert len(cases) == 2 * 7 * 4096
    vals = [tr.format_value(*c) for c in cases]
    want = [tr.expected_format(*c) for c in cases]
    assert want[0] == "0.000122070312" and want[1] == "0.000366210938" and want[4096] == "1.000122070312"
    assert want[-1] == "-17999999.999877929688"
    # cli::fmt_fixed12
    text = "".join(float.hex(v) + "\n" for v in vals)
    r = subprocess.run([CLI, "--host-selftest", "format"], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    got = r.stdout.decode().splitlines()
    assert len(got) == len(want)
    bad = [(float.hex(v), g, w) for v, g, w in zip(vals, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    # dst_format_distance, what --nearest / --closest / --mst / --max-distance / --summary, the Newick lengths and the
    # near ties' digits go through
    lib = da.load()
    buf = C.create_string_buffer(64)
    raw = da.MEASURES["raw"]
    bad = []
    for v, w in zip(vals, want):
        n = lib.dst_format_distance(raw, v, 0, buf, 64)
        if buf.value.decode() != w or n != len(w):
            bad.append((float.hex(v), buf.value.decode(), w))
    assert not bad, (len(bad), bad[:5])
