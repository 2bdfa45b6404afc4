"""CPU: the host side of the per-window distances: dst_sliding_windows against its restatement, the four symbols
(declared, exported, typed), the ABI version, the additivity of the reference over a partition of the columns, and the
usage and --regions file errors of `distance --windows / --regions` (no device is opened for any of them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distance_amd as da
import oracle
from distance_amd import _lib
from helpers import random_alignment, to_fasta_bytes
from window_reference import ALL, WIDTH, expected_counts, expected_tallies, sliding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG, ERR_CAPACITY = 1, 6


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


# ---- dst_sliding_windows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0, 1, 7, 128, 1000])
def test_sliding_windows_against_the_restatement(length):
    lib = da.load()
    for width in (1, 2, 7, 128, 1000, 1001):
        for step in (1, 2, 7, 128, 1000, 1001):
            want = sliding(length, width, step)
            got = da.sliding_windows(length, width, step)
            assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (length, width, step)
            count = C.c_uint32(77)
            assert lib.dst_sliding_windows(length, width, step, None, None, 0, C.byref(count)) == 0
            assert count.value == len(want)
            assert (want[:, 0] < want[:, 1]).all() and (want[:-1, 1] < length).all()   # none empty, none ends early but the last
            if len(want):
                assert int(want[-1, 1]) == length or step > width   # (a step above the width can skip the end)
                b, e = np.zeros(len(want), np.uint64), np.zeros(len(want), np.uint64)
                rc = lib.dst_sliding_windows(length, width, step, b.ctypes.data, e.ctypes.data, len(want) - 1, C.byref(count))
                assert rc == ERR_CAPACITY and count.value == len(want)


def test_sliding_windows_errors():
    lib = da.load()
    count = C.c_uint32(5)
    one = np.zeros(1, np.uint64)
    assert lib.dst_sliding_windows(10, 0, 1, None, None, 0, C.byref(count)) == ERR_ARG and count.value == 0
    assert lib.dst_sliding_windows(10, 1, 0, None, None, 0, C.byref(count)) == ERR_ARG
    assert lib.dst_sliding_windows(10, 1, 1, None, None, 0, None) == ERR_ARG
    assert lib.dst_sliding_windows(10, 1, 1, one.ctypes.data, None, 1, C.byref(count)) == ERR_ARG
    # exactly the maximum is fine, one more is not; *count says how many it would take
    assert lib.dst_sliding_windows(da.WINDOWS_MAX, 1, 1, None, None, 0, C.byref(count)) == 0 and count.value == da.WINDOWS_MAX
    assert lib.dst_sliding_windows(da.WINDOWS_MAX + 1, 1, 1, None, None, 0, C.byref(count)) == ERR_CAPACITY
    assert count.value == da.WINDOWS_MAX + 1
    assert lib.dst_sliding_windows(2 ** 63, 1, 1, None, None, 0, C.byref(count)) == ERR_CAPACITY and count.value == 2 ** 32 - 1
    assert lib.dst_sliding_windows(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, None, None, 0, C.byref(count)) == 0 and count.value == 1
    assert lib.dst_sliding_windows(2 ** 64 - 1, 5, 2 ** 64 - 2, None, None, 0, C.byref(count)) == 0 and count.value == 2
    assert lib.dst_sliding_windows(2 ** 64 - 1, 5, 2 ** 64 - 1, None, None, 0, C.byref(count)) == 0 and count.value == 1
    with pytest.raises(da.DistanceError) as e:
        da.sliding_windows(10, 0, 3)
    assert e.value.status == ERR_ARG


# ---- the symbols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_args", [("dst_run_windows", 14), ("dst_run_windows_host", 13), ("dst_window_base_counts", 7),
                                         ("dst_sliding_windows", 7)])
def test_declared_exported_and_typed(name, n_args):
    assert name in da.declared_symbols()
    assert hasattr(da.load(), name)
    assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_constant_matches_header():
    m = re.search(r"#define\s+DST_WINDOWS_MAX\s+(\d+)u", open(_lib.HEADER_PATH).read())
    assert m and int(m.group(1)) == da.WINDOWS_MAX == _lib.WINDOWS_MAX == 65536


def test_null_context_is_err_arg():
    lib = da.load()
    w = np.zeros(1, np.uint64)
    out = np.zeros(16, np.uint32)
    assert lib.dst_run_windows(None, 2, 1, 0, 1, 0, 1, w.ctypes.data, w.ctypes.data, 1, 1, out.ctypes.data, 64, None) == ERR_ARG
    assert lib.dst_run_windows_host(None, 2, 1, 0, 1, 0, 1, w.ctypes.data, w.ctypes.data, 1, 1, out.ctypes.data, 64) == ERR_ARG
    assert lib.dst_window_base_counts(None, 0, w.ctypes.data, w.ctypes.data, 1, out.ctypes.data, 16) == ERR_ARG


# ---- the reference itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
def test_reference_is_additive_over_a_partition(measure):
    a, b = random_alignment(5, 301, seed=11, p_ambig=0.1, p_gap=0.1, divergence=0.3), random_alignment(4, 301, seed=12, p_ambig=0.1)
    cuts = [0, 1, 32, 33, 128, 128, 200, 301]   # (with one empty piece)
    windows = np.array(list(zip(cuts[:-1], cuts[1:])), np.uint64)
    whole = oracle.tallies_rect(measure, a, b)[:, :, :WIDTH[measure]].reshape(20, -1)
    parts = expected_tallies(measure, a, b, windows)
    assert parts.shape == (7, 20, WIDTH[measure]) and not parts[4].any()
    assert np.array_equal(parts.astype(np.uint64).sum(axis=0), whole)
    sq = expected_tallies(measure, a, None, windows, square=True, rb=1, re=4)
    i, j = np.triu_indices(5, 1)
    keep = (i >= 1) & (i < 4)
    want = oracle.tallies_rect(measure, a, a)[i[keep], j[keep], :WIDTH[measure]]
    assert np.array_equal(sq.astype(np.uint64).sum(axis=0), want)
    counts = expected_counts(a, windows)
    assert np.array_equal(counts.astype(np.uint64).sum(axis=0), oracle.count_bases_matrix(a))


# ---- the CLI's refusals, before any device is opened -----------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("windows_host")
    codes = random_alignment(3, 40, seed=3)
    fasta = d / "a.fasta"
    fasta.write_bytes(b"".join(b">r%d\n%s\n" % (k, to_fasta_bytes(r)) for k, r in enumerate(codes)))
    good = d / "good.tsv"
    good.write_bytes(b"g1\t1\t40\n\ng2\t7\t7\n")
    return d, str(fasta), str(good)


def run_cli(args, stdin=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env, timeout=60)


def test_usage_refusals(files):
    _, fasta, good = files
    cases = [
        (["--step", "3"], "the argument '--step <S>' requires '--windows <W>'"),
        (["--step", "3", "--regions", good], "the argument '--step <S>' requires '--windows <W>'"),
        (["--windows", "5", "--regions", good], "the argument '--windows <W>' cannot be used with '--regions <FILE>'"),
        (["--windows", "5", "--windows", "6"], "the argument '--windows <W>' cannot be used multiple times"),
        (["--regions", good, "--regions", good], "the argument '--regions <FILE>' cannot be used multiple times"),
        (["--windows", "5", "--step", "1", "--step", "2"], "the argument '--step <S>' cannot be used multiple times"),
        (["--windows", "0"], "invalid value '0' for '--windows <W>'"),
        (["--windows", "x"], "invalid value 'x' for '--windows <W>'"),
        (["--windows", "-1"], "invalid value '-1' for '--windows <W>'"),
        (["--windows", "5", "--step", "0"], "invalid value '0' for '--step <S>'"),
        (["--windows", "5", "-s", fasta], "the argument '--windows <W>' cannot be used with '--stream <stream>'"),
        (["--regions", good, "--stream", fasta], "the argument '--regions <FILE>' cannot be used with '--stream <stream>'"),
        (["--windows", "5", "--gpus", "2"], "the argument '--windows <W>' cannot be used with '--gpus <n>' naming more than one GPU"),
        (["--regions", good, "--devices", "0,1"],
         "the argument '--regions <FILE>' cannot be used with '--devices <list>' naming more than one GPU"),
    ]
    others = [["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"], ["--clusters", "1"],
              ["--representatives", "1"], ["--max-distance", "1"], ["--summary", "1"], ["--groups", good], ["--groups-within", "1"],
              ["--per-record"], ["--histogram", "1"], ["--bins", "4"], ["--matrix", "tsv"], ["--tree", "nj"], ["--bootstrap", "2"],
              ["--seed", "2"], ["--mst"], ["--sites"], ["--dendrogram", "average"]]
    for other in others:
        for mine, shown in ((["--windows", "5"], "--windows <W>"), (["--regions", good], "--regions <FILE>")):
            cases.append((mine + other, f"the argument '{shown}' cannot be used with '{other[0]}"))
    for args, message in cases:
        r = run_cli(args + [fasta])
        first = r.stderr.decode().splitlines()[0]
        assert r.returncode == 2 and r.stdout == b"" and first.startswith("error: " + message), (args, r.returncode, first)


def test_regions_file_errors(files):
    d, fasta, _ = files
    cases = [
        (b"g1\t1\n", "line 1 of", "fewer than three fields"),
        (b"g1\t1\t2\n\nno tabs here\n", "line 3 of", "fewer than three fields"),
        (b"g1\t1\t2\t3\n", "line 1 of", "more than three fields"),
        (b"\t1\t2\n", "line 1 of", "empty name"),
        (b"g1\t1\t2\ng2\tx\t2\n", "line 2 of", "not a whole number"),
        (b"g1\t1\t-2\n", "line 1 of", "not a whole number"),
        (b"g1\t0\t2\n", "line 1 of", "1 <= start <= end"),
        (b"g1\t5\t4\n", "line 1 of", "1 <= start <= end"),
        (b"g1\t1\t40\ng2\t40\t41\n", "line 2 of", "past the alignment's 40 sites"),
        (b"\n\n", "", "names no region"),
        (b"", "", "names no region"),
        (b"".join(b"r%d\t1\t1\n" % k for k in range(65537)), "line 65537 of", "more than 65536 regions"),
    ]
    for k, (text, where, what) in enumerate(cases):
        path = d / f"bad{k}.tsv"
        path.write_bytes(text)
        r = run_cli(["--regions", str(path), fasta])
        err = r.stderr.decode()
        assert r.returncode == 1 and r.stdout == b"", (text[:30], r.returncode, err)
        assert err.startswith('Error: Message("--regions: ') and where in err and what in err, (text[:30], err)
    r = run_cli(["--regions", str(d / "missing.tsv"), fasta])
    assert r.returncode == 1 and b"NotFound" in r.stderr


def test_more_windows_than_the_maximum_is_an_error_before_the_device(files):
    d, _, _ = files
    wide = d / "wide.fasta"
    wide.write_bytes(b">a\n" + b"A" * 65537 + b"\n>b\n" + b"C" * 65537 + b"\n")
    r = run_cli(["--windows", "1", str(wide)])
    assert r.returncode == 1 and r.stdout == b"" and b"65537 windows, more than 65536" in r.stderr
    r = run_cli(["--windows", "1", "--step", "2", str(wide)])   # 32,769 windows: accepted, and then there is no device
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
