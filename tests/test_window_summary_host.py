"""Host side of dst_window_summary / --window-summary: the symbol, the numpy restatement on cases written out by hand, the
designed hostile set held to its design with the oracle, and the CLI's usage errors before any device is opened.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import random_alignment, to_fasta_bytes
from summary_reference import fixed_point
from window_summary_cases import ALL, F64, hostile_partner, hostile_set, hostile_windows, oracle_window_payloads
from window_summary_reference import assert_window_summary, window_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


# ---- the symbol ------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed():
    assert "dst_window_summary" in da.declared_symbols()
    assert hasattr(da.load(), "dst_window_summary")
    # the prototype of include/distance_hip.h: ctx, measure, square, two slots, two window arrays, n_windows, threshold,
    # totals, three per-record arrays, rec_cap
    assert len(_lib._SIGS["dst_window_summary"][1]) == 14
    header = open(os.path.join(ROOT, "include", "distance_hip.h")).read()
    proto = header[header.index("int dst_window_summary("):]
    assert proto[:proto.index(";")].count(",") + 1 == 14


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_null_context_is_err_arg():
    w = np.zeros(1, np.uint64)
    tot = (_lib.SummaryTotals * 1)()
    assert da.load().dst_window_summary(None, 2, 1, 0, 1, w.ctypes.data, w.ctypes.data, 1, 0.0, tot, None, None, None, 0) == ERR_ARG


# ---- the reference on cases whose answers are written here ---------------------------------------------------------------------
def test_reference_square_by_hand():
    # 3 records, 2 windows; the condensed pairs (0,1) (0,2) (1,2)
    vals = np.array([[0.5, np.nan, 0.25],
                     [-0.0, np.inf, 1.5]])
    got = window_summary("raw", vals, 3, 3, True, 0.5)
    want = {"pairs": np.array([3, 3], np.uint64), "nan_pairs": np.array([1, 0], np.uint64),
            "summable_pairs": np.array([2, 2], np.uint64), "links": np.array([2, 1], np.uint64),
            "total_sum": np.array([0.75, 1.5]),
            # window 0: record 0 has (0,1) = 0.5 and a NaN; record 1 has 0.5 and 0.25; record 2 a NaN and 0.25
            # window 1: record 0 has -0.0 (links at T = 0.5, summable) and +inf (neither); record 1 -0.0 and 1.5; record 2 +inf, 1.5
            "within": np.array([[1, 2, 1], [1, 1, 0]], np.uint32), "summable": np.array([[1, 2, 1], [1, 2, 1]], np.uint32),
            "sum": np.array([[0.5, 0.75, 0.25], [0.0, 1.5, 1.5]])}
    assert_window_summary(got, want)
    assert not np.signbit(got["sum"][1, 0])   # (the integer sum of -0.0 is +0)
    # T = inf links +inf too; T = -1 links nothing
    assert window_summary("raw", vals, 3, 3, True, np.inf)["links"].tolist() == [2, 3]
    assert window_summary("raw", vals, 3, 3, True, -1.0)["links"].tolist() == [0, 0]
    assert not window_summary("raw", vals, 3, 3, True, -1.0)["within"].any()


def test_reference_rectangle_by_hand():
    # 2 rows x 3 columns, 2 windows, n: every pair summable, none NaN; T = 2.9 links v <= 2
    vals = np.array([[0, 3, 2, 5, 1, 2],
                     [4, 4, 4, 0, 0, 0]], np.int64)
    got = window_summary("n", vals, 2, 3, False, 2.9)
    want = {"pairs": np.array([6, 6], np.uint64), "nan_pairs": np.array([0, 0], np.uint64),
            "summable_pairs": np.array([6, 6], np.uint64), "links": np.array([4, 3], np.uint64),
            "total_sum": np.array([13.0, 12.0]),
            "within": np.array([[2, 2], [0, 3]], np.uint32), "summable": np.array([[3, 3], [3, 3]], np.uint32),
            "sum": np.array([[5.0, 8.0], [12.0, 0.0]])}
    assert_window_summary(got, want)
    assert_window_summary(window_summary("n", vals, 2, 3, False, 2), want)   # floor(T)


# ---- the designed hostile set holds what it was designed to hold ------------------------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
def test_hostile_set_is_hostile(measure):
    a, b, windows = hostile_set(), hostile_partner(), hostile_windows()
    assert (a[0] == 240).all() and np.array_equal(a[1], a[2]) and (a[1] != a[3]).all()
    for partner in (None, b):
        vals = oracle_window_payloads(measure, a, partner, windows)
        empty = vals[list(map(tuple, windows.tolist())).index((7, 7))]
        if measure in F64:
            assert np.isnan(empty).all()
            # NaN pairs in a window that is not empty, pairs that are neither NaN nor summable (jc69: p = 0.75 exactly), and
            # a window whose sum of q needs both words
            nan = np.isnan(vals)
            assert nan[0].any() and not nan[0].all(), measure
            ok, q = fixed_point(measure, vals)
            ok, q = ok.reshape(vals.shape), q.reshape(vals.shape)
            if measure == "jc69":
                assert (np.isposinf(vals[0])).any() and (~ok & ~nan)[1:11].any()
            if measure in ("jc69", "k80", "tn93"):
                assert (~ok & ~nan).any(), measure
            assert int(q[0].sum()) > 2 ** 32 and (q.sum(axis=1) > 2 ** 32).sum() >= 3, measure
        else:
            # n / n_high: no NaN exists, every pair is summable, and q is a count of sites: its sum cannot reach 2^32 before
            # pairs x sites does (36 x 40 here), so the two-word sum is met by the f64 measures
            assert not empty.any() and vals[0].max() == 40 and vals.min() == 0
        ref = window_summary(measure, vals, len(a), len(a) if partner is None else len(b), partner is None, 0.5)
        assert ref["pairs"][0] == (36 if partner is None else 45)
        assert 0 < ref["links"][0] < ref["pairs"][0], measure   # the identical records link, the distant ones do not


# ---- the CLI's refusals, before any device is opened -----------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_summary_host")
    codes = random_alignment(3, 40, seed=3)
    fasta = d / "a.fasta"
    fasta.write_bytes(b"".join(b">r%d\n%s\n" % (k, to_fasta_bytes(r)) for k, r in enumerate(codes)))
    good = d / "good.tsv"
    good.write_bytes(b"g1\t1\t40\n\ng2\t7\t7\n")
    bad = d / "bad.tsv"
    bad.write_bytes(b"g1\t1\t41\n")
    return d, str(fasta), str(good), str(bad)


def run_cli(args, stdin=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env, timeout=60)


def test_usage_refusals(files):
    _, fasta, good, _ = files
    mine = "the argument '--window-summary <T>' "
    by = "the argument '--window-summary-by <what>' "
    cases = [
        (["--window-summary", "1"], mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--window-summary", "1", "--step", "2"], mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--windows", "5", "--window-summary", "1", "--window-summary", "1"], mine + "cannot be used multiple times"),
        (["--windows", "5", "--window-summary", "x"], "invalid value 'x' for '--window-summary <T>': not a number"),
        (["--windows", "5", "--window-summary", "nan"], "invalid value 'nan' for '--window-summary <T>': not a number"),
        (["--regions", good, "--window-summary", "-1"],
         "invalid value '-1' for '--window-summary <T>': the threshold must not be negative"),
        (["--window-summary"], "a value is required for '--window-summary <T>' but none was supplied"),
        (["--windows", "5", "--window-summary", "1", "-s", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--regions", good, "--window-summary", "1", "--stream", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--windows", "5", "--window-summary", "1", "--gpus", "2"], mine + "cannot be used with '--gpus <n>' naming more than one GPU"),
        (["--regions", good, "--window-summary", "1", "--devices", "0,1"],
         mine + "cannot be used with '--devices <list>' naming more than one GPU"),
        (["--windows", "5", "--window-summary", "1", "--window-nearest", "2"], mine + "cannot be used with '--window-nearest <K>'"),
        (["--windows", "5", "--window-summary", "1", "--window-closest", "2", "-s", fasta],
         mine + "cannot be used with '--window-closest <K>'"),
        (["--windows", "5", "--window-summary", "1", "--pairs", good], mine + "cannot be used with '--pairs <FILE>'"),
        (["--windows", "5", "--window-summary-by", "record"], by + "requires '--window-summary <T>'"),
        (["--window-summary-by", "window"], by + "requires '--window-summary <T>'"),
        (["--windows", "5", "--window-summary", "1", "--window-summary-by", "pair"],
         "invalid value 'pair' for '--window-summary-by <what>'"),
        (["--window-summary-by"], "a value is required for '--window-summary-by <what>' but none was supplied"),
        # pinned by the earlier host tests and still a usage error
        (["--windows", "5", "--summary", "1"], "the argument '--windows <W>' cannot be used with '--summary <T>'"),
    ]
    others = [["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"], ["--clusters", "1"],
              ["--representatives", "1"], ["--max-distance", "1"], ["--summary", "1"], ["--groups", good], ["--groups-within", "1"],
              ["--per-record"], ["--histogram", "1"], ["--bins", "4"], ["--matrix", "tsv"], ["--tree", "nj"], ["--bootstrap", "2"],
              ["--seed", "2"], ["--mst"], ["--sites"], ["--dendrogram", "average"]]
    for other in others:
        for windows in (["--windows", "5"], ["--regions", good]):
            cases.append((windows + ["--window-summary", "1"] + other, mine + f"cannot be used with '{other[0]}"))
    for args, message in cases:
        r = run_cli(args if args[-1] in ("--window-summary", "--window-summary-by") else args + [fasta])
        first = r.stderr.decode().splitlines()[0]
        assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, first)
        assert first.startswith("error: " + message), (args, first)


@pytest.mark.parametrize("args", [["--windows", "10", "--step", "5", "--window-summary", "2"],
                                  ["--window-summary", "inf", "--regions", None, "-m", "tn93", "--window-summary-by", "record"],
                                  ["--windows", "10", "--window-summary=0.5", "--window-summary-by=window", "-o", "out.tsv"]])
def test_an_accepted_line_ends_at_the_missing_device(files, args):
    d, fasta, good, _ = files
    args = [good if a is None else str(d / a) if a == "out.tsv" else a for a in args]
    r = run_cli(args + [fasta])
    assert r.returncode == 1 and r.stdout == b"" and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args + [fasta, fasta])
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args, stdin=open(fasta, "rb").read())
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr


def test_a_bad_regions_file_ends_the_run_before_the_device(files):
    _, fasta, _, bad = files
    r = run_cli(["--regions", bad, "--window-summary", "1", fasta])
    assert r.returncode != 0 and r.stdout == b"" and b"past the alignment's 40 sites" in r.stderr
    assert b"no MI355X" not in r.stderr


def test_help_names_the_flags():
    r = run_cli(["--help"])
    assert r.returncode == 0 and b"--window-summary <T>" in r.stdout and b"--window-summary-by <what>" in r.stdout
