"""Host side of dst_nearest_windows / --window-nearest: the symbol, the numpy restatement on a case written out by hand,
and the CLI's usage errors before any device is opened.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import random_alignment, to_fasta_bytes
from window_nearest_reference import full_rect, full_square, keys, nearest, oracle_payloads, take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


# ---- the symbol ------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed():
    assert "dst_nearest_windows" in da.declared_symbols()
    assert hasattr(da.load(), "dst_nearest_windows")
    assert len(_lib._SIGS["dst_nearest_windows"][1]) == 17


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_null_context_is_err_arg():
    w = np.zeros(1, np.uint64)
    idx = np.zeros(4, np.uint32)
    ku = np.zeros(1, np.uint32)
    assert da.load().dst_nearest_windows(None, 2, 1, 0, 1, 0, 1, w.ctypes.data, w.ctypes.data, 1, 1, 0, idx.ctypes.data, None, None, 4,
                                         ku.ctypes.data_as(_lib._u32p)) == ERR_ARG


# ---- the reference on a case whose answer is written here ----------------------------------------------------------------------
def test_reference_rectangle_by_hand():
    # 2 windows x 3 rows x 4 columns
    p = np.array([[[3, 1, 2, 1],      # window 0, row 0: 1 (col 1) = 1 (col 3) < 2 < 3
                   [0, 0, 0, 0],      #           row 1: all equal -> index order
                   [5, 4, 9, 4]],     #           row 2: 4 (col 1) = 4 (col 3) < 5 < 9
                  [[7, 7, 7, 6],      # window 1
                   [2, 9, 1, 3],
                   [-1, 0, -2, 8]]], np.int64)
    want3 = [[[1, 3, 2], [3, 0, 1]],
             [[0, 1, 2], [2, 0, 3]],
             [[1, 3, 0], [2, 0, 1]]]
    got = nearest(p, 3)
    assert got.dtype == np.uint32 and got.shape == (3, 2, 3) and got.tolist() == want3
    assert nearest(p, 1).tolist() == [[[1], [3]], [[0], [2]], [[1], [2]]]
    assert nearest(p, 9).shape == (3, 2, 4) and nearest(p, 9)[0, 0].tolist() == [1, 3, 2, 0]
    assert take(p, got).tolist() == [[[1, 1, 2], [6, 7, 7]], [[0, 0, 0], [1, 2, 3]], [[4, 4, 5], [-2, -1, 0]]]
    # rows 1 .. 2 only, from the same payloads
    assert nearest(p[:, 1:], 3).tolist() == want3[1:]


def test_reference_square_by_hand():
    # 4 records, 2 windows; the condensed pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    cond = np.array([[0.5, 0.25, 0.5, np.nan, 0.0, 0.25],
                     [-0.0, 0.0, 1.0, np.inf, np.nan, 2.0]])
    full = full_square(cond, 4)
    assert full.shape == (2, 4, 4) and full[0, 2, 0] == 0.25 and full[0, 3, 1] == 0.0 and np.isnan(full[0, 2, 1])
    got = nearest(full, 3, square=True)
    # window 0: record 0: 0.25 (2) < 0.5 (1) = 0.5 (3); record 1: 0.0 (3) < 0.5 (0) < NaN (2); record 2: 0.25 (0) = 0.25 (3) <
    # NaN (1); record 3: 0.0 (1) < 0.25 (2) < 0.5 (0).  window 1: -0.0 ties with +0.0 (index order), NaN after +inf.
    assert got.tolist() == [[[2, 1, 3], [1, 2, 3]],
                            [[3, 0, 2], [0, 2, 3]],
                            [[0, 3, 1], [0, 3, 1]],
                            [[1, 2, 0], [0, 2, 1]]]
    # the swap: record 3's neighbour 1 is the canonical pair (1, 3), condensed entry 4
    vals = take(full, got)
    assert vals[3, 0, 0] == cond[0, 4] and vals[2, 0, 0] == cond[0, 1] and np.isnan(vals[1, 0, 2])
    # a row range reads the same rows
    part = nearest(full[:, 2:4], 2, square=True, row_begin=2)
    assert part.tolist() == [[[0, 3], [0, 3]], [[1, 2], [0, 2]]]
    assert np.array_equal(take(full, part, row_begin=2), vals[2:4, :, :2], equal_nan=True)
    # one record: no candidate
    assert nearest(np.zeros((2, 1, 1)), 3, square=True).shape == (1, 2, 0)


def test_reference_keys():
    v = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf])
    k = keys(v)
    assert k[3] == k[4] and list(np.argsort(k, kind="stable")) == [6, 5, 3, 4, 2, 1, 0]
    assert list(np.argsort(keys(np.array([3, -1, 0, -(2 ** 63), 2 ** 63 - 1], np.int64)))) == [3, 1, 2, 0, 4]


def test_reference_oracle_payloads():
    a, b = random_alignment(3, 60, seed=1), random_alignment(4, 60, seed=2)
    windows = np.array([(0, 60), (5, 5), (10, 30)], np.uint64)
    n = oracle_payloads("n", a, b, windows)
    assert n.dtype == np.int64 and n.shape == (3, 3, 4) and not n[1].any() and (n[2] <= n[0]).all()
    r = oracle_payloads("raw", a, None, windows, square=True)
    assert r.shape == (3, 3, 3) and np.isnan(r[1]).all() and np.array_equal(r[0], r[0].T)
    assert full_rect(n.reshape(3, 12), 3, 4).shape == (3, 3, 4)


# ---- the CLI's refusals, before any device is opened -----------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_nearest_host")
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
    mine = "the argument '--window-nearest <K>' "
    cases = [
        (["--window-nearest", "3"], mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--window-nearest", "3", "--step", "2"], mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--windows", "5", "--window-nearest", "3", "--window-nearest", "3"], mine + "cannot be used multiple times"),
        (["--windows", "5", "--window-nearest", "0"], "invalid value '0' for '--window-nearest <K>': 0 is not in 1..=256"),
        (["--windows", "5", "--window-nearest", "257"], "invalid value '257' for '--window-nearest <K>': 257 is not in 1..=256"),
        (["--regions", good, "--window-nearest", "x"], "invalid value 'x' for '--window-nearest <K>'"),
        (["--windows", "5", "--window-nearest", "-1"], "invalid value '-1' for '--window-nearest <K>'"),
        (["--windows", "5", "--window-nearest", "3", "-s", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--regions", good, "--window-nearest", "3", "--stream", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--windows", "5", "--window-nearest", "3", "--gpus", "2"], mine + "cannot be used with '--gpus <n>' naming more than one GPU"),
        (["--regions", good, "--window-nearest", "3", "--devices", "0,1"],
         mine + "cannot be used with '--devices <list>' naming more than one GPU"),
        (["--window-nearest"], "a value is required for '--window-nearest <K>' but none was supplied"),
        # pinned by tests/test_windows_host.py and still a usage error
        (["--windows", "5", "--nearest", "3"], "the argument '--windows <W>' cannot be used with '--nearest <k>'"),
    ]
    others = [["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"], ["--clusters", "1"],
              ["--representatives", "1"], ["--max-distance", "1"], ["--summary", "1"], ["--groups", good], ["--groups-within", "1"],
              ["--per-record"], ["--histogram", "1"], ["--bins", "4"], ["--matrix", "tsv"], ["--tree", "nj"], ["--bootstrap", "2"],
              ["--seed", "2"], ["--mst"], ["--sites"], ["--dendrogram", "average"]]
    for other in others:
        for windows in (["--windows", "5"], ["--regions", good]):
            cases.append((windows + ["--window-nearest", "3"] + other, mine + f"cannot be used with '{other[0]}"))
    for args, message in cases:
        r = run_cli(args if args == ["--window-nearest"] else args + [fasta])
        first = r.stderr.decode().splitlines()[0]
        assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, first)
        assert first.startswith("error: " + message), (args, first)


@pytest.mark.parametrize("args", [["--windows", "10", "--step", "5", "--window-nearest", "2"],
                                  ["--window-nearest", "256", "--regions", None, "-m", "tn93"],
                                  ["--windows", "10", "--window-nearest=1", "--slab-pairs", "1", "-o", "out.tsv"]])
def test_an_accepted_line_ends_at_the_missing_device(files, args):
    d, fasta, good = files
    args = [good if a is None else str(d / a) if a == "out.tsv" else a for a in args]
    r = run_cli(args + [fasta])
    assert r.returncode == 1 and r.stdout == b"" and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args + [fasta, fasta])
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args, stdin=open(fasta, "rb").read())
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr


def test_help_names_the_flag():
    r = run_cli(["--help"])
    assert r.returncode == 0 and b"--window-nearest <K>" in r.stdout
