"""Host side of dst_window_group_summary / --window-groups: the symbol, the numpy restatement on cases written out by hand,
the one-group form held to dst_window_summary's reference on the designed hostile set, and the CLI's usage and label-file
errors before any device is opened.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from group_summary_reference import bits
from helpers import random_alignment, to_fasta_bytes
from window_group_summary_reference import WINDOW_GROUPS_MAX, assert_window_group_summary, check_window_consequences, window_group_summary
from window_summary_cases import ALL, hostile_partner, hostile_set, hostile_windows, oracle_window_payloads
from window_summary_reference import window_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


# ---- the symbol ------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed():
    assert "dst_window_group_summary" in da.declared_symbols()
    assert hasattr(da.load(), "dst_window_group_summary")
    # the prototype of include/distance_hip.h: ctx, measure, square, two slots, two window arrays, n_windows, two label
    # arrays with their counts, threshold, cells and their room, three per-record arrays and their room
    assert len(_lib._SIGS["dst_window_group_summary"][1]) == 19
    header = open(os.path.join(ROOT, "include", "distance_hip.h")).read()
    proto = header[header.index("int dst_window_group_summary("):]
    assert proto[:proto.index(";")].count(",") + 1 == 19
    assert "#define DST_WINDOW_GROUPS_MAX 256u" in header
    assert da.WINDOW_GROUPS_MAX == WINDOW_GROUPS_MAX == 256


def test_null_context_is_err_arg():
    w = np.zeros(1, np.uint64)
    g = np.zeros(3, np.uint32)
    cells = (_lib.GroupCell * 1)()
    assert da.load().dst_window_group_summary(None, 2, 1, 0, 1, w.ctypes.data, w.ctypes.data, 1, g.ctypes.data, 1, None, 0, 0.0,
                                              cells, 1, None, None, None, 0) == ERR_ARG


# ---- the reference on cases whose answers are written here ---------------------------------------------------------------------
def test_reference_square_by_hand():
    # 4 records in groups 0, 1, 0 and none; 2 windows; the condensed pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    vals = np.array([[0.5, 0.25, 9.0, NAN, 9.0, 9.0],
                     [-0.0, np.inf, 9.0, 1.5, 9.0, 9.0]])
    got = window_group_summary("raw", vals, 4, 4, True, 0.5, [0, 1, 0, -1], 2)
    u = lambda x: np.array(x, np.uint64)
    want = {
        # cell (0, 0): the pair (0, 2); cells (0, 1) and (1, 0): the pairs (0, 1) and (1, 2); cell (1, 1): one record, no pair
        "pairs": u([[[1, 2], [2, 0]]] * 2),
        "nan_pairs": u([[[0, 1], [1, 0]], [[0, 0], [0, 0]]]),
        "summable_pairs": u([[[1, 1], [1, 0]], [[0, 2], [2, 0]]]),   # (window 1: +inf is neither NaN nor summable)
        "links": u([[[1, 1], [1, 0]], [[0, 1], [1, 0]]]),
        "sum": np.array([[[0.25, 0.5], [0.5, 0.0]], [[0.0, 1.5], [1.5, 0.0]]]),
        "min": np.array([[[0.25, 0.5], [0.5, NAN]], [[np.inf, 0.0], [0.0, NAN]]]),
        "max": np.array([[[0.25, 0.5], [0.5, NAN]], [[np.inf, 1.5], [1.5, NAN]]]),
        # per record and group of the partner; record 3 has a row although it has no group, and is nobody's partner
        "rec_within": np.array([[[1, 1], [1, 0], [1, 0], [0, 0]], [[0, 1], [1, 0], [0, 0], [0, 0]]], np.uint32),
        "rec_summable": np.array([[[1, 1], [1, 0], [1, 0], [2, 1]], [[0, 1], [2, 0], [0, 1], [2, 1]]], np.uint32),
        "rec_sum": np.array([[[0.25, 0.5], [0.5, 0.0], [0.25, 0.0], [18.0, 9.0]], [[0.0, 0.0], [1.5, 0.0], [0.0, 1.5], [18.0, 9.0]]]),
    }
    assert_window_group_summary(got, want)
    assert not np.signbit(got["min"][1, 0, 1])   # (-0.0 comes back from its key as +0.0)
    check_window_consequences(got, [0, 1, 0, -1], True)


def test_reference_rectangle_by_hand():
    # 2 rows (groups 0, 0) x 3 columns (groups 1, 0, none), 2 windows, n; T = 2.9 links v <= 2
    vals = np.array([[0, 3, 2, 5, 1, 2],
                     [4, 4, 4, 0, 0, 0]], np.int64)
    got = window_group_summary("n", vals, 2, 3, False, 2.9, [0, 0], 1, [1, 0, -1], 2)
    u = lambda x: np.array(x, np.uint64)
    want = {"pairs": u([[[2, 2]]] * 2), "nan_pairs": u([[[0, 0]]] * 2), "summable_pairs": u([[[2, 2]]] * 2),
            "links": u([[[1, 1]], [[1, 1]]]), "sum": np.array([[[4.0, 5.0]], [[4.0, 4.0]]]),
            "min": np.array([[[1, 0]], [[0, 0]]], np.int64), "max": np.array([[[3, 5]], [[4, 4]]], np.int64),
            "rec_within": np.array([[[0, 1], [1, 0]], [[0, 0], [1, 1]]], np.uint32),
            "rec_summable": np.array([[[1, 1], [1, 1]]] * 2, np.uint32),
            "rec_sum": np.array([[[3.0, 0.0], [1.0, 5.0]], [[4.0, 4.0], [0.0, 0.0]]])}
    assert_window_group_summary(got, want)
    check_window_consequences(got, [0, 0], False)


# ---- one group with every record assigned is dst_window_summary ------------------------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
def test_one_group_equals_the_window_summary_reference(measure):
    a, b, windows = hostile_set(), hostile_partner(), hostile_windows()
    for partner in (None, b):
        square = partner is None
        n_cols = len(a) if square else len(b)
        vals = oracle_window_payloads(measure, a, partner, windows)
        one = window_group_summary(measure, vals, len(a), n_cols, square, 0.5, np.zeros(len(a), int), 1, np.zeros(n_cols, int), 1)
        ref = window_summary(measure, vals, len(a), n_cols, square, 0.5)
        for cell, total in (("pairs", "pairs"), ("nan_pairs", "nan_pairs"), ("summable_pairs", "summable_pairs"), ("links", "links"),
                            ("sum", "total_sum")):
            assert bits(one[cell][:, 0, 0]).tobytes() == bits(ref[total]).tobytes(), (measure, square, cell)
        for rec, per in (("rec_within", "within"), ("rec_summable", "summable"), ("rec_sum", "sum")):
            assert bits(one[rec][:, :, 0]).tobytes() == bits(ref[per]).tobytes(), (measure, square, rec)


# ---- the CLI's refusals, before any device is opened -----------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_groups_host")
    codes = random_alignment(3, 40, seed=3)
    fasta = d / "a.fasta"
    fasta.write_bytes(b"".join(b">r%d\n%s\n" % (k, to_fasta_bytes(r)) for k, r in enumerate(codes)))
    regions = d / "regions.tsv"
    regions.write_bytes(b"g1\t1\t40\n\ng2\t7\t7\n")
    labels = d / "labels.tsv"
    labels.write_bytes(b"r0\ta\nr1\tb\nr2\ta\n")
    return d, str(fasta), str(regions), str(labels)


def run_cli(args, stdin=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env, timeout=60)


def test_usage_refusals(files):
    _, fasta, regions, labels = files
    mine = "the argument '--window-groups <FILE>' "
    within = "the argument '--window-groups-within <T>' "
    by = "the argument '--window-groups-by <what>' "
    needs = "requires '--windows <W>' or '--regions <FILE>'"
    cases = [
        (["--window-groups", labels], mine + needs),
        (["--window-groups", labels, "--step", "2"], mine + needs),
        (["--windows", "5", "--window-groups", labels, "--window-groups", labels], mine + "cannot be used multiple times"),
        (["--window-groups"], "a value is required for '--window-groups <FILE>' but none was supplied"),
        (["--windows", "5", "--window-groups", labels, "-s", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--regions", regions, "--window-groups", labels, "--stream", fasta], mine + "cannot be used with '--stream <stream>'"),
        (["--windows", "5", "--window-groups", labels, "--gpus", "2"], mine + "cannot be used with '--gpus <n>' naming more than one GPU"),
        (["--regions", regions, "--window-groups", labels, "--devices", "0,1"],
         mine + "cannot be used with '--devices <list>' naming more than one GPU"),
        (["--windows", "5", "--window-groups", labels, "--window-nearest", "2"], mine + "cannot be used with '--window-nearest <K>'"),
        (["--windows", "5", "--window-groups", labels, "--window-closest", "2", "-s", fasta],
         mine + "cannot be used with '--window-closest <K>'"),
        (["--windows", "5", "--window-groups", labels, "--window-summary", "1"], mine + "cannot be used with '--window-summary <T>'"),
        (["--windows", "5", "--window-groups", labels, "--pairs", regions], mine + "cannot be used with '--pairs <FILE>'"),
        (["--windows", "5", "--window-groups-within", "1"], within + "requires '--window-groups <FILE>'"),
        (["--window-groups-within", "1"], within + "requires '--window-groups <FILE>'"),
        (["--windows", "5", "--window-groups", labels, "--window-groups-within", "1", "--window-groups-within", "1"],
         within + "cannot be used multiple times"),
        (["--windows", "5", "--window-groups", labels, "--window-groups-within", "x"],
         "invalid value 'x' for '--window-groups-within <T>': not a number"),
        (["--windows", "5", "--window-groups", labels, "--window-groups-within", "nan"],
         "invalid value 'nan' for '--window-groups-within <T>': not a number"),
        (["--regions", regions, "--window-groups", labels, "--window-groups-within", "-1"],
         "invalid value '-1' for '--window-groups-within <T>': the threshold must not be negative"),
        (["--window-groups-within"], "a value is required for '--window-groups-within <T>' but none was supplied"),
        (["--windows", "5", "--window-groups-by", "record"], by + "requires '--window-groups <FILE>'"),
        (["--window-groups-by", "cell"], by + "requires '--window-groups <FILE>'"),
        (["--windows", "5", "--window-groups", labels, "--window-groups-by", "pair"],
         "invalid value 'pair' for '--window-groups-by <what>'"),
        (["--window-groups-by"], "a value is required for '--window-groups-by <what>' but none was supplied"),
        # pinned by the earlier host tests and still the usage error it was
        (["--windows", "5", "--groups", labels], "the argument '--windows <W>' cannot be used with '--groups <FILE>'"),
        (["--regions", regions, "--groups", labels], "the argument '--regions <FILE>' cannot be used with '--groups <FILE>'"),
    ]
    others = [["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"], ["--clusters", "1"],
              ["--representatives", "1"], ["--max-distance", "1"], ["--summary", "1"], ["--groups", labels], ["--groups-within", "1"],
              ["--per-record"], ["--histogram", "1"], ["--bins", "4"], ["--matrix", "tsv"], ["--tree", "nj"], ["--bootstrap", "2"],
              ["--seed", "2"], ["--mst"], ["--sites"], ["--dendrogram", "average"]]
    for other in others:
        for windows in (["--windows", "5"], ["--regions", regions]):
            cases.append((windows + ["--window-groups", labels] + other, mine + f"cannot be used with '{other[0]}"))
    bare = ("--window-groups", "--window-groups-within", "--window-groups-by")
    for args, message in cases:
        r = run_cli(args if args[-1] in bare else args + [fasta])
        first = r.stderr.decode().splitlines()[0]
        assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, first)
        assert first.startswith("error: " + message), (args, first)


@pytest.mark.parametrize("args", [["--windows", "10", "--step", "5", "--window-groups", "L"],
                                  ["--window-groups", "L", "--regions", "R", "-m", "tn93", "--window-groups-by", "record",
                                   "--window-groups-within", "inf"],
                                  ["--windows", "10", "--window-groups=L", "--window-groups-by=cell", "--window-groups-within=0.5",
                                   "-o", "out.tsv"]])
def test_an_accepted_line_ends_at_the_missing_device(files, args):
    d, fasta, regions, labels = files
    fill = {"L": labels, "R": regions, "out.tsv": str(d / "out.tsv"), "--window-groups=L": "--window-groups=" + labels}
    args = [fill.get(a, a) for a in args]
    r = run_cli(args + [fasta])
    assert r.returncode == 1 and r.stdout == b"" and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args + [fasta, fasta])
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args, stdin=open(fasta, "rb").read())
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr


def test_the_label_file_errors_come_before_the_device(files):
    d, fasta, _, _ = files

    def refused(content, text, inputs=(fasta,)):
        path = d / "bad_labels.tsv"
        path.write_bytes(content)
        r = run_cli(["--windows", "10", "--window-groups", str(path)] + list(inputs))
        err = r.stderr.decode()
        assert r.returncode != 0 and r.stdout == b"" and text in err, (content[:40], err)
        assert "no MI355X" not in err

    refused(b"r0 a\n", "--window-groups: line 1 of")
    refused(b"r0 a\n", "has no tab: expected 'id<TAB>group'")
    refused(b"r0\t\n", "has an empty group")
    refused(b"r0\ta\tb\n", "has more than two fields")
    refused(b"r0\ta\n\nr0\tb\n", "gives 'r0' the group 'b', line 1 gave it 'a'")
    refused(b"x\ta\n", "--window-groups: no record of the first input has a group in")
    r = run_cli(["--windows", "10", "--window-groups", str(d / "absent.tsv"), fasta])
    assert r.returncode != 0 and r.stdout == b"" and b"no MI355X" not in r.stderr
    # more than 256 groups in one input (--groups itself takes 1,024)
    n = WINDOW_GROUPS_MAX + 1
    many = d / "many.fasta"
    many.write_bytes(b"".join(b">s%d\nACGT\n" % k for k in range(n)))
    refused(b"".join(b"s%d\tg%d\n" % (k, k) for k in range(n)),
            "--window-groups: line 257 of", inputs=(str(many),))
    refused(b"".join(b"s%d\tg%d\n" % (k, k) for k in range(n)),
            "starts group 257 of the first input: more than 256 groups", inputs=(str(many),))
    # ... and an id that is in no input is a warning, after which the run goes on to the device
    path = d / "warn.tsv"
    path.write_bytes(b"r0\ta\nr1\tb\nnobody\tc\n")
    r = run_cli(["--windows", "10", "--window-groups", str(path), fasta])
    err = r.stderr.decode()
    assert "warning: --window-groups: 1 ids of" in err and "are not in the input and were skipped" in err
    assert r.returncode == 1 and "no MI355X / HIP device visible" in err


def test_help_names_the_flags():
    r = run_cli(["--help"])
    assert r.returncode == 0
    for flag in (b"--window-groups <FILE>", b"--window-groups-within <T>", b"--window-groups-by <what>"):
        assert flag in r.stdout
