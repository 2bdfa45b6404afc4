"""GPU (-m gpu): `distance --windows W --step S --window-summary T [--window-summary-by window|record]` and the same with
`--regions FILE`, end to end on a 40-record, 700-site FASTA with ambiguity letters: byte-compared with lines built here from
Engine.window_summary and dst_format_distance, the window fields checked against the plain --windows / --regions run's.  One
and two inputs, stdin, -o."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, LETTERS, random_alignment
from window_reference import sliding

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
BY_WINDOW = "window\tstart\tend\tpairs\tcompared\twithin\tmean"
BY_RECORD = "sequence\twindow\tstart\tend\twithin\tcompared\tmean"
N, NB, L = 40, 5, 700
REGIONS = [("whole", 1, 700), ("orf1", 10, 400), ("spike", 300, 650), ("one", 129, 129), ("orf1", 10, 400), ("tail", 699, 700)]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def write_fasta(path, prefix, codes):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    with open(path, "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">{prefix}{r} description\n" + "".join(lut[int(c)] for c in row) + "\n")


def run(args, stdin=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    a = random_alignment(N, L, seed=77, divergence=0.05, p_ambig=0.03, p_gap=0.02)
    b = random_alignment(NB, L, seed=78, divergence=0.05, p_ambig=0.03, p_gap=0.02, root=a[0])
    d = tmp_path_factory.mktemp("window_summary")
    write_fasta(d / "a.fasta", "a", a)
    write_fasta(d / "b.fasta", "b", b)
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" for name, first, last in REGIONS))
    return {"a": a, "b": b, "dir": d}


def window_fields(plain, nw):
    """(window, start, end) of the plain run's first nw lines: its first pair, every window in the given order"""
    lines = plain.splitlines()[1:1 + nw]
    return ["\t".join(x.split("\t")[2:5]) for x in lines]


def mean_text(total, compared):
    return da.format_distance("raw", total / compared if compared else float("nan"))


def expected(al, measure, windows, threshold, two, fields):
    """both forms' text from Engine.window_summary"""
    with da.Engine(0) as eng:
        eng.upload(0, al["a"])
        if two:
            eng.upload(1, al["b"])
        s = eng.window_summary(measure, np.array(windows, np.uint64), threshold, square=not two)
    by_window = BY_WINDOW + "\n" + "".join(
        f"{fields[w]}\t{int(s['pairs'][w])}\t{int(s['summable_pairs'][w])}\t{int(s['links'][w])}\t"
        f"{mean_text(s['total_sum'][w], int(s['summable_pairs'][w]))}\n" for w in range(len(windows)))
    by_record = BY_RECORD + "\n" + "".join(
        f"a{i}\t{fields[w]}\t{int(s['within'][w, i])}\t{int(s['summable'][w, i])}\t"
        f"{mean_text(s['sum'][w, i], int(s['summable'][w, i]))}\n" for i in range(N) for w in range(len(windows)))
    return by_window, by_record


@pytest.mark.parametrize("measure,threshold", [("n", "4"), ("tn93", "0.05")])
@pytest.mark.parametrize("two", [False, True])
def test_sliding_windows(alignment, measure, threshold, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(int(b), int(e)) for b, e in sliding(L, 100, 50)]
    base = ["--windows", "100", "--step", "50", "-m", measure]
    fields = window_fields(run(base + files), len(windows))
    assert fields[0] == "1\t1\t100" and fields[1] == "2\t51\t150" and len(fields) == len(windows)
    by_window, by_record = expected(alignment, measure, windows, float(threshold), two, fields)
    assert run(base + ["--window-summary", threshold] + files) == by_window
    assert run(base + ["--window-summary", threshold, "--window-summary-by", "window"] + files) == by_window
    assert run(base + ["--window-summary", threshold, "--window-summary-by", "record"] + files) == by_record


@pytest.mark.parametrize("measure,threshold", [("n", "4"), ("tn93", "0.05")])
@pytest.mark.parametrize("two", [False, True])
def test_regions(alignment, measure, threshold, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(first - 1, last) for _, first, last in REGIONS]
    base = ["--regions", str(d / "regions.tsv"), "-m", measure]
    fields = window_fields(run(base + files), len(windows))
    assert fields == [f"{name}\t{first}\t{last}" for name, first, last in REGIONS]
    by_window, by_record = expected(alignment, measure, windows, float(threshold), two, fields)
    assert run(base + ["--window-summary", threshold] + files) == by_window
    assert run(base + ["--window-summary=" + threshold, "--window-summary-by=record"] + files) == by_record


def test_output_file_stdin_and_inf(alignment):
    d = alignment["dir"]
    a = str(d / "a.fasta")
    windows = [(int(x), int(y)) for x, y in sliding(L, 300, 300)]
    base = ["--windows", "300", "-m", "raw", "--window-summary", "inf"]
    fields = window_fields(run(["--windows", "300", "-m", "raw", a]), len(windows))
    by_window, by_record = expected(alignment, "raw", windows, float("inf"), False, fields)
    got = run(base + [a])
    assert got == by_window
    out = d / "out.tsv"
    assert run(base + ["-o", str(out), a]) == "" and out.read_text() == got
    with open(a, "rb") as fh:
        assert run(base + ["--window-summary-by", "record"], stdin=fh) == by_record
    # every compared pair lies within inf
    for line in got.splitlines()[1:]:
        f = line.split("\t")
        assert f[4] == f[5]
