"""GPU (-m gpu): `distance --windows W [--step S]` and `distance --regions FILE` end to end on a 40-record, 700-site FASTA
with ambiguity letters: the value of every line is the third field of the CLI's own long output on the FASTA cut to the
window's columns; the ids, the window / start / end fields and the line order are the specified ones.  One and two
inputs, stdin, -o, every -m, --slab-pairs."""
import os
import subprocess

import pytest

from helpers import CODES, LETTERS, random_alignment
from window_reference import ALL, sliding

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\twindow\tstart\tend\tdistance"
N, NB, L = 40, 5, 700
REGIONS = [("whole", 1, 700), ("orf1", 10, 400), ("spike", 300, 650), ("one", 129, 129), ("orf1", 10, 400), ("tail", 699, 700)]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def write_fasta(path, prefix, codes, lo=0, hi=None):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    with open(path, "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">{prefix}{r} description\n" + "".join(lut[int(c)] for c in row[lo:hi]) + "\n")


def run(args, stdin=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    a = random_alignment(N, L, seed=77, divergence=0.05, p_ambig=0.03, p_gap=0.02)
    b = random_alignment(NB, L, seed=78, divergence=0.05, p_ambig=0.03, p_gap=0.02, root=a[0])
    d = tmp_path_factory.mktemp("windows")
    write_fasta(d / "a.fasta", "a", a)
    write_fasta(d / "b.fasta", "b", b)
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" + ("\n" if k == 1 else "") for k, (name, first, last) in enumerate(REGIONS)))
    return {"a": a, "b": b, "dir": d, "cut": {}}


def cut_values(al, measure, lo, hi, two):
    """the third fields (and the ids) of the long output on the inputs cut to columns [lo, hi)"""
    key = (measure, lo, hi, two)
    if key not in al["cut"]:
        d = al["dir"]
        write_fasta(d / "cut_a.fasta", "a", al["a"], lo, hi)
        files = [str(d / "cut_a.fasta")]
        if two:
            write_fasta(d / "cut_b.fasta", "b", al["b"], lo, hi)
            files.append(str(d / "cut_b.fasta"))
        lines = run(["-m", measure] + files).splitlines()
        assert lines[0] == "sequence1\tsequence2\tdistance"
        al["cut"][key] = [x.split("\t") for x in lines[1:]]
    return al["cut"][key]


def check(al, text, measure, windows, two):
    """windows: (name, 0-based begin, end).  Per pair in the long output's order, per window in the given order."""
    lines = text.splitlines()
    assert lines[0] == HEADER
    pairs = N * NB if two else N * (N - 1) // 2
    assert len(lines) == 1 + pairs * len(windows)
    for w, (name, lo, hi) in enumerate(windows):
        cut = cut_values(al, measure, lo, hi, two)
        assert len(cut) == pairs
        for p in range(pairs):
            got = lines[1 + p * len(windows) + w].split("\t")
            assert got == [cut[p][0], cut[p][1], name, str(lo + 1), str(hi), cut[p][2]], (measure, name, p, got)


@pytest.mark.parametrize("measure", ALL)
def test_sliding_windows_every_measure(alignment, measure):
    windows = [(str(k + 1), int(b), int(e)) for k, (b, e) in enumerate(sliding(L, 128, 50))]
    assert len(windows) == 13 and windows[-1][1:] == (600, 700)
    check(alignment, run(["--windows", "128", "--step", "50", "-m", measure, str(alignment["dir"] / "a.fasta")]), measure, windows,
          False)


def test_one_window_and_the_default_step(alignment):
    a = str(alignment["dir"] / "a.fasta")
    text = run(["--windows", "1000", a])   # one window, cut at the width: the long output with three more fields
    check(alignment, text, "raw", [("1", 0, 700)], False)
    long_form = run([a]).splitlines()
    assert [x.split("\t")[::5] for x in text.splitlines()[1:]] == [x.split("\t")[::2] for x in long_form[1:]]
    windows = [(str(k + 1), int(b), int(e)) for k, (b, e) in enumerate(sliding(L, 300, 300))]   # --step defaults to W
    assert [w[1:] for w in windows] == [(0, 300), (300, 600), (600, 700)]
    check(alignment, run(["--windows", "300", "-m", "k80", a]), "k80", windows, False)


@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_regions_two_inputs_stdin_and_output_file(alignment, measure):
    d = alignment["dir"]
    a, b, regions = str(d / "a.fasta"), str(d / "b.fasta"), str(d / "regions.tsv")
    windows = [(name, first - 1, last) for name, first, last in REGIONS]
    two = run(["--regions", regions, "-m", measure, a, b])
    check(alignment, two, measure, windows, True)
    one = run(["--regions", regions, "-m", measure, a])
    check(alignment, one, measure, windows, False)
    with open(a, "rb") as fh:
        assert run(["--regions", regions, "-m", measure], stdin=fh) == one
    out = d / f"out_{measure}.tsv"
    assert run(["--regions", regions, "-m", measure, "-o", str(out), a, b]) == ""
    assert out.read_text() == two


@pytest.mark.parametrize("measure", ["raw", "tn93"])
def test_slab_pairs_bound_does_not_change_the_output(alignment, measure):
    d = alignment["dir"]
    a, b = str(d / "a.fasta"), str(d / "b.fasta")
    for files in ([a], [a, b]):
        want = run(["--windows", "128", "--step", "50", "-m", measure] + files)
        for bound in ("7", "500"):   # fewer pair-windows than one row has (a row per call), and a few rows per call
            assert run(["--windows", "128", "--step", "50", "-m", measure, "--slab-pairs", bound] + files) == want, (bound, files)
    check(alignment, want, measure, [(str(k + 1), int(b_), int(e_)) for k, (b_, e_) in enumerate(sliding(L, 128, 50))], True)
