"""GPU (-m gpu): `distance --windows W --step S --window-nearest K` and `--regions FILE --window-nearest K` end to end on a
40-record, 700-site FASTA with ambiguity letters: the output is the lines that Engine.nearest_windows' index picks from the
same CLI's plain --windows / --regions output, per record of the first input, per window, nearest first, the two ids in
the plain line's order (swapped where the neighbour comes first in the file).  One and two inputs, stdin, -o, --slab-pairs."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, LETTERS, random_alignment
from window_reference import pair_index, sliding

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
    d = tmp_path_factory.mktemp("window_nearest")
    write_fasta(d / "a.fasta", "a", a)
    write_fasta(d / "b.fasta", "b", b)
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" for name, first, last in REGIONS))
    return {"a": a, "b": b, "dir": d}


def picked(al, plain, measure, windows, k, two):
    """the lines of the plain run that the engine's index names, in --window-nearest's order"""
    lines = plain.splitlines()
    assert lines[0] == HEADER
    nw = len(windows)
    n_cols = NB if two else N
    i, j = pair_index(not two, N, n_cols)
    where = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(i, j))}
    assert len(lines) == 1 + len(where) * nw
    with da.Engine(0) as eng:
        eng.upload(0, al["a"])
        if two:
            eng.upload(1, al["b"])
        idx, _ = eng.nearest_windows(measure, np.array(windows, np.uint64), k, square=not two)
    out = [HEADER]
    for r in range(N):
        for w in range(nw):
            for c in idx[r, w].tolist():
                pair = (r, c) if two or r < c else (c, r)   # a neighbour before the record: the plain line has it first
                line = lines[1 + where[pair] * nw + w]
                assert line.split("\t")[:2] == [f"a{pair[0]}", f"{'b' if two else 'a'}{pair[1]}"]
                out.append(line)
    return "\n".join(out) + "\n", idx


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
@pytest.mark.parametrize("two", [False, True])
def test_sliding_windows(alignment, measure, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(int(b), int(e)) for b, e in sliding(L, 100, 50)]
    base = ["--windows", "100", "--step", "50", "-m", measure]
    plain = run(base + files)
    got = run(base + ["--window-nearest", "3"] + files)
    want, idx = picked(alignment, plain, measure, windows, 3, two)
    assert got == want
    assert idx.shape == (N, len(windows), 3)
    if not two:
        rows = np.arange(N)[:, None, None]
        assert (idx < rows).any() and (idx > rows).any()   # both orders of the ids occur
    assert run(base + ["--window-nearest", "3", "--slab-pairs", "1"] + files) == got


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
@pytest.mark.parametrize("two", [False, True])
def test_regions(alignment, measure, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(first - 1, last) for _, first, last in REGIONS]
    base = ["--regions", str(d / "regions.tsv"), "-m", measure]
    plain = run(base + files)
    got = run(base + ["--window-nearest", "3"] + files)
    want, _ = picked(alignment, plain, measure, windows, 3, two)
    assert got == want
    names = [x.split("\t")[2] for x in got.splitlines()[1:1 + 3 * len(REGIONS)]]
    assert names == [name for name, _, _ in REGIONS for _ in range(3)]
    assert run(base + ["--window-nearest", "3", "--slab-pairs", "1"] + files) == got


def test_k_above_the_candidates_output_file_and_stdin(alignment):
    d = alignment["dir"]
    a, b = str(d / "a.fasta"), str(d / "b.fasta")
    windows = [(int(x), int(y)) for x, y in sliding(L, 300, 300)]
    base = ["--windows", "300", "-m", "k80", "--window-nearest", "256"]
    got = run(base + [a, b])   # five candidates: all of them, nearest first
    want, idx = picked(alignment, run(["--windows", "300", "-m", "k80", a, b]), "k80", windows, 256, True)
    assert got == want and idx.shape == (N, 3, NB)
    out = d / "out.tsv"
    assert run(base + ["-o", str(out), a, b]) == "" and out.read_text() == got
    with open(a, "rb") as fh:
        one = run(["--windows", "300", "-m", "k80", "--window-nearest", "2"], stdin=fh)
    assert one == run(["--windows", "300", "-m", "k80", "--window-nearest", "2", a])
    assert one == picked(alignment, run(["--windows", "300", "-m", "k80", a]), "k80", windows, 2, False)[0]
