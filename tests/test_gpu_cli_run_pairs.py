"""GPU (-m gpu): `distance --pairs FILE` end to end on a small FASTA with ambiguity letters: every forward line is a line
of the full run, byte for byte, for every -m; reversed lines carry the same value with the ids as given; the order is the
file's; --sites agrees with --max-distance inf --sites; two inputs, -o and stdin."""
import os
import subprocess

import numpy as np
import pytest

from helpers import CODES, LETTERS, random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance"
N, NB, L = 40, 7, 300
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")


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
def inputs(tmp_path_factory):
    codes = random_alignment(N, L, seed=93, divergence=0.02, p_ambig=0.01, p_gap=0.01)
    codes[5] = codes[3]          # identical records
    codes[9, 20], codes[11, 20] = 192, 48   # R against Y
    d = tmp_path_factory.mktemp("run_pairs")
    write_fasta(d / "a.fasta", "a", codes)
    write_fasta(d / "b.fasta", "b", codes[::-1][:NB])
    rng = np.random.default_rng(93)
    row, col = rng.integers(0, N, 150), rng.integers(0, N, 150)
    row[:4], col[:4] = (3, 5, 39, 0), (5, 3, 0, 39)
    keep = row != col
    pairs = list(zip(row[keep].tolist(), col[keep].tolist()))
    with open(d / "pairs.tsv", "w") as fh:
        for k, (i, j) in enumerate(pairs):
            fh.write(f"a{i}\ta{j}\n" + ("\n" if k % 17 == 0 else ""))   # (with empty lines)
    return str(d / "a.fasta"), str(d / "b.fasta"), str(d / "pairs.tsv"), pairs, d


@pytest.mark.parametrize("measure", ALL)
def test_one_file(inputs, measure):
    fa, _, pf, pairs, d = inputs
    full = run(["-m", measure, fa]).splitlines()
    assert full[0] == HEADER
    line_of = {tuple(x.split("\t")[:2]): x for x in full[1:]}
    got = run(["-m", measure, "--pairs", pf, fa]).splitlines()
    assert got[0] == HEADER and len(got) == 1 + len(pairs)
    forward = 0
    for (i, j), line in zip(pairs, got[1:]):          # the file's order
        if i < j:
            assert line == line_of[(f"a{i}", f"a{j}")], (i, j)
            forward += 1
        else:
            want = line_of[(f"a{j}", f"a{i}")].split("\t")[2]
            assert line == f"a{i}\ta{j}\t{want}", (i, j)
    assert 10 < forward < len(pairs) - 10
    assert run(["--pairs", pf, "-m", measure, "--slab-pairs", "50", fa]).splitlines() == got
    if measure in ("n", "tn93"):
        out = d / f"out_{measure}.tsv"
        assert run(["-m", measure, "--pairs", pf, "-o", str(out), fa]) == ""
        assert out.read_text().splitlines() == got
        with open(fa, "rb") as fh:
            assert run(["--pairs", pf, "-m", measure], stdin=fh).splitlines() == got


@pytest.mark.parametrize("measure", ["n", "k80", "tn93"])
def test_sites(inputs, measure):
    fa, _, pf, pairs, _ = inputs
    links = run(["-m", measure, "--max-distance", "inf", "--sites", fa]).splitlines()
    assert links[0] == HEADER + "\tsites"
    line_of = {tuple(x.split("\t")[:2]): x for x in links[1:]}
    plain = run(["-m", measure, "--pairs", pf, fa]).splitlines()
    got = run(["-m", measure, "--pairs", pf, "--sites", fa]).splitlines()
    assert got[0] == HEADER + "\tsites" and len(got) == len(plain)
    shared = 0
    for (i, j), p, g in zip(pairs, plain[1:], got[1:]):
        assert g.rsplit("\t", 1)[0] == p
        if i < j and (f"a{i}", f"a{j}") in line_of:   # (a pair without a distance, NaN, is no link)
            assert g == line_of[(f"a{i}", f"a{j}")], (i, j)
            shared += 1
    assert shared > 10


def test_two_files(inputs):
    fa, fb, _, _, d = inputs
    rng = np.random.default_rng(94)
    pairs = list(zip(rng.integers(0, N, 60).tolist(), rng.integers(0, NB, 60).tolist()))
    with open(d / "pairs_ab.tsv", "w") as fh:
        fh.writelines(f"a{i}\tb{j}\n" for i, j in pairs)
    with open(d / "pairs_ba.tsv", "w") as fh:
        fh.writelines(f"b{j}\ta{i}\n" for i, j in pairs)
    for measure in ("raw", "tn93"):
        for first, second, pf, flip in ((fa, fb, "pairs_ab.tsv", False), (fb, fa, "pairs_ba.tsv", True)):
            full = run(["-m", measure, first, second]).splitlines()
            line_of = {tuple(x.split("\t")[:2]): x for x in full[1:]}
            got = run(["-m", measure, "--pairs", str(d / pf), first, second]).splitlines()
            assert got[0] == HEADER and len(got) == 1 + len(pairs)
            for (i, j), line in zip(pairs, got[1:]):
                assert line == line_of[(f"b{j}", f"a{i}") if flip else (f"a{i}", f"b{j}")], (measure, flip, i, j)
