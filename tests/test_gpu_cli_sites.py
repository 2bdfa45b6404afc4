"""GPU (-m gpu): `distance --max-distance T --sites` and `distance --mst --sites` end to end on a small FASTA with
ambiguity letters: the first three fields are the run's without --sites, the fourth is the reference's sites rendered with
the letter map; one and two inputs, -o and stdin."""
import os
import subprocess

import numpy as np
import pytest

from helpers import CODES, LETTERS, random_alignment
from pair_sites_reference import expected, render

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance\n"
SITES_HEADER = "sequence1\tsequence2\tdistance\tsites\n"
N, NB, L = 60, 9, 300


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
    codes = random_alignment(N, L, seed=91, divergence=0.004, p_ambig=0.004, p_gap=0.004)
    codes[5] = codes[3]          # identical records: a line without sites
    codes[7] = codes[3]
    codes[7, 10] = 240           # N against a base: distance 0 and no site either
    codes[11] = codes[9]
    codes[9, 20], codes[11, 20] = 192, 48   # R against Y: a site of n, raw and k80, not of tn93
    d = tmp_path_factory.mktemp("sites")
    write_fasta(d / "a.fasta", "a", codes)
    write_fasta(d / "b.fasta", "b", codes[:NB])
    return codes, str(d / "a.fasta"), str(d / "b.fasta")


def check(plain, with_sites, measure, row_codes, col_codes, row_prefix, col_prefix):
    """every line of with_sites = the line of plain + the reference's field; returns the fourth fields"""
    plain, got = plain.splitlines(), with_sites.splitlines()
    assert plain[0] + "\n" == HEADER and got[0] + "\n" == SITES_HEADER and len(plain) == len(got) > 3
    row = [int(x.split("\t")[0][len(row_prefix):]) for x in plain[1:]]
    col = [int(x.split("\t")[1][len(col_prefix):]) for x in plain[1:]]
    off, sites, bases = expected(measure, row_codes, col_codes, row, col)
    fields = []
    for k, (p, g) in enumerate(zip(plain[1:], got[1:])):
        assert g.rsplit("\t", 1)[0] == p, (k, p, g)
        fields.append(g.rsplit("\t", 1)[1])
        assert fields[-1] == render(sites, bases, off[k], off[k + 1]), (k, g)
    return fields


@pytest.mark.parametrize("measure", ["n", "raw", "k80", "tn93"])
def test_max_distance_one_file(alignment, tmp_path, measure):
    codes, fa, _ = alignment
    t = "3" if measure == "n" else "0.011"
    plain = run(["-m", measure, "--max-distance", t, fa])
    got = run(["-m", measure, "--max-distance", t, "--sites", fa])
    fields = check(plain, got, measure, codes, codes, "a", "a")
    assert "." in fields and any("," in f for f in fields)
    assert run(["--sites", "-m", measure, f"--max-distance={t}", "--slab-pairs", "7", fa]) == got
    if measure == "n":
        assert any("R21Y" in f for f in fields)
        out = tmp_path / "sites.tsv"
        assert run(["-m", measure, "--max-distance", t, "--sites", "-o", str(out), fa]) == ""
        assert out.read_text() == got
        with open(fa, "rb") as fh:
            assert run(["--max-distance", t, "-m", measure, "--sites"], stdin=fh) == got
    if measure == "tn93":
        assert not any("R21Y" in f for f in fields)


def test_max_distance_two_files(alignment):
    codes, fa, fb = alignment
    for first, second, rc, cc, rp, cp in ((fa, fb, codes, codes[:NB], "a", "b"), (fb, fa, codes[:NB], codes, "b", "a")):
        plain = run(["-m", "n_high", "--max-distance", "3", first, second])
        got = run(["-m", "n_high", "--max-distance", "3", "--sites", first, second])
        fields = check(plain, got, "n_high", rc, cc, rp, cp)
        assert "." in fields and len(fields) > NB


@pytest.mark.parametrize("measure", ["n", "jc69", "tn93"])
def test_mst(alignment, tmp_path, measure):
    codes, fa, _ = alignment
    plain = run(["-m", measure, "--mst", fa])
    got = run(["-m", measure, "--mst", "--sites", fa])
    fields = check(plain, got, measure, codes, codes, "a", "a")
    assert len(fields) == N - 1 and "." in fields and any(f != "." for f in fields)
    out = tmp_path / "mst.tsv"
    assert run(["-m", measure, "--sites", "--mst", "-o", str(out), fa]) == ""
    assert out.read_text() == got
    with open(fa, "rb") as fh:
        assert run(["--mst", "-m", measure, "--sites"], stdin=fh) == got
