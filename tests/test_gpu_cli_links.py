"""GPU (-m gpu): `distance --max-distance T` end to end — the header and exactly those lines of the full run whose pair is
a link, byte for byte and in the full run's order: every measure, two inputs, -o, stdin, any slab bound, T = inf (the
full output) and T = 0 on a set without duplicates (the header only)."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, LETTERS, random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance\n"
N = 200


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
    codes = random_alignment(N, 500, seed=83)
    codes[5] = codes[3]   # identical records: links at 0
    codes[150] = codes[3]
    d = tmp_path_factory.mktemp("links")
    write_fasta(d / "a.fasta", "a", codes)
    write_fasta(d / "b.fasta", "b", codes[:23])
    return codes, str(d / "a.fasta"), str(d / "b.fasta")


@pytest.mark.parametrize("measure", ["n", "n_high", "raw", "jc69", "k80", "tn93"])
def test_output_is_the_full_output_filtered(alignment, tmp_path, measure):
    codes, fasta, _ = alignment
    full = run(["-m", measure, fasta]).splitlines(keepends=True)
    assert full[0] == HEADER and len(full) == 1 + N * (N - 1) // 2
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square(measure)
        if measure in da.INT_MEASURES:
            t = float(np.quantile(vals, 0.03))
            keep = [k for k, line in enumerate(full[1:]) if int(line.rstrip("\n").split("\t")[2]) <= t]
            text = str(int(t))
        else:
            t = float(np.quantile(vals[np.isfinite(vals)], 0.03))
            text = repr(t)   # (the shortest text that reads back as t)
            row, col = eng.links(measure, float(text), values=False)
            keep = (row.astype(np.int64) * (2 * N - row - 1) // 2 + (col.astype(np.int64) - row - 1)).tolist()
    assert 3 <= len(keep) < len(full) - 1
    want = HEADER + "".join(full[1 + k] for k in keep)
    assert run(["-m", measure, "--max-distance", text, fasta]) == want
    assert run(["-m", measure, f"--max-distance={text}", "--slab-pairs", "1", "-t", "2", fasta]) == want
    if measure in ("n", "tn93"):
        out = tmp_path / "links.tsv"
        assert run(["-m", measure, "--max-distance", text, "-o", str(out), fasta]) == ""
        assert out.read_text() == want
        with open(fasta, "rb") as fh:
            assert run(["--max-distance", text, "-m", measure], stdin=fh) == want
        assert run(["-m", measure, "--max-distance", "inf", fasta]) == "".join(
            line for line in full if not line.endswith("\tNaN\n"))


def test_two_inputs(alignment):
    codes, fa, fb = alignment
    for first, second, nr, nc in ((fa, fb, N, 23), (fb, fa, 23, N)):
        full = run(["-m", "n_high", first, second]).splitlines(keepends=True)
        assert len(full) == 1 + nr * nc
        want = HEADER + "".join(line for line in full[1:] if int(line.rstrip("\n").split("\t")[2]) <= 40)
        got = run(["-m", "n_high", "--max-distance", "40.5", first, second])
        assert got == want and HEADER != want != "".join(full)
        assert run(["-m", "n_high", "--max-distance", "40", "--slab-pairs", "100", "-i", first, second]) == want
    full = run(["-m", "tn93", fb, fa])
    assert run(["-m", "tn93", "--max-distance", "inf", fb, fa]) == full and "NaN" not in full


def test_zero_without_duplicates(tmp_path):
    codes = random_alignment(40, 300, seed=84)
    write_fasta(tmp_path / "u.fasta", "u", codes)
    for m in ("n", "raw"):
        assert run(["-m", m, "--max-distance", "0", str(tmp_path / "u.fasta")]) == HEADER
