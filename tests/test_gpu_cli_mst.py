"""GPU (-m gpu): `distance --mst` end to end — each line byte for byte the line the full run prints for that pair, the
lines in the reference forest's order (Kruskal over the device's own values), the same through -o, stdin and any slab
bound."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, LETTERS, random_alignment
from mst_reference import kruskal

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
    ids = [f"{prefix}{r}" for r in range(len(codes))]
    with open(path, "w") as fh:
        for i, row in zip(ids, codes):
            fh.write(f">{i} description\n" + "".join(lut[int(c)] for c in row) + "\n")
    return ids


def run(args, stdin=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    codes = random_alignment(N, 500, seed=81)
    codes[5] = codes[3]   # identical records: ties at 0 that fall to (i, j)
    codes[150] = codes[3]
    path = tmp_path_factory.mktemp("mst") / "a.fasta"
    return codes, write_fasta(path, "a", codes), str(path)


@pytest.mark.parametrize("measure", ["n_high", "raw", "tn93"])
def test_lines_are_the_full_runs_in_reference_order(alignment, tmp_path, measure):
    codes, ids, fasta = alignment
    full = run(["-m", measure, fasta]).splitlines(keepends=True)
    assert full[0] == HEADER and len(full) == 1 + N * (N - 1) // 2
    with da.Engine(0) as eng:   # the order is the device values' (DST_OUT_DISTANCE), the text the full run's
        eng.upload(0, codes)
        edges, _ = kruskal(N, eng.run_square(measure))
    assert len(edges) == N - 1
    i, j = edges[:, 0], edges[:, 1]
    at = i * (2 * N - i - 1) // 2 + (j - i - 1)   # canonical order: the full run's line 1 + at
    want = HEADER + "".join(full[1 + int(a)] for a in at)
    for a, (x, y) in zip(at[:3], edges[:3]):
        assert full[1 + int(a)].startswith(f"{ids[x]}\t{ids[y]}\t")
    got = run(["-m", measure, "--mst", fasta])
    assert got == want
    out = tmp_path / "mst.tsv"
    assert run(["-m", measure, "--mst", "-o", str(out), fasta]) == ""
    assert out.read_text() == want
    with open(fasta, "rb") as fh:
        assert run(["--mst", "-m", measure], stdin=fh) == want
    assert run(["-m", measure, "--mst", "--slab-pairs", "1500", fasta]) == want
