"""GPU (-m gpu): `distance --tree nj` end to end — the Newick line byte for byte what Python builds from Engine.nj and
the records' ids through da.newick, for every measure, from a file, from stdin, into -o, with quoted ids — and its
errors for fewer than 3 records and for a non-finite distance."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import nj_reference as R
from helpers import CODES, LETTERS, random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def fasta(codes, ids):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    return "".join(f">{i} description\n" + "".join(lut[int(c)] for c in row) + "\n" for i, row in zip(ids, codes)).encode()


def engine_tree(codes, measure, ids):
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        return da.newick(*eng.nj(measure), ids)


@pytest.mark.parametrize("measure", ["n", "n_high", "raw", "jc69", "k80", "tn93"])
def test_file(tmp_path, measure):
    codes = random_alignment(80, 700, seed=91, divergence=0.04)
    ids = [f"s{r}" for r in range(80)]
    (tmp_path / "a.fasta").write_bytes(fasta(codes, ids))
    want = engine_tree(codes, measure, ids)
    r = subprocess.run([CLI, "-m", measure, "--tree", "nj", str(tmp_path / "a.fasta")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    names, parent, _ = R.parse_newick(r.stdout)
    assert sorted(names) == sorted(ids) and len(parent) == 2 * 80 - 2


def test_stdin_output_slabs_and_quoted_ids(tmp_path):
    codes = random_alignment(60, 400, seed=92, divergence=0.05)
    ids = [f"rec_{r}" for r in range(57)] + ["it's", "a:b", "(x)"]
    text = fasta(codes, ids)
    want = engine_tree(codes, "tn93", ids)
    assert b"'it''s'" in want and b"'a:b'" in want and b"'(x)'" in want
    r = subprocess.run([CLI, "-m", "tn93", "--tree=nj"], input=text, capture_output=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()
    out = tmp_path / "tree.nwk"
    r = subprocess.run([CLI, "--tree", "nj", "-m", "tn93", "--slab-pairs", "7", "-o", str(out)], input=text,
                       capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert out.read_bytes() == want


def test_errors(tmp_path):
    codes = random_alignment(10, 50, seed=93)
    r = subprocess.run([CLI, "--tree", "nj"], input=fasta(codes[:2], ["a", "b"]), capture_output=True)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr.startswith(b"error: "), r.stderr
    codes[6] = CODES[14]   # all N: raw is NaN against every record
    ids = [f"q{r}" for r in range(10)]
    r = subprocess.run([CLI, "--tree", "nj", "-m", "raw"], input=fasta(codes, ids), capture_output=True)
    assert r.returncode != 0 and r.stdout == b"", r.stderr
    assert r.stderr.startswith(b"error: ") and b"'q0'" in r.stderr and b"'q6'" in r.stderr
