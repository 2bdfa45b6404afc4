"""GPU (-m gpu): `distance --dendrogram <linkage>` end to end — the Newick line byte for byte what da.newick_rooted
writes for the restatement's tree (dendrogram_reference.py) of the library's distances and the records' ids, for every
linkage, from a file, from stdin, into -o, with --slab-pairs and quoted ids, for two records — and its error for a
non-finite distance."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import dendrogram_reference as R
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


def reference_text(codes, measure, linkage, ids):
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        D = R.square(len(codes), eng.run_square(measure))
    parent, length, _ = R.dendrogram(D, linkage)
    return da.newick_rooted(parent, length, ids)


@pytest.mark.parametrize("linkage", R.LINKAGES)
@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_file(tmp_path, measure, linkage):
    codes = random_alignment(80, 700, seed=91, divergence=0.04)
    ids = [f"s{r}" for r in range(80)]
    (tmp_path / "a.fasta").write_bytes(fasta(codes, ids))
    want = reference_text(codes, measure, linkage, ids)
    r = subprocess.run([CLI, "-m", measure, "--dendrogram", linkage, str(tmp_path / "a.fasta")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    assert r.stdout.count(b"\n") == 1 and r.stdout.endswith(b");\n") and r.stdout.count(b"(") == 79


def test_stdin_output_slabs_and_quoted_ids(tmp_path):
    codes = random_alignment(60, 400, seed=92, divergence=0.05)
    ids = [f"rec_{r}" for r in range(57)] + ["it's", "a:b", "(x)"]
    text = fasta(codes, ids)
    want = reference_text(codes, "tn93", "average", ids)
    assert b"'it''s'" in want and b"'a:b'" in want and b"'(x)'" in want
    r = subprocess.run([CLI, "-m", "tn93", "--dendrogram=average"], input=text, capture_output=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()
    out = tmp_path / "tree.nwk"
    r = subprocess.run([CLI, "--dendrogram", "average", "-m", "tn93", "--slab-pairs", "7", "-o", str(out)], input=text,
                       capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert out.read_bytes() == want


def test_two_records_and_one():
    codes = random_alignment(2, 50, seed=93)
    r = subprocess.run([CLI, "--dendrogram", "complete", "-m", "n"], input=fasta(codes, ["a", "b"]), capture_output=True)
    assert r.returncode == 0, r.stderr
    want = reference_text(codes, "n", "complete", ["a", "b"])
    assert r.stdout == want and want.startswith(b"(a:") and want.count(b",") == 1
    r = subprocess.run([CLI, "--dendrogram", "complete"], input=fasta(codes[:1], ["a"]), capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"error: "), r.stderr


def test_non_finite():
    codes = random_alignment(10, 50, seed=93)
    codes[6] = CODES[14]   # all N: raw is NaN against every record
    ids = [f"q{r}" for r in range(10)]
    r = subprocess.run([CLI, "--dendrogram", "average", "-m", "raw"], input=fasta(codes, ids), capture_output=True)
    assert r.returncode == 1 and r.stdout == b"", r.stderr
    assert r.stderr.startswith(b"error: ") and b"'q0'" in r.stderr and b"'q6'" in r.stderr
