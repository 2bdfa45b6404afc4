"""GPU (-m gpu): `distance --tree nj --bootstrap B` end to end — the labelled Newick line byte for byte what Python
builds from Engine.nj, Engine.nj_bootstrap and da.newick; without its labels, the plain `--tree nj` line — and a failing
replicate (exit 1, `error: `, nothing on stdout)."""
import os
import subprocess

import numpy as np
import pytest

import bootstrap_reference as B
import distance_amd as da
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


@pytest.mark.parametrize("measure", ["raw", "tn93", "n"])
def test_labelled_tree(tmp_path, measure):
    codes = random_alignment(50, 600, seed=95, divergence=0.04)
    ids = [f"s{r}" for r in range(49)] + ["it's"]
    path = tmp_path / "a.fasta"
    path.write_bytes(fasta(codes, ids))
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        parent, length = eng.nj(measure)
        support = eng.nj_bootstrap(measure, codes, parent, 8, seed=3)
    want = da.newick(parent, length, ids, support=support)
    r = subprocess.run([CLI, "-m", measure, "--tree", "nj", "--bootstrap", "8", "--seed", "3", str(path)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    plain = subprocess.run([CLI, "-m", measure, "--tree", "nj", str(path)], capture_output=True)
    assert plain.returncode == 0 and B.strip_labels(r.stdout) == plain.stdout
    _, _, _, labels = B.parse_labelled(r.stdout)
    got = sorted(x for x in labels if x is not None)
    assert len(got) == 50 - 3 and got[-1] <= 8
    # the default seed is 1; -o and --slab-pairs do not change the text
    out = tmp_path / "t.nwk"
    r1 = subprocess.run([CLI, "-m", measure, "--tree=nj", "--bootstrap=8", "--slab-pairs", "13", "-o", str(out),
                         str(path)], capture_output=True)
    assert r1.returncode == 0 and r1.stdout == b"", r1.stderr.decode()
    r2 = subprocess.run([CLI, "-m", measure, "--tree", "nj", "--bootstrap", "8", "--seed", "1", str(path)],
                        capture_output=True)
    assert out.read_bytes() == r2.stdout


def test_failing_replicate(tmp_path):
    n, L = 12, 300
    codes = random_alignment(n, L, seed=96)
    codes[:, 40] = 136
    codes[7] = CODES[14]
    codes[7, 40] = 136          # one resolved site: a replicate without column 40 has NaN raw distances
    assert any(40 not in set(B.columns(1, r, L).tolist()) for r in range(32))
    ids = [f"q{r}" for r in range(n)]
    r = subprocess.run([CLI, "-m", "raw", "--tree", "nj", "--bootstrap", "32"], input=fasta(codes, ids),
                       capture_output=True)
    assert r.returncode == 1 and r.stdout == b"", r.stderr
    assert r.stderr.startswith(b"error: bootstrap replicate ") and b"'q0'" in r.stderr and b"'q7'" in r.stderr
