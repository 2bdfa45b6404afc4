"""GPU (-m gpu): `distance --clusters T` end to end — the TSV text byte for byte what Python builds from the engine's
labels and the records' ids (clusters numbered from 1 in order of first record), from a file, from stdin and into -o."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, LETTERS, random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def clustered_codes(n, L, seed):
    """Copies of a few parents with a handful of changes each: clusters at small thresholds."""
    rng = np.random.default_rng(seed)
    parents = random_alignment(max(n // 8, 1), L, seed=seed)
    codes = parents[rng.integers(0, len(parents), n)].copy()
    for r in range(n):
        sites = rng.choice(L, rng.integers(0, 6), replace=False)
        codes[r, sites] = rng.choice(CODES[:4], len(sites))
    return np.ascontiguousarray(codes)


def fasta(codes, prefix):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    ids = [f"{prefix}{r}" for r in range(len(codes))]
    text = "".join(f">{i} description\n" + "".join(lut[int(c)] for c in row) + "\n" for i, row in zip(ids, codes))
    return ids, text.encode()


def expected(ids, labels):
    number, lines = {}, ["sequence\tcluster\n"]
    for i, lab in enumerate(labels):
        if int(lab) == i:
            number[i] = len(number) + 1
        lines.append(f"{ids[i]}\t{number[int(lab)]}\n")
    return "".join(lines)


@pytest.mark.parametrize("measure,threshold", [("raw", "0.004"), ("tn93", "0.004"), ("n_high", "3"), ("n", "0")])
def test_file(tmp_path, measure, threshold):
    codes = clustered_codes(90, 700, seed=81)
    ids, text = fasta(codes, "s")
    (tmp_path / "a.fasta").write_bytes(text)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        labels, links = eng.clusters(measure, float(threshold))
    assert 1 < len(np.unique(labels)) < 90 or threshold == "0"
    r = subprocess.run([CLI, "-m", measure, "--clusters", threshold, str(tmp_path / "a.fasta")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == expected(ids, labels)


def test_stdin_and_output(tmp_path):
    codes = clustered_codes(120, 500, seed=82)
    ids, text = fasta(codes, "rec_")
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        labels, _ = eng.clusters("tn93", 0.005)
    want = expected(ids, labels)
    r = subprocess.run([CLI, "-m", "tn93", "--clusters=0.005"], input=text, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == want
    out = tmp_path / "clusters.tsv"
    r = subprocess.run([CLI, "--clusters", "0.005", "-m", "tn93", "-o", str(out)], input=text, capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert out.read_text() == want
    # inf: every pair whose value is not NaN links
    r = subprocess.run([CLI, "--clusters", "inf"], input=text, capture_output=True)
    assert r.stdout.decode() == "sequence\tcluster\n" + "".join(f"{i}\t1\n" for i in ids)
