"""GPU (-m gpu): `distance --representatives T` end to end — the TSV text byte for byte what Python builds from
Engine.representatives' rep and tallies, the records' ids, dst_finalize and dst_format_distance: from a file, from stdin,
into -o, and with one-row slabs."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from test_gpu_cli_clusters import clustered_codes, fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def expected(codes, ids, measure, threshold):
    """(text, rep): one line per record, a member's value from the tallies of the pair (representative, record)"""
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        rep, _, tallies = eng.representatives(measure, float(threshold), tallies=True)
        counts = eng.base_counts(0) if measure == "tn93" else None
    lines = ["sequence\trepresentative\tdistance\n"]
    for j, r in enumerate(rep):
        r = int(r)
        if r == j:
            lines.append(f"{ids[j]}\t{ids[j]}\t\n")
        else:
            qc, tc = (counts[r], counts[j]) if counts is not None else (None, None)
            lines.append(f"{ids[j]}\t{ids[r]}\t{da.format_distance(measure, da.finalize(measure, tallies[j], qc, tc))}\n")
    return "".join(lines), rep


@pytest.mark.parametrize("measure,threshold", [("n", "3"), ("raw", "0.004"), ("tn93", "0.004")])
def test_file(tmp_path, measure, threshold):
    codes = clustered_codes(90, 700, seed=81)
    ids, text = fasta(codes, "s")
    (tmp_path / "a.fasta").write_bytes(text)
    want, rep = expected(codes, ids, measure, threshold)
    kept = int((rep == np.arange(90)).sum())
    assert 1 < kept < 90
    r = subprocess.run([CLI, "-m", measure, "--representatives", threshold, str(tmp_path / "a.fasta")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == want
    # a representative's line: its own id twice and an empty third field, the line ends with the tab
    body = r.stdout.decode().splitlines()[1:]
    own = [x for x in body if x.endswith("\t")]
    assert len(own) == kept and all(x.split("\t")[0] == x.split("\t")[1] and x.split("\t")[2] == "" for x in own)
    assert all(len(x.split("\t")) == 3 for x in body)
    # one-row slabs: identical bytes
    r1 = subprocess.run([CLI, "-m", measure, "--representatives", threshold, "--slab-pairs", "1", str(tmp_path / "a.fasta")],
                        capture_output=True)
    assert r1.returncode == 0, r1.stderr.decode()
    assert r1.stdout == r.stdout


def test_stdin_and_output(tmp_path):
    codes = clustered_codes(120, 500, seed=82)
    ids, text = fasta(codes, "rec_")
    want, _ = expected(codes, ids, "tn93", "0.005")
    r = subprocess.run([CLI, "-m", "tn93", "--representatives=0.005"], input=text, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == want
    out = tmp_path / "representatives.tsv"
    r = subprocess.run([CLI, "--representatives", "0.005", "-m", "tn93", "-o", str(out)], input=text, capture_output=True)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert out.read_text() == want
    # inf: record 0 stands for every record whose distance to it is not NaN
    want_inf, rep = expected(codes, ids, "raw", "inf")
    assert not rep.any()
    r = subprocess.run([CLI, "--representatives", "inf"], input=text, capture_output=True)
    assert r.returncode == 0 and r.stdout.decode() == want_inf
