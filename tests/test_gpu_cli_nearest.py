"""GPU (-m gpu): `distance --nearest K` end to end — the TSV text byte for byte what Python builds from the oracle's
values, in the documented order (per row record in input order, its neighbours by (key of the device's value, index)),
and the usage errors of the flag."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import CODES, LETTERS, random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance\n"


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


def keys(vals):
    vals = np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def order(key_row, k, exclude=-1):
    idx = [j for j in range(len(key_row)) if j != exclude]
    return sorted(idx, key=lambda j: (int(key_row[j]), j))[:k]


def text(ids_r, ids_c, device_vals, oracle_vals, k, square, measure):
    """device_vals / oracle_vals: n_rows x n_cols (square: full symmetric) matrices."""
    lines = [HEADER]
    kk = keys(device_vals)
    for i in range(len(ids_r)):
        for j in order(kk[i], k, exclude=i if square else -1):
            v = oracle_vals[i, j]
            lines.append(f"{ids_r[i]}\t{ids_c[j]}\t{oracle.format_distance(int(v) if measure in da.INT_MEASURES else float(v))}\n")
    return "".join(lines)


def full(cond, n):
    m = np.zeros((n, n), cond.dtype)
    iu = np.triu_indices(n, 1)
    m[iu] = cond
    m[(iu[1], iu[0])] = cond
    return m


def run(args):
    r = subprocess.run([CLI] + args, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.mark.parametrize("measure", ["raw", "tn93"])
def test_square(tmp_path, measure):
    codes = random_alignment(70, 600, seed=61)
    ids = write_fasta(tmp_path / "a.fasta", "a", codes)
    with da.Engine(0) as eng:   # the order is the device values' (DST_OUT_DISTANCE), the text the oracle's
        eng.upload(0, codes)
        dev = full(eng.run_square(measure), 70)
    want = text(ids, ids, dev, full(oracle.all_pairs_square(measure, codes), 70), 3, True, measure)
    assert run(["-m", measure, "--nearest", "3", str(tmp_path / "a.fasta")]) == want


def test_two_files(tmp_path):
    a = random_alignment(40, 500, seed=62)
    b = random_alignment(90, 500, seed=63)
    ida = write_fasta(tmp_path / "a.fasta", "a", a)
    idb = write_fasta(tmp_path / "b.fasta", "b", b)
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        dev = eng.run_rect("raw", 0, 1)
    want = text(ida, idb, dev, oracle.all_pairs_rect("raw", a, b), 4, False, "raw")
    assert run(["--nearest", "4", str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")]) == want


@pytest.mark.parametrize("args", [
    ["--nearest", "0"], ["--nearest", "257"], ["--nearest=0"],
    ["--nearest", "3", "-s", "{b}"], ["--nearest", "3", "--gpus", "2"], ["--nearest", "3", "--devices", "0,1"],
])
def test_usage_errors(tmp_path, args):
    codes = random_alignment(10, 50, seed=64)
    write_fasta(tmp_path / "a.fasta", "a", codes)
    write_fasta(tmp_path / "b.fasta", "b", codes)
    args = [x.replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    r = subprocess.run([CLI] + args + [str(tmp_path / "a.fasta")], capture_output=True)
    assert r.returncode == 2, r.stderr.decode()
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: ")
