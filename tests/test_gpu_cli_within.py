"""GPU (-m gpu): `distance --within T [-m M] -i loaded.fasta -s big.fasta` end to end — the stream-mode header, then
exactly the lines of the full `-s` run whose distance is at most T, in that run's order and with that run's bytes: every
measure, -o, stdin, both wire formats, batches cut by --slab-pairs, T = inf, and an empty stream."""
import os
import subprocess

import numpy as np
import pytest

from helpers import random_alignment, to_fasta_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance\n"
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
N_L, N_S, L = 40, 90, 300


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(args, stdin=None, wire=None):
    env = {k: v for k, v in os.environ.items() if k != "DISTANCE_WIRE"}
    if wire:
        env["DISTANCE_WIRE"] = wire
    r = subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def fasta(prefix, codes):
    return b"".join(b">" + f"{prefix}{r}".encode() + b" description\n" + to_fasta_bytes(row) + b"\n" for r, row in enumerate(codes))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("within")
    both = random_alignment(N_L + N_S, L, seed=331)              # one root: the distances are small and finite
    loaded, streamed = both[:N_L], both[N_L:]
    streamed[40] = streamed[7]                        # equal records across batches ...
    streamed[41] = loaded[3]                          # ... a streamed record equal to a loaded one: distance 0
    streamed[50] = 240                                # ... and one without a resolved site: NaN for the f64 measures
    (d / "a.fasta").write_bytes(fasta("a", loaded))
    (d / "b.fasta").write_bytes(fasta("b", streamed))
    return str(d / "a.fasta"), str(d / "b.fasta"), d


_full = {}


def full_run(files, measure):
    """the full -s run of the measure, once"""
    if measure not in _full:
        _full[measure] = run(["-m", measure, "-i", files[0], "-s", files[1]])
        lines = _full[measure].splitlines(keepends=True)
        assert lines[0] == HEADER and len(lines) == 1 + N_L * N_S
    return _full[measure]


def filtered(full_text, T):
    """the full run's lines whose own third field is at most T (NaN is not)"""
    lines = full_text.splitlines(keepends=True)
    return "".join([HEADER] + [x for x in lines[1:] if float(x.rstrip("\n").split("\t")[2]) <= T])


def between_two_values(full_text, share):
    """a threshold half way between two neighbouring distinct values of the full run (at least 1e-6 apart: far more than
    the 12 printed decimals can hide), at or above the `share` quantile of its finite values"""
    vals = np.array([float(x.split("\t")[2]) for x in full_text.splitlines()[1:]])
    vals = vals[np.isfinite(vals)]
    u = np.unique(vals)
    for q in range(int(np.searchsorted(u, np.quantile(vals, share))), len(u) - 1):
        if u[q + 1] - u[q] > 1e-6:
            return float((u[q] + u[q + 1]) / 2)
    raise AssertionError("no gap")


@pytest.mark.parametrize("measure", ALL)
def test_lines_are_the_full_runs_within_T(files, measure):
    full = full_run(files, measure)
    thresholds = [0, 3, 12.5, 1e3] if measure in ("n", "n_high") else [0, between_two_values(full, 0.1), between_two_values(full, 0.6)]
    for T in thresholds:
        want = filtered(full, T)
        got = run(["-m", measure, "--within", repr(T), "-i", files[0], "-s", files[1]])
        assert got == want, (measure, T)
        assert want.count("\n") >= 2                                 # (streamed[41] is a loaded record: distance 0)
    assert filtered(full, thresholds[-2]).count("\n") < filtered(full, thresholds[-1]).count("\n") <= 1 + N_L * N_S


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
def test_the_same_bytes_whatever_the_plumbing(files, measure):
    a, b, d = files
    full = full_run(files, measure)
    T = between_two_values(full, 0.3)
    want = filtered(full, T)
    assert 1 + N_L < want.count("\n") < 1 + N_L * N_S
    flags = ["-m", measure, "--within", repr(T), "-i", a]
    out = d / f"out_{measure}.tsv"
    assert run(flags + ["-s", b, "-o", str(out)]) == "" and out.read_text() == want
    assert run(flags + ["-s", "-"], stdin=open(b, "rb").read()) == want
    assert run(flags + ["-s", b], wire="codes") == want
    assert run(["--within=" + repr(T), "-s", b, "--slab-pairs", str(N_L * 7), "-m", measure, a]) == want     # 13 batches
    assert run(flags + ["-s", "-", "--slab-pairs", str(N_L)], stdin=open(b, "rb").read(), wire="codes") == want   # 90 batches


@pytest.mark.parametrize("measure", ["n_high", "jc69", "k80"])
def test_inf_is_the_full_run_without_its_nan_lines(files, measure):
    full = full_run(files, measure)
    lines = full.splitlines(keepends=True)
    want = "".join(x for x in lines if not x.rstrip("\n").endswith("NaN"))
    assert want == filtered(full, float("inf"))
    if measure != "n_high":
        assert want.count("\n") <= len(lines) - N_L                  # the all-N streamed record's lines
    assert run(["-m", measure, "--within", "inf", "-i", files[0], "-s", files[1]]) == want


def test_an_empty_stream(files):
    empty = files[2] / "empty.fasta"
    empty.write_text("")
    r = subprocess.run([CLI, "--within", "3", "-i", files[0], "-s", str(empty)], capture_output=True)
    assert r.returncode == 1 and b"Empty FASTA file" in r.stderr
    assert r.stdout.decode() in ("", HEADER)
    plain = subprocess.run([CLI, "-i", files[0], "-s", str(empty)], capture_output=True)
    assert (r.returncode, r.stdout, r.stderr) == (plain.returncode, plain.stdout, plain.stderr)
