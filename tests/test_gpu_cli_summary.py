"""GPU (-m gpu): `distance --summary T` and `distance --histogram W --bins B` end to end against Engine.summary formatted
in Python: every measure, two inputs, -o, stdin, any slab bound, and the integer bin edges of -m n."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import random_alignment
from test_gpu_cli_links import write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
N = 120


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(args, stdin=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    codes = random_alignment(N, 400, seed=85)
    codes[5] = codes[3]   # identical records: within at 0
    codes[9] = 240        # an all-N record: NaN against everything, mean NaN
    d = tmp_path_factory.mktemp("summary")
    write_fasta(d / "a.fasta", "a", codes)
    write_fasta(d / "b.fasta", "b", codes[:17])
    return codes, str(d / "a.fasta"), str(d / "b.fasta")


def summary_text(ids, s):
    out = "sequence\twithin\tcompared\tmean\n"
    for k, name in enumerate(ids):
        c = int(s["summable"][k])
        mean = s["sum"][k] / c if c else float("nan")
        out += f"{name}\t{int(s['within'][k])}\t{c}\t{da.format_distance('raw', mean)}\n"
    return out


def histogram_text(measure, s, width):
    out = "distance\tpairs\n"
    for b, count in enumerate(s["hist"]):
        edge = str(b * int(width)) if measure in da.INT_MEASURES else da.format_distance(measure, b * width)
        out += f"{edge}\t{int(count)}\n"
    return out + f"NaN\t{s['nan_pairs']}\n"


@pytest.mark.parametrize("measure", ["n", "n_high", "raw", "jc69", "k80", "tn93"])
def test_one_input(alignment, tmp_path, measure):
    codes, fasta, _ = alignment
    ids = [f"a{r}" for r in range(N)]
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square(measure)
        finite = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
        t = float(np.quantile(finite, 0.05))
        text = str(int(t)) if measure in da.INT_MEASURES else repr(t)
        want = summary_text(ids, eng.summary(measure, float(text)))
        width = 2.0 if measure in da.INT_MEASURES else float(repr(float(finite.max()) / 20))
        wtext = "2" if measure in da.INT_MEASURES else repr(width)
        hist = histogram_text(measure, eng.summary(measure, bins=24, width=width, per_record=False), width)
        hist256 = histogram_text(measure, eng.summary(measure, bins=256, width=width, per_record=False), width)
    assert want.count("\n") == N + 1 and ("\tNaN\n" in want) == (measure not in da.INT_MEASURES)   # the all-N record's mean
    assert run(["-m", measure, "--summary", text, fasta]) == want
    assert run(["-m", measure, f"--summary={text}", "--slab-pairs", "1", "-t", "2", fasta]) == want
    assert run(["-m", measure, "--histogram", wtext, "--bins", "24", fasta]) == hist
    assert run(["-m", measure, f"--histogram={wtext}", "--bins=24", "--slab-pairs", "1", fasta]) == hist
    assert run(["-m", measure, "--histogram", wtext, fasta]) == hist256   # --bins defaults to 256
    assert hist.count("\n") == 26 and hist.endswith(f"NaN\t{0 if measure in da.INT_MEASURES else N - 1}\n")
    if measure in ("n", "tn93"):
        out = tmp_path / "summary.tsv"
        assert run(["-m", measure, "--summary", text, "-o", str(out), fasta]) == ""
        assert out.read_text() == want
        with open(fasta, "rb") as fh:
            assert run(["--histogram", wtext, "--bins", "24", "-m", measure], stdin=fh) == hist
    if measure == "n":
        edges = [line.split("\t")[0] for line in hist.splitlines()[1:-1]]
        assert edges == [str(2 * b) for b in range(24)]   # integer bin edges


def test_two_inputs(alignment):
    codes, fa, fb = alignment
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(codes[:17]))
        for first, second, rs, cs, prefix, nr in ((fa, fb, 0, 1, "a", N), (fb, fa, 1, 0, "b", 17)):
            ids = [f"{prefix}{r}" for r in range(nr)]
            for m, t, w in (("n_high", 30.0, 5.0), ("k80", 0.06, 0.01)):
                want = summary_text(ids, eng.summary(m, t, square=False, row_slot=rs, col_slot=cs))
                assert run(["-m", m, "--summary", repr(t), first, second]) == want
                assert run(["-m", m, "--summary", repr(t), "--slab-pairs", "40", "-i", first, second]) == want
                hist = histogram_text(m, eng.summary(m, square=False, row_slot=rs, col_slot=cs, bins=12, width=w, per_record=False), w)
                assert run(["-m", m, "--histogram", repr(w), "--bins", "12", first, second]) == hist
