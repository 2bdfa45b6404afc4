"""GPU (-m gpu): `distance --stream-summary T [--stream-summary-for loaded|streamed]` and `distance --stream-histogram W
[--stream-bins B]` with `-i loaded.fasta -s big.fasta`, end to end.  The yardstick is the loaded-set form of the same
question: `--summary T big.fasta loaded.fasta` for the streamed side, `--summary T loaded.fasta big.fasta` and
`--histogram W --bins B loaded.fasta big.fasta` for the loaded side and the histogram, byte for byte.  tn93's tallies are
not symmetric in the two records (the streamed record's base counts are q), so its loaded side and histogram are formed
from SummaryStream.result() the way test_gpu_cli_summary.py forms its expected lines.  Every mode also with -o, `-s -`,
DISTANCE_WIRE=codes and two batch bounds."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import random_alignment, to_fasta_bytes
from test_gpu_cli_summary import histogram_text, summary_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
SYMMETRIC = ("n", "n_high", "raw", "jc69", "k80")
N_L, N_S, L = 120, 200, 300


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
    d = tmp_path_factory.mktemp("stream_summary")
    both = random_alignment(N_L + N_S, L, seed=431)   # upper-case FASTA with IUPAC codes and gaps
    loaded, streamed = both[:N_L], both[N_L:]
    streamed[40] = streamed[7]                        # equal records across batches ...
    streamed[41] = loaded[3]                          # ... a streamed record equal to a loaded one: within at T = 0
    streamed[50] = 240                                # ... and an all-N record on either side: NaN, mean NaN
    loaded[9] = 240
    (d / "a.fasta").write_bytes(fasta("a", loaded))
    (d / "b.fasta").write_bytes(fasta("b", streamed))
    return str(d / "a.fasta"), str(d / "b.fasta"), d, loaded, streamed


SMALL = ["--slab-pairs", str(37 * N_L), "--batchsize", "2"]   # (--slab-pairs bounds a stream's batches) 37 records: six batches


def thresholds(measure):
    return ("3", "2") if measure in da.INT_MEASURES else ("0.03", "0.004")   # (T, W)


def variants(files, mode, measure, want):
    """the mode's output with -o, from stdin, with the code bytes on the wire and at another batch bound"""
    a, b, d = files[:3]
    base = ["-m", measure] + mode
    assert run(base + SMALL + ["-i", a, "-s", b], wire="codes") == want
    assert run(base + ["--slab-pairs", str(3 * N_L), "-i", a, "-s", b]) == want
    assert run(base + ["--slab-pairs", "1", "-i", a, "-s", b]) == want           # one record per batch
    with open(b, "rb") as fh:
        assert run(base + SMALL + [a, "-s", "-"], stdin=fh.read()) == want
    out = d / f"{measure}.tsv"
    assert run(base + SMALL + ["-o", str(out), "-i", a, "-s", b]) == ""
    assert out.read_text() == want


@pytest.mark.parametrize("measure", ALL)
def test_streamed_side_is_the_rectangle_with_the_stream_as_rows(files, measure):
    a, b = files[:2]
    T = thresholds(measure)[0]
    want = run(["-m", measure, "--summary", T, b, a])
    lines = want.splitlines()
    assert lines[0] == "sequence\twithin\tcompared\tmean" and len(lines) == 1 + N_S and lines[1].startswith("b0\t")
    assert ("\tNaN" in want) == (measure not in da.INT_MEASURES)
    mode = ["--stream-summary", T, "--stream-summary-for", "streamed"]
    assert run(["-m", measure] + mode + SMALL + ["-i", a, "-s", b]) == want


@pytest.mark.parametrize("measure", ALL)
def test_loaded_side_and_histogram(files, measure):
    a, b, _, loaded, streamed = files
    T, W = thresholds(measure)
    if measure in SYMMETRIC:
        want = run(["-m", measure, "--summary", T, a, b])
        hist = run(["-m", measure, "--histogram", W, "--bins", "24", a, b])
        hist256 = run(["-m", measure, "--histogram", W, a, b])
    else:
        with da.Engine(0) as eng:
            eng.upload(0, loaded)
            res = {}
            for bins in (24, 256):
                with eng.summary_stream(measure, N_S, threshold=float(T), bins=bins, width=float(W)) as st:
                    st.push(streamed)
                    st.pop()
                    res[bins] = st.result()
        want = summary_text([f"a{r}" for r in range(N_L)], res[24])
        hist, hist256 = histogram_text(measure, res[24], float(W)), histogram_text(measure, res[256], float(W))
    lines = want.splitlines()
    assert lines[0] == "sequence\twithin\tcompared\tmean" and len(lines) == 1 + N_L and lines[1].startswith("a0\t")
    assert hist.count("\n") == 26 and hist256.count("\n") == 258
    assert run(["-m", measure, "--stream-summary", T] + SMALL + ["-i", a, "-s", b]) == want
    assert run(["-m", measure, "--stream-histogram", W, "--stream-bins", "24"] + SMALL + ["-i", a, "-s", b]) == hist
    assert run(["-m", measure, "--stream-histogram", W] + SMALL + ["-i", a, "-s", b]) == hist256   # --stream-bins defaults to 256


@pytest.mark.parametrize("mode", ["loaded", "streamed", "histogram"])
def test_output_file_stdin_wire_and_batch_bounds(files, mode):
    a, b = files[:2]
    measure = "k80"
    T, W = thresholds(measure)
    flags = {"loaded": [f"--stream-summary={T}", "--stream-summary-for=loaded"],
             "streamed": ["--stream-summary", T, "--stream-summary-for", "streamed"],
             "histogram": [f"--stream-histogram={W}", "--stream-bins=24"]}[mode]
    want = run(["-m", measure] + {"loaded": ["--summary", T, a, b], "streamed": ["--summary", T, b, a],
                                  "histogram": ["--histogram", W, "--bins", "24", a, b]}[mode])
    variants(files, flags, measure, want)


def test_thresholds_zero_and_inf(files):
    a, b = files[:2]
    for T in ("0", "inf"):
        assert run(["-m", "n", "--stream-summary", T] + SMALL + ["-i", a, "-s", b]) == run(["-m", "n", "--summary", T, a, b])
        assert (run(["-m", "k80", "--stream-summary", T, "--stream-summary-for", "streamed"] + SMALL + ["-i", a, "-s", b])
                == run(["-m", "k80", "--summary", T, b, a]))
    at_0 = run(["-m", "n", "--stream-summary", "0", "-i", a, "-s", b]).splitlines()
    assert int(at_0[1 + 3].split("\t")[1]) >= 1                       # a3 has an equal record in the stream
    assert np.array_equal([x.split("\t")[0] for x in at_0[1:]], [f"a{r}" for r in range(N_L)])
