"""GPU (-m gpu): `distance --windows W --step S --window-closest K -i query.fasta -s panel.fasta` and `--regions FILE
--window-closest K` end to end on the designed set of window_closest_cases as FASTA files: byte for byte what
`--window-nearest K query.fasta panel.fasta` prints, for every measure, with several batches, stdin, both wires and -o."""
import os
import subprocess

import pytest

from helpers import CODES, LETTERS
from window_closest_cases import loaded_set, streamed_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\twindow\tstart\tend\tdistance"
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
# the designed windows as regions (1-based, inclusive; an empty window has no region)
REGIONS = [("whole", 1, 300), ("cut", 6, 133), ("chunk", 129, 256), ("one", 131, 131), ("last", 300, 300), ("cut", 6, 133), ("first", 1, 128)]
SLIDING = ["--windows", "100", "--step", "50"]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def write_fasta(path, prefix, codes):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    with open(path, "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">{prefix}{r} description\n" + "".join(lut[int(c)] for c in row) + "\n")


def run(args, stdin=None, env=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_closest")
    write_fasta(d / "q.fasta", "q", loaded_set())
    write_fasta(d / "panel.fasta", "p", streamed_set())
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" for name, first, last in REGIONS))
    return d, str(d / "q.fasta"), str(d / "panel.fasta"), str(d / "regions.tsv")


_nearest = {}


def window_nearest(windows, measure, q, panel):
    """the loaded-set run the stream's output is held to, once per (windows, measure)"""
    key = (tuple(windows), measure)
    if key not in _nearest:
        _nearest[key] = run(windows + ["-m", measure, "--window-nearest", "3", q, panel])
    return _nearest[key]


@pytest.mark.parametrize("measure", ALL)
def test_sliding_windows_and_regions_equal_window_nearest(files, measure):
    _, q, panel, regions = files
    for windows, n_windows in ((SLIDING, 5), (["--regions", regions], len(REGIONS))):
        want = window_nearest(windows, measure, q, panel)
        lines = want.splitlines()
        assert lines[0] == HEADER and len(lines) == 1 + 9 * n_windows * 3
        got = run(windows + ["-m", measure, "--window-closest", "3", "-i", q, "-s", panel])
        assert got == want, (measure, windows[0])


@pytest.mark.parametrize("measure", ["raw", "tn93"])
def test_batches_stdin_codes_wire_and_output_file(files, measure):
    d, q, panel, regions = files
    want = window_nearest(SLIDING, measure, q, panel)
    base = SLIDING + ["-m", measure, "--window-closest", "3"]
    # --slab-pairs bounds the batch: 9 loaded records, 64 streamed records per batch, 5 batches
    assert run(base + ["--slab-pairs", "576", "-i", q, "-s", panel]) == want
    assert run(base + ["--slab-pairs", "9", "-i", q, "-s", panel]) == want       # one record per batch
    with open(panel, "rb") as fh:
        assert run(base + [q, "-s", "-"], stdin=fh) == want
    assert run(base + ["--slab-pairs", "576", "-i", q, "-s", panel], env=dict(os.environ, DISTANCE_WIRE="codes")) == want
    out = d / f"out_{measure}.tsv"
    assert run(base + ["-o", str(out), "-i", q, "-s", panel]) == "" and out.read_text() == want
    want_regions = window_nearest(["--regions", regions], measure, q, panel)
    assert run(["--regions", regions, "-m", measure, "--window-closest", "3", "--slab-pairs", "576", "-i", q, "-s", panel]) == want_regions
