"""GPU (-m gpu): `distance --site-counts [--site-groups FILE]` and `distance --windows W [--step S] | --regions FILE
--window-site-stats [--site-groups FILE]`, end to end on an upper-case FASTA with ambiguity letters, byte for byte against
site_counts_reference's text: with and without groups, overlapping and repeated regions, a region in which nothing is
called, -o, stdin, -m ignored, the walk in small ranges of sites, and the warning for ids that are in no input."""
import os
import subprocess

import numpy as np
import pytest

from helpers import CODES, LETTERS, random_alignment
from site_counts_reference import counts_text, group_sizes, site_counts, site_stats, stats_text
from window_reference import sliding

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
N, L = 30, 700
BLANK = (150, 160)   # columns that hold N in every record
REGIONS = [("whole", 1, 700), ("orf1", 10, 140), ("blank", 151, 160), ("one", 129, 129), ("orf1b", 100, 300), ("orf1", 10, 140)]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(args, stdin=None, stderr=None, env=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin, env=env)
    assert r.returncode == 0, r.stderr.decode()
    if stderr is not None:
        stderr.append(r.stderr.decode())
    return r.stdout.decode()


@pytest.fixture(scope="module")
def al(tmp_path_factory):
    codes = random_alignment(N, L, seed=91, divergence=0.05, p_ambig=0.03, p_gap=0.04)
    codes[:, BLANK[0]:BLANK[1]] = 240
    d = tmp_path_factory.mktemp("site_counts")
    lut = {int(c): chr(LETTERS[k]).upper() for k, c in enumerate(CODES)}
    with open(d / "a.fasta", "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">a{r} description\n" + "".join(lut[int(c)] for c in row) + "\n")
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" for name, first, last in REGIONS))
    # groups z, x, y in order of their first record (a0: z, a1: x, a2: y); a6, a13, a20, a27 have none; two ids are nowhere
    names = ["z", "x", "y"]
    labels = np.array([-1 if i % 7 == 6 else i % 3 for i in range(N)])
    with open(d / "labels.tsv", "w") as fh:
        fh.write("nobody\tz\n" + "".join(f"a{i}\t{names[i % 3]}\n" for i in range(N) if i % 7 != 6) + "noone\tq\n")
    return {"codes": codes, "dir": d, "fasta": str(d / "a.fasta"), "labels_file": str(d / "labels.tsv"), "labels": labels,
            "names": names, "regions": str(d / "regions.tsv")}


def grouping(al, grouped):
    if grouped:
        return al["labels"], 3, al["names"], group_sizes(al["labels"], N, 3), ["--site-groups", al["labels_file"]]
    return None, 1, ["all"], [N], []


def fmt(x):
    return f"{x:.12f}"


@pytest.mark.parametrize("grouped", [False, True])
def test_site_counts(al, grouped, tmp_path):
    g, G, names, sizes, flags = grouping(al, grouped)
    want = counts_text(site_counts(al["codes"], g, G), names, sizes)
    err = []
    got = run(["--site-counts"] + flags + [al["fasta"]], stderr=err)
    assert got == want
    assert err[0].count("warning: --site-groups: 2 ids of") == (1 if grouped else 0)
    # -m is accepted and ignored; -o; stdin; many small ranges of sites
    out = tmp_path / "out.tsv"
    assert run(["-m", "tn93", "--site-counts", "-o", str(out)] + flags + [al["fasta"]]) == "" and out.read_text() == want
    with open(al["fasta"], "rb") as fh:
        assert run(["--site-counts"] + flags, stdin=fh) == want
    small = dict(os.environ, DISTANCE_SITE_RANGE_ENTRIES=str(37 * G * 5))
    assert run(["--site-counts"] + flags + [al["fasta"]], env=small) == want


@pytest.mark.parametrize("grouped", [False, True])
def test_window_site_stats(al, grouped, tmp_path):
    g, G, names, sizes, flags = grouping(al, grouped)
    counts = site_counts(al["codes"], g, G)
    # --windows 128 --step 50: overlapping windows that cross the chunks
    windows = sliding(L, 128, 50)
    plain = run(["--windows", "128", "--step", "50", al["fasta"]]).splitlines()[1:1 + len(windows)]
    fields = ["\t".join(x.split("\t")[2:5]) for x in plain]
    assert fields[1] == "2\t51\t178"
    want = stats_text(site_stats(counts, windows, sizes), fields, names, fmt)
    assert run(["--windows", "128", "--step", "50", "--window-site-stats"] + flags + [al["fasta"]]) == want
    # --regions: overlapping and repeated regions, one in which nothing is called, one site
    regions = [(first - 1, last) for _, first, last in REGIONS]
    fields = [f"{name}\t{first}\t{last}" for name, first, last in REGIONS]
    stats = site_stats(counts, regions, sizes)
    assert not stats["called"][2].any()
    want = stats_text(stats, fields, names, fmt)
    assert "\tNaN\tNaN\n" in want
    args = ["--regions", al["regions"], "--window-site-stats"] + flags
    assert run(args + [al["fasta"]]) == want
    out = tmp_path / "out.tsv"
    assert run(["-m", "k80"] + args + ["-o", str(out), al["fasta"]]) == "" and out.read_text() == want
    with open(al["fasta"], "rb") as fh:
        assert run(args, stdin=fh) == want
    # ranges of 37 sites: most regions cross a range's end and are counted on their own
    small = dict(os.environ, DISTANCE_SITE_RANGE_ENTRIES=str(37 * G * 5))
    assert run(args + [al["fasta"]], env=small) == want
