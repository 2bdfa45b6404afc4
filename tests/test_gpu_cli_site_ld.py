"""GPU (-m gpu): `distance --ld R2 [--ld-min-count C] [--ld-groups FILE]`, end to end on an upper-case FASTA with ambiguity
letters, byte for byte against site_ld_reference's text: with and without groups, R2 0 and 1, a minimum count, stdin, -o,
-m ignored, small slabs, and a group with fewer than two listed sites."""
import os
import subprocess

import numpy as np
import pytest

from helpers import CODES, LETTERS
from site_ld_reference import ld_text, listed_sites

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
N, L = 40, 300
A, T, G, C_, N_, R = 136, 24, 72, 40, 240, 192


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(args, stdin=None, env=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin, env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def fmt(x):
    return f"{x:.12f}"


@pytest.fixture(scope="module")
def al(tmp_path_factory):
    """40 records x 300 sites, 36 variable sites in correlated blocks with a few N and R; groups z, x, y by i % 3 (a6, a13, ...
    have none); group y is made monomorphic everywhere but at one site, so it lists fewer than two"""
    rng = np.random.default_rng(77)
    codes = np.full((N, L), A, np.uint8)
    codes[:, 1::2] = C_
    labels = np.array([-1 if i % 7 == 6 else i % 3 for i in range(N)])
    base = rng.random((6, N)) < 0.4
    variable = sorted(rng.permutation(L)[:36].tolist() + [0, 127, 128])
    for p, s in enumerate(variable):
        minor = base[p % 6] ^ (rng.random(N) < 0.03 * (p // 6))
        minor &= labels != 2
        codes[minor, s] = G if s % 2 == 0 else T
        codes[rng.random(N) < 0.04, s] = N_ if p % 2 else R
    codes[[2, 5], 128] = G   # the one site that varies inside group y
    codes[:, 299], codes[3, 299] = C_, T   # one record alone holds the other base: listed at C = 1 only
    d = tmp_path_factory.mktemp("site_ld")
    lut = {int(c): chr(LETTERS[k]).upper() for k, c in enumerate(CODES)}
    with open(d / "a.fasta", "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">a{r} description\n" + "".join(lut[int(c)] for c in row) + "\n")
    names = ["z", "x", "y"]
    with open(d / "labels.tsv", "w") as fh:
        fh.write("".join(f"a{i}\t{names[i % 3]}\n" for i in range(N) if i % 7 != 6))
    return {"codes": codes, "fasta": str(d / "a.fasta"), "labels_file": str(d / "labels.tsv"), "labels": labels, "names": names}


@pytest.mark.parametrize("r2", ["0", "0.2", "1"])
def test_one_group(al, r2, tmp_path):
    want = ld_text(al["codes"], float(r2), fmt=fmt)
    assert want.count("\n") > 1
    assert run(["--ld", r2, al["fasta"]]) == want
    if r2 == "0.2":   # -m is accepted and ignored; -o; stdin; small slabs
        out = tmp_path / "out.tsv"
        assert run(["-m", "tn93", "--ld", r2, "-o", str(out), al["fasta"]]) == "" and out.read_text() == want
        with open(al["fasta"], "rb") as fh:
            assert run(["--ld", r2], stdin=fh) == want
        assert run(["--ld", r2, "--slab-pairs", "7", al["fasta"]]) == want
        assert run(["--ld", r2, "--slab-pairs", "100", al["fasta"]]) == want


def test_minimum_count(al):
    one, two = ld_text(al["codes"], 0.1, 1, fmt=fmt), ld_text(al["codes"], 0.1, 2, fmt=fmt)
    assert len(listed_sites(al["codes"], None, 0, 2)[0]) < len(listed_sites(al["codes"], None, 0, 1)[0]) and one != two
    assert run(["--ld", "0.1", "--ld-min-count", "2", al["fasta"]]) == two
    assert run(["--ld", "0.1", "--ld-min-count", "1", al["fasta"]]) == one
    nothing = run(["--ld", "0.1", "--ld-min-count", "30", al["fasta"]])
    assert nothing == ld_text(al["codes"], 0.1, 30, fmt=fmt) and nothing.count("\n") == 1


@pytest.mark.parametrize("r2", ["0", "0.5"])
def test_groups(al, r2):
    want = ld_text(al["codes"], float(r2), 1, al["labels"], al["names"], fmt=fmt)
    assert len(listed_sites(al["codes"], al["labels"], 2, 1)[0]) == 1   # group y: the header's lines only from z and x
    assert "\tz\t" in want and "\tx\t" in want and "\ty\t" not in want
    assert run(["--ld", r2, "--ld-groups", al["labels_file"], al["fasta"]]) == want
    assert run(["--ld", r2, "--ld-groups", al["labels_file"], "--slab-pairs", "50", al["fasta"]]) == want
