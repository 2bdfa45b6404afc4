"""GPU (-m gpu): `distance --matrix tsv|phylip` end to end.  The expected bytes come from the CLI's own long output of
the same input (tested against the reference elsewhere): cell (i, j) is the line of the canonical pair, the diagonal
the measure of a record against itself (oracle.pair_distance, formatted as the long output formats)."""
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
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def fasta(codes, prefix):
    lut = {int(c): chr(LETTERS[k]) for k, c in enumerate(CODES)}
    ids = [f"{prefix}{r}" for r in range(len(codes))]
    text = "".join(f">{i} description\n" + "".join(lut[int(c)] for c in row) + "\n" for i, row in zip(ids, codes))
    return ids, text.encode()


def run(args, env=None, stdin=None):
    r = subprocess.run([CLI] + args, capture_output=True, input=stdin, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.stderr.decode())
    return r.stdout


def long_values(out):
    lines = out.split(b"\n")[1:-1]   # (the long output's header line)
    return [line.rsplit(b"\t", 1)[1] for line in lines]


def expected_square(measure, codes, ids, long_out, style):
    n = len(codes)
    cells = np.empty((n, n), dtype=object)
    iu = np.triu_indices(n, 1)
    for i, j, v in zip(iu[0], iu[1], long_values(long_out)):
        cells[i, j] = cells[j, i] = v
    for i in range(n):
        v = oracle.pair_distance("n_high" if measure == "n" else measure, codes[i], codes[i])
        cells[i, i] = da.format_distance(measure, v).encode()
    sep = b"\t" if style == "tsv" else b" "
    head = (b"".join(b"\t" + i.encode() for i in ids) + b"\n") if style == "tsv" else b"%d\n" % n
    return head + b"".join(ids[i].encode() + b"".join(sep + c for c in cells[i]) + b"\n" for i in range(n))


@pytest.fixture(scope="module")
def one_file(tmp_path_factory):
    codes = random_alignment(150, 800, seed=61)
    codes[7, :] = 240   # a record with no resolved site
    ids, text = fasta(codes, "s")
    p = tmp_path_factory.mktemp("m") / "a.fasta"
    p.write_bytes(text)
    return codes, ids, p, text


@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("style", ["tsv", "phylip"])
def test_square(one_file, measure, style):
    codes, ids, path, _ = one_file
    long_out = run(["-m", measure, str(path)])
    got = run(["-m", measure, "--matrix", style, str(path)])
    assert got == expected_square(measure, codes, ids, long_out, style)


def test_two_files_tsv(tmp_path):
    a = random_alignment(60, 500, seed=1)
    b = random_alignment(170, 500, seed=2)
    ia, ta = fasta(a, "a")
    ib, tb = fasta(b, "b")
    (tmp_path / "a.fasta").write_bytes(ta)
    (tmp_path / "b.fasta").write_bytes(tb)
    for measure in ("raw", "tn93", "n"):
        vals = long_values(run(["-m", measure, str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")]))
        want = b"".join(b"\t" + i.encode() for i in ib) + b"\n"
        want += b"".join(ia[i].encode() + b"".join(b"\t" + v for v in vals[i * 170:(i + 1) * 170]) + b"\n" for i in range(60))
        got = run(["-m", measure, "--matrix=tsv", str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")])
        assert got == want, measure
        assert run(["-m", measure, "--matrix", "tsv", "--slab-pairs", "700", str(tmp_path / "a.fasta"),
                    str(tmp_path / "b.fasta")], env={"DISTANCE_HOST_FORMAT": "1"}) == want, measure


def test_stdin_output_host_format_and_slabs(one_file, tmp_path):
    codes, ids, path, text = one_file
    for measure in ("raw", "jc69", "tn93"):
        want = expected_square(measure, codes, ids, run(["-m", measure, str(path)]), "tsv")
        assert run(["-m", measure, "--matrix", "tsv"], stdin=text) == want
        out = tmp_path / "m.tsv"
        assert run(["-m", measure, "--matrix", "tsv", "-o", str(out), str(path)]) == b""
        assert out.read_bytes() == want
        assert run(["-m", measure, "--matrix", "tsv", str(path)], env={"DISTANCE_HOST_FORMAT": "1"}) == want
        assert run(["-m", measure, "--matrix", "tsv", "--devices", "0,0,0", "--slab-pairs", "500", "-t", "4",
                    str(path)]) == want
        assert run(["-m", measure, "--matrix", "tsv", "--slab-pairs", "1", str(path)]) == want
