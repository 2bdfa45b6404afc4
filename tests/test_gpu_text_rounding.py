"""GPU (-m gpu): exact ties of the 12th decimal and two-digit values through every `{:.12}` text writer.

The designed sets of text_rounding_cases.py (whose tallies test_text_rounding_host.py asserts on the oracle alone):
  * the tie set: pairs (0, k) with raw = a / 8192, a odd (v x 10^12 ends in exactly .5: the only values whose last digit
    the `tie && (R & 1)` branch decides), the same values through 16,384 and 24,576 sites, controls one count either
    side, 0 and 1.  raw is no near-tie measure: the device's digits are final.  The expectation is the exact quotient in
    decimal arithmetic (tr.expected_field), not a formatter.
  * the long set: jc69 = 10.18 over 262,143 sites, a text of 15 characters (no other test prints more than 14), in the
    32-bit tally form, next to 8.97, NaN and 3.8e-6.  The expectation is "%.12f" of the oracle's value.

Through put_fixed12 (number_kernel: text_square / text_rect; matrix_kernel: text_matrix, both styles, rows that cross
the 256-cell chunk, ids of every length so that numbers start at every offset modulo 16), patch_near_ties (the long
set's jc69), dst_format_distance (nearest, --nearest, --mst, --max-distance) and cli::fmt_fixed12 (stream mode on both
wire formats, DISTANCE_HOST_FORMAT=1).  Only row ranges that hold record 0 are formatted, never the tie set's triangle."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import distance_amd as da
import oracle
import text_rounding_cases as tr
from helpers import CODES, LETTERS
from mst_reference import kruskal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
THREADS = min(16, len(os.sched_getaffinity(0)))
HEADER = b"sequence1\tsequence2\tdistance\n"
SEP = {"tsv": b"\t", "phylip": b" "}
ROWS = 3                   # record 0 and two more rows


def field(v):
    """`{:.12}` of an oracle value, as tests/test_gpu_text.py builds it"""
    v = float(v)
    if np.isnan(v):
        return b"NaN"
    if np.isinf(v):
        return b"-inf" if v < 0 else b"inf"
    return b"%.12f" % v


def long_lines(ids_a, ids_b, cells, rows, square):
    """the long text of rows `rows` of a cell matrix: (i, j > i) of a square, else every column"""
    return b"".join(ids_a[i].encode() + b"\t" + ids_b[j].encode() + b"\t" + cells[i][j] + b"\n"
                    for i in rows for j in range(i + 1 if square else 0, len(ids_b)))


def matrix_rows(ids, cells, rows, style):
    return b"".join(ids[i].encode() + b"".join(SEP[style] + c for c in cells[i]) + b"\n" for i in rows)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ties():
    """the tie set and its expected cells: rows 0 .. ROWS - 1 against every record; row 0 and column 0 by the decimal
    expectation of the designed (n, d), the other cells of rows 1 .. by "%.12f" of the oracle's value"""
    codes, cases, ids = tr.tie_alignment()
    c = SimpleNamespace(codes=codes, cases=cases, ids=ids, n=len(codes))
    c.designed = [tr.expected_field(0, tr.TIE_L).encode()] + [tr.expected_field(n, d).encode() for n, d in cases]
    vals = oracle.all_pairs_rect("raw", codes[:ROWS], codes, threads=THREADS)
    c.cells = [[field(v) for v in row] for row in vals]
    assert c.cells[0] == c.designed                               # (the host test's claim, on this machine's libc)
    c.cells[0] = list(c.designed)
    for i in range(1, ROWS):
        c.cells[i][0] = c.designed[i]
    c.jc69 = oracle.all_pairs_square("jc69", codes, pair_range=(0, c.n - 1), threads=THREADS)
    return c


@pytest.fixture(scope="module")
def long_set():
    codes, cases, ids = tr.long_jc69_alignment()
    c = SimpleNamespace(codes=codes, cases=cases, ids=ids, n=len(codes))
    c.values = oracle.all_pairs_square("jc69", codes, threads=THREADS)
    c.cells = np.empty((c.n, c.n), dtype=object)
    iu = np.triu_indices(c.n, 1)
    for i, j, v in zip(iu[0], iu[1], c.values):
        c.cells[i, j] = c.cells[j, i] = field(v)
    for i in range(c.n):
        c.cells[i, i] = field(oracle.pair_distance("jc69", codes[i], codes[i]))
    assert c.cells[0, 1].startswith(b"10.18") and len(c.cells[0, 1]) == 15 and c.cells[0, 3] == b"NaN"
    return c


@pytest.mark.parametrize("path", ["dense", "auto"])
def test_exact_ties_of_raw_in_every_device_text(eng, ties, path):
    c = ties
    n, ids = c.n, c.ids
    eng.set_path("auto")
    eng.upload(0, c.codes)
    eng.set_ids(0, ids)
    eng.upload(1, c.codes[:1])
    eng.set_ids(1, ["the_root"])
    eng.set_path(path)
    try:
        stats = eng.text_stats()
        tl = eng.run_square("raw", 0, 1, tallies=True)
        assert [tuple(int(x) for x in t) for t in tl] == c.cases, path
        if path == "dense":
            assert eng.last_path() == "dense"
        # the long text: row 0 whole, rows 0 .. 2 in one call and cut into two
        want0 = long_lines(ids, ids, c.cells, [0], True)
        got0 = eng.text_square("raw", 0, 1)
        bad = [(g, w) for g, w in zip(got0.split(b"\n"), want0.split(b"\n")) if g != w]
        assert got0 == want0, (path, len(bad), bad[:4])
        want = long_lines(ids, ids, c.cells, range(ROWS), True)
        assert eng.text_square("raw", 0, ROWS) == want, path
        assert eng.text_square("raw", 0, 1) + eng.text_square("raw", 1, ROWS) == want, path
        # the rectangle against the root alone, both slot orders, ids swapped
        col = [[v] for v in c.designed]
        assert eng.text_rect("raw", 0, 1, 0, n) == long_lines(ids, ["the_root"], col, range(n), False), path
        assert eng.text_rect("raw", 0, 1, 0, n, swap_ids=True) == b"".join(
            b"the_root\t" + ids[k].encode() + b"\t" + c.designed[k] + b"\n" for k in range(n)), path
        assert eng.text_rect("raw", 1, 0, 0, 1) == long_lines(["the_root"], ids, [c.designed], [0], False), path
        assert eng.text_rect("raw", 1, 0, 0, 1, swap_ids=True) == b"".join(
            ids[k].encode() + b"\tthe_root\t" + c.designed[k] + b"\n" for k in range(n)), path
        # the matrix: rows 0 .. 2, whole and cut; column 0 of rows 1 .. is the mirrored cell
        for style in ("tsv", "phylip"):
            want = matrix_rows(ids, c.cells, range(ROWS), style)
            got = eng.text_matrix("raw", 0, ROWS, style=style)
            if got != want:
                g, w = got.split(b"\n")[0].split(SEP[style]), want.split(b"\n")[0].split(SEP[style])
                bad = [(k, a, b) for k, (a, b) in enumerate(zip(g, w)) if a != b]
                assert False, (path, style, len(g), len(w), len(bad), bad[:4])
            assert eng.text_matrix("raw", 0, 1, style=style) + eng.text_matrix("raw", 1, ROWS, style=style) == want, (path, style)
        mirrored = eng.text_matrix("raw", 1, ROWS).split(b"\n")
        assert [line.split(b"\t")[1] for line in mirrored[:-1]] == c.designed[1:ROWS]
        assert eng.text_stats() == stats, "raw notes no near tie"
        # the same upload through the tally source (jc69 finalised in the text kernel): an ordinary case
        assert eng.text_square("jc69", 0, 1) == oracle.tsv_square("jc69", c.jc69, ids, 0, 1), path
    finally:
        eng.set_path("auto")


def test_a_two_digit_jc69_in_every_device_text(eng, long_set):
    c = long_set
    n, ids = c.n, c.ids
    eng.set_path("auto")
    eng.upload(0, c.codes)
    eng.set_ids(0, ids)
    tl = eng.run_square("jc69", 0, 1, tallies=True)
    assert [tuple(int(x) for x in t) for t in tl] == c.cases
    want = long_lines(ids, ids, c.cells, range(n), True)
    assert oracle.tsv_square("jc69", c.values, ids) == want
    assert eng.text_square("jc69", 0, n) == want
    assert eng.text_square("jc69", 0, 1) + eng.text_square("jc69", 1, n) == want
    for style in ("tsv", "phylip"):
        assert eng.text_matrix("jc69", style=style) == matrix_rows(ids, c.cells, range(n), style), style
    # record 0's neighbours, finalised and formatted on the host: the same fields
    idx, vals, ntl = eng.nearest("jc69", 4, tallies=True)
    assert sorted(int(j) for j in idx[0]) == [1, 2, 3, 4] and [int(j) for j in idx[0][:3]] == [4, 2, 1]   # NaN last
    for j, t in zip(idx[0], ntl[0]):
        assert tuple(int(x) for x in t) == c.cases[int(j) - 1]
        assert da.format_distance("jc69", da.finalize("jc69", t)).encode() == c.cells[0, int(j)], int(j)


def write_fasta(path, ids, codes):
    lut = np.zeros(256, np.uint8)
    lut[CODES] = np.frombuffer(LETTERS, np.uint8)
    with open(path, "wb") as fh:
        for i, row in zip(ids, codes):
            fh.write(b">" + i.encode() + b" description\n" + lut[row].tobytes() + b"\n")


def run(args, env=None):
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (args, r.stderr.decode())
    return r.stdout


def of_record_0(out, id0):
    """the lines of a long output whose first id is record 0's"""
    return [line for line in out.split(b"\n")[1:-1] if line.startswith(id0.encode() + b"\t")]


def cli_checks(tmp_path, measure, ids, codes, cells, values, threshold):
    """one set through the CLI.  cells: n x n expected texts (diagonal included); values: the condensed square (what
    orders --nearest and --mst, where NaN comes last)"""
    n = len(ids)
    fa, fr = str(tmp_path / "set.fasta"), str(tmp_path / "root.fasta")
    write_fasta(fa, ids, codes)
    write_fasta(fr, ids[:1], codes[:1])
    want = HEADER + long_lines(ids, ids, cells, range(n), True)
    got = run(["-m", measure, fa])
    bad = [(g, w) for g, w in zip(got.split(b"\n"), want.split(b"\n")) if g != w]
    assert got == want, (len(bad), bad[:4])
    assert run(["-m", measure, fa], env={"DISTANCE_HOST_FORMAT": "1"}) == want
    assert run(["-m", measure, "--matrix", "phylip", fa]) == b"%d\n" % n + matrix_rows(ids, cells, range(n), "phylip")
    line = {j: ids[0].encode() + b"\t" + ids[j].encode() + b"\t" + cells[0][j] for j in range(1, n)}
    # --nearest: record 0's five (or all) nearest by (value, index)
    full = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    full[iu] = values
    key = [(np.inf if np.isnan(full[0, j]) else full[0, j], np.isnan(full[0, j]), j) for j in range(1, n)]
    k_near = min(5, n - 1)
    nearest = [j for _, _, j in sorted(key)[:k_near]]
    assert of_record_0(run(["-m", measure, "--nearest", str(k_near), fa]), ids[0]) == [line[j] for j in nearest]
    # --mst: record 0's edges of the reference forest, in its order
    edges, _ = kruskal(n, values)
    mine = [int(j) for i, j in edges if i == 0]
    assert mine and of_record_0(run(["-m", measure, "--mst", fa]), ids[0]) == [line[j] for j in mine]
    # --max-distance
    linked = [j for j in range(1, n) if full[0, j] <= threshold]
    assert len(linked) >= 3
    assert of_record_0(run(["-m", measure, "--max-distance", repr(threshold), fa]), ids[0]) == [line[j] for j in linked]
    # stream mode (cli::fmt_fixed12 on the host): the set against the loaded root, both wire formats
    want = HEADER + b"".join(ids[0].encode() + b"\t" + ids[j].encode() + b"\t" + cells[0][j] + b"\n" for j in range(n))
    assert run(["-m", measure, "-i", fr, "-s", fa]) == want
    assert run(["-m", measure, "-i", fr, "-s", fa], env={"DISTANCE_WIRE": "codes"}) == want


def test_exact_ties_of_raw_through_the_cli(tmp_path, ties):
    """the root and the d = 8,192 records (255 of them, 6 MB of FASTA): the whole triangle of that subset"""
    sub = tr.cli_subset(ties.cases)
    n = len(sub)
    codes = np.ascontiguousarray(ties.codes[sub])
    ids = ["s%d" % k if i == "" else i for k, i in zip(sub, (ties.ids[k] for k in sub))]   # a FASTA header needs an id
    values = oracle.all_pairs_square("raw", codes, threads=THREADS)
    cells = np.empty((n, n), dtype=object)
    iu = np.triu_indices(n, 1)
    for i, j, v in zip(iu[0], iu[1], values):
        cells[i, j] = cells[j, i] = field(v)
    for i in range(n):
        cells[i, i] = b"0.000000000000"
    for j, k in enumerate(sub):
        assert cells[0, j] == ties.designed[k]                  # (the host test's claim, on this machine's libc)
        cells[0, j] = cells[j, 0] = ties.designed[k]
    up = [j for j, k in enumerate(sub) if k and tr.rounds_up(*ties.cases[k - 1])]
    stay = [j for j, k in enumerate(sub) if k and tr.is_tie(*ties.cases[k - 1]) and j not in up]
    assert len(up) >= 80 and len(stay) >= 80
    cli_checks(tmp_path, "raw", ids, codes, cells, values, 0.001)


def test_a_two_digit_jc69_through_the_cli(tmp_path, long_set):
    c = long_set
    cli_checks(tmp_path, "jc69", c.ids, c.codes, c.cells, c.values, 11.0)
