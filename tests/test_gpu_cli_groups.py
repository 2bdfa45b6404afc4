"""GPU (-m gpu): `distance --groups FILE [--groups-within T] [--per-record]` end to end against Engine.group_summary
formatted in Python: one and two inputs, -o, stdin, any slab bound, groups numbered by first record, skipped ids,
duplicate ids, and the label file's errors."""
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
N, NB = 90, 17
NAMES = ("delta", "alpha", "omicron lineage")   # in order of first record; the label file lists them in another order


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(args, stdin=None, warning=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    if warning is None:
        assert b"warning:" not in r.stderr, r.stderr
    else:
        assert r.stderr.decode().count(warning) == 1 and r.stderr.count(b"warning:") == 1, r.stderr
    return r.stdout.decode()


def labels_of(n):
    """record r in group r mod 3 (named NAMES), every 8th record (from 4) without a label"""
    g = np.arange(n) % 3
    g[4::8] = -1
    return g


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    codes = random_alignment(N, 400, seed=86)
    codes[6] = codes[3]   # identical records of one group: min 0
    codes[9] = 240        # a record without a resolved site (group 0): NaN against everything
    d = tmp_path_factory.mktemp("groups")
    write_fasta(d / "a.fasta", "a", codes)
    write_fasta(d / "b.fasta", "b", codes[:NB])
    ga, gb = labels_of(N), labels_of(NB)
    lines = [f"a{r}\t{NAMES[ga[r]]}\n" for r in range(N) if ga[r] >= 0] + [f"b{r}\t{NAMES[gb[r]]}\n" for r in range(NB) if gb[r] >= 0]
    # the file's order is not the records': groups are still numbered by their first record
    (d / "g.tsv").write_text("".join(reversed(lines[:40])) + "\n" + "".join(lines[40:]))
    (d / "ga.tsv").write_text("".join(x for x in lines if x.startswith("a")))
    return codes, str(d / "a.fasta"), str(d / "b.fasta"), str(d / "g.tsv"), str(d / "ga.tsv")


def fmt(measure, known, value):
    return da.format_distance(measure, value) if known else "NaN"


def cells_text(measure, s, names_r, names_c, square, within):
    out = "group1\tgroup2\tpairs\tcompared" + ("\twithin" if within else "") + "\tmean\tmin\tmax\n"
    for a, ra in enumerate(names_r):
        for b, cb in enumerate(names_c):
            if square and b < a:
                continue
            c = int(s["summable_pairs"][a, b])
            known = int(s["pairs"][a, b]) > int(s["nan_pairs"][a, b])
            out += f"{ra}\t{cb}\t{int(s['pairs'][a, b])}\t{c}" + (f"\t{int(s['links'][a, b])}" if within else "")
            out += f"\t{fmt('raw', c > 0, s['sum'][a, b] / c if c else 0.0)}"
            out += f"\t{fmt(measure, known, s['min'][a, b])}\t{fmt(measure, known, s['max'][a, b])}\n"
    return out


def records_text(ids, s, names_c, within):
    out = "sequence\tgroup\tcompared" + ("\twithin" if within else "") + "\tmean\n"
    for x, name in enumerate(ids):
        for g, cg in enumerate(names_c):
            c = int(s["rec_summable"][x, g])
            out += f"{name}\t{cg}\t{c}" + (f"\t{int(s['rec_within'][x, g])}" if within else "")
            out += f"\t{fmt('raw', c > 0, s['rec_sum'][x, g] / c if c else 0.0)}\n"
    return out


@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_one_input(alignment, tmp_path, measure):
    codes, fasta, _, groups, groups_a = alignment
    ids = [f"a{r}" for r in range(N)]
    g = labels_of(N)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square(measure)
        finite = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
        t = float(np.quantile(finite, 0.3))
        text = str(int(t)) if measure in da.INT_MEASURES else repr(t)
        plain = eng.group_summary(measure, g, 3, per_record=True)
        cut = eng.group_summary(measure, g, 3, float(text), per_record=True)
    want = cells_text(measure, plain, NAMES, NAMES, True, False)
    assert want.count("\n") == 1 + 6 and want.splitlines()[1].startswith("delta\tdelta\t")
    if measure == "tn93":
        assert plain["nan_pairs"][0].sum() > 0 and plain["min"][0, 0] == 0.0   # the all-N record; the identical pair
    skipped = "warning: --groups: 15 ids of"   # the second input's labels are in the file too
    assert run(["-m", measure, "--groups", groups, fasta], warning=skipped) == want
    assert run(["-m", measure, "--groups", groups_a, fasta]) == want
    assert run(["-m", measure, f"--groups={groups_a}", "--slab-pairs", "1", "-t", "2", fasta]) == want
    want_cut = cells_text(measure, cut, NAMES, NAMES, True, True)
    assert run(["-m", measure, "--groups", groups_a, "--groups-within", text, fasta]) == want_cut
    assert want_cut != cells_text(measure, plain, NAMES, NAMES, True, True)   # (the threshold matters)
    assert run(["-m", measure, "--groups", groups_a, "--per-record", fasta]) == records_text(ids, plain, NAMES, False)
    assert run(["-m", measure, "--groups", groups_a, "--per-record", f"--groups-within={text}", fasta]) == records_text(ids, cut, NAMES, True)
    out = tmp_path / "out.tsv"
    assert run(["-m", measure, "--groups", groups_a, "-o", str(out), fasta]) == "" and out.read_text() == want
    with open(fasta, "rb") as fh:
        assert run(["-m", measure, "--groups", groups_a], stdin=fh) == want


@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_two_inputs(alignment, measure):
    codes, fasta_a, fasta_b, groups, _ = alignment
    ga, gb = labels_of(N), labels_of(NB)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(codes[:NB]))
        s = eng.group_summary(measure, ga, 3, 2.0 if measure == "n" else 0.04, square=False, col_groups=gb, n_col_groups=3, per_record=True)
        back = eng.group_summary(measure, gb, 3, square=False, row_slot=1, col_slot=0, col_groups=ga, n_col_groups=3)
    t = "2" if measure == "n" else "0.04"
    want = cells_text(measure, s, NAMES, NAMES, False, True)
    assert want.count("\n") == 1 + 9
    assert run(["-m", measure, "--groups", groups, "--groups-within", t, fasta_a, fasta_b]) == want
    assert run(["-m", measure, "--groups", groups, "--groups-within", t, "--slab-pairs", "40", "-i", fasta_a, fasta_b]) == want
    assert run(["-m", measure, "--groups", groups, "--groups-within", t, "--per-record", fasta_a, fasta_b]) == \
        records_text([f"a{r}" for r in range(N)], s, NAMES, True)
    assert run(["-m", measure, "--groups", groups, fasta_b, fasta_a]) == cells_text(measure, back, NAMES, NAMES, False, False)


def test_group_order_and_duplicate_ids(tmp_path):
    """Groups are numbered by their first record in input order, per input; every record with a listed id gets the group."""
    codes = random_alignment(6, 60, seed=87, divergence=0.3)
    write_fasta(tmp_path / "plain.fasta", "r", codes)
    rows = open(tmp_path / "plain.fasta").read().splitlines()[1::2]
    names = ["s0", "s1", "dup", "s3", "dup", "s5"]   # records 2 and 4 share an id
    (tmp_path / "a.fasta").write_text("".join(f">{names[k]}\n{rows[k]}\n" for k in range(6)))
    (tmp_path / "b.fasta").write_text("".join(f">{names[k]}\n{rows[k]}\n" for k in (5, 1)))
    (tmp_path / "g.tsv").write_text("s5\tzeta\ns1\tbeta\ndup\tzeta\ns0\tmid\nghost\tbeta\n")
    ga = np.array([0, 1, 2, -1, 2, 2])    # mid, beta, zeta by first record; s3 has no label
    gb = np.array([0, 1])                 # the second input: zeta (s5) first, then beta (s1)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(codes[[5, 1]]))
        one = eng.group_summary("raw", ga, 3, per_record=True)
        two = eng.group_summary("raw", ga, 3, square=False, col_groups=gb, n_col_groups=2)
    warn = "warning: --groups: 1 ids of"
    a, b, g = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta"), str(tmp_path / "g.tsv")
    assert one["pairs"][2, 2] == 3   # dup, dup, s5
    assert run(["--groups", g, a], warning=warn) == cells_text("raw", one, ("mid", "beta", "zeta"), ("mid", "beta", "zeta"), True, False)
    assert run(["--groups", g, "--per-record", a], warning=warn) == records_text(names, one, ("mid", "beta", "zeta"), False)
    assert run(["--groups", g, a, b], warning=warn) == cells_text("raw", two, ("mid", "beta", "zeta"), ("zeta", "beta"), False, False)


def test_label_errors_with_a_device(tmp_path):
    codes = random_alignment(4, 40, seed=88)
    write_fasta(tmp_path / "a.fasta", "a", codes)
    a = str(tmp_path / "a.fasta")
    (tmp_path / "g.tsv").write_text("a0\tx\na1\ty\na0\ty\n")
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), a], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"line 3 of" in r.stderr and b"gives 'a0' the group 'y', line 1 gave it 'x'" in r.stderr
    n = 1025
    write_fasta(tmp_path / "big.fasta", "r", np.repeat(codes[:1], n, axis=0))
    (tmp_path / "g.tsv").write_text("".join(f"r{k}\tg{k}\n" for k in range(n)))
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "big.fasta")], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"line 1025 of" in r.stderr and b"more than 1024 groups" in r.stderr
    (tmp_path / "g.tsv").write_text("".join(f"r{k}\tg{k % 1024}\n" for k in range(n)))
    out = run(["-m", "n", "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "big.fasta")])
    assert out.count("\n") == 1 + 1024 * 1025 // 2 and out.splitlines()[1].startswith("g0\tg0\t1\t1\t")
    (tmp_path / "g.tsv").write_text("nobody\tx\n")
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), a], capture_output=True)
    assert r.returncode == 1 and b"no record of the first input has a group" in r.stderr
