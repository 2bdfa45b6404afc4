"""GPU (-m gpu): `distance --windows W [--step S] | --regions FILE --window-groups FILE [--window-groups-within T]
[--window-groups-by cell|record]`, end to end on an upper-case FASTA with ambiguity letters: per window the lines are, byte
for byte, the plain run's window fields and then what `distance --groups FILE` prints on the FASTA cut to the window's
columns.  One and two inputs, --windows and --regions, a region in which nothing can be compared, -o, stdin and the warning
for ids that are in no input."""
import os
import subprocess

import pytest

from helpers import CODES, LETTERS, random_alignment
from window_reference import sliding

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
N, NB, L = 30, 5, 260
N_CODE = 240
BLANK = (150, 160)   # columns that hold N in every record: a region inside them compares nothing
REGIONS = [("whole", 1, 260), ("orf1", 10, 140), ("blank", 151, 160), ("one", 129, 129), ("orf1", 10, 140)]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def write_fasta(path, prefix, codes):
    lut = {int(c): chr(LETTERS[k]).upper() for k, c in enumerate(CODES)}
    with open(path, "w") as fh:
        for r, row in enumerate(codes):
            fh.write(f">{prefix}{r} description\n" + "".join(lut[int(c)] for c in row) + "\n")


def run(args, stdin=None, stderr=None):
    r = subprocess.run([CLI] + args, capture_output=True, stdin=stdin)
    assert r.returncode == 0, r.stderr.decode()
    if stderr is not None:
        stderr.append(r.stderr.decode())
    return r.stdout.decode()


@pytest.fixture(scope="module")
def alignment(tmp_path_factory):
    a = random_alignment(N, L, seed=77, divergence=0.05, p_ambig=0.03, p_gap=0.02)
    b = random_alignment(NB, L, seed=78, divergence=0.05, p_ambig=0.03, p_gap=0.02, root=a[0])
    a[:, BLANK[0]:BLANK[1]] = N_CODE
    b[:, BLANK[0]:BLANK[1]] = N_CODE
    d = tmp_path_factory.mktemp("window_groups")
    write_fasta(d / "a.fasta", "a", a)
    write_fasta(d / "b.fasta", "b", b)
    with open(d / "regions.tsv", "w") as fh:
        fh.write("".join(f"{name}\t{first}\t{last}\n" for name, first, last in REGIONS))
    with open(d / "labels.tsv", "w") as fh:   # three groups in a, two of them in b; a6, a13, a20, a27 and b4 have none
        fh.write("".join(f"a{i}\t{'xyz'[i % 3]}\n" for i in range(N) if i % 7 != 6))
        fh.write("".join(f"b{i}\t{'yx'[i % 2]}\n" for i in range(NB - 1)))
    return {"a": a, "b": b, "dir": d}


def window_fields(plain, nw):
    """(window, start, end) of the plain run's first nw lines: its first pair, every window in the given order"""
    lines = plain.splitlines()[1:1 + nw]
    return ["\t".join(x.split("\t")[2:5]) for x in lines]


def expected(al, measure, windows, fields, two, within, tag):
    """both forms' text: the window fields and `distance --groups` on the FASTA cut to each window's columns"""
    d = al["dir"]
    labels = str(d / "labels.tsv")
    extra = ["--groups-within", within] if within else []
    by_cell, per, seen = [], [], {}
    for w, (lo, hi) in enumerate(windows):
        if (lo, hi) not in seen:   # (a repeated region: the same cut, run once)
            cut = [str(d / f"{tag}_{w}_a.fasta")] + ([str(d / f"{tag}_{w}_b.fasta")] if two else [])
            write_fasta(cut[0], "a", al["a"][:, lo:hi])
            if two:
                write_fasta(cut[1], "b", al["b"][:, lo:hi])
            seen[lo, hi] = (run(["-m", measure, "--groups", labels] + extra + cut).splitlines(),
                            run(["-m", measure, "--groups", labels, "--per-record"] + extra + cut).splitlines())
        cells, records = seen[lo, hi]
        assert cells[0] == "group1\tgroup2\tpairs\tcompared" + ("\twithin" if within else "") + "\tmean\tmin\tmax"
        assert records[0] == "sequence\tgroup\tcompared" + ("\twithin" if within else "") + "\tmean"
        by_cell += [fields[w] + "\t" + line for line in cells[1:]]
        per.append([line.split("\t", 1) for line in records[1:]])
    head = "window\tstart\tend\tgroup1\tgroup2\tpairs\tcompared" + ("\twithin" if within else "") + "\tmean\tmin\tmax"
    rec_head = "sequence\twindow\tstart\tend\tgroup\tcompared" + ("\twithin" if within else "") + "\tmean"
    groups = len(per[0]) // N   # lines per record
    by_record = [per[w][x * groups + g][0] + "\t" + fields[w] + "\t" + per[w][x * groups + g][1]
                 for x in range(N) for w in range(len(windows)) for g in range(groups)]
    return "\n".join([head] + by_cell) + "\n", "\n".join([rec_head] + by_record) + "\n"


@pytest.mark.parametrize("measure,within", [("n", "4"), ("raw", "0.05"), ("tn93", "0.05")])
@pytest.mark.parametrize("two", [False, True])
def test_sliding_windows(alignment, measure, within, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(int(b), int(e)) for b, e in sliding(L, 128, 100)]
    base = ["--windows", "128", "--step", "100", "-m", measure]
    fields = window_fields(run(base + files), len(windows))
    assert fields[0] == "1\t1\t128" and fields[1] == "2\t101\t228" and len(fields) == len(windows) == 3
    by_cell, by_record = expected(alignment, measure, windows, fields, two, within, f"s_{measure}_{int(two)}")
    mine = ["--window-groups", str(d / "labels.tsv"), "--window-groups-within", within]
    assert run(base + mine + files) == by_cell
    assert run(base + mine + ["--window-groups-by", "record"] + files) == by_record
    # one input prints a <= b, two print every cell
    assert len(by_cell.splitlines()) - 1 == 3 * (3 * 2 if two else 6)


@pytest.mark.parametrize("two", [False, True])
def test_regions_and_a_region_without_a_compared_pair(alignment, two):
    d = alignment["dir"]
    files = [str(d / "a.fasta")] + ([str(d / "b.fasta")] if two else [])
    windows = [(first - 1, last) for _, first, last in REGIONS]
    base = ["--regions", str(d / "regions.tsv"), "-m", "raw"]
    fields = window_fields(run(base + files), len(windows))
    assert fields == [f"{name}\t{first}\t{last}" for name, first, last in REGIONS]
    by_cell, by_record = expected(alignment, "raw", windows, fields, two, None, f"r_{int(two)}")
    mine = ["--window-groups=" + str(d / "labels.tsv")]
    got = run(base + mine + ["--window-groups-by=cell"] + files)
    assert got == by_cell
    assert run(base + mine + ["--window-groups-by", "record"] + files) == by_record
    # the region of N columns by the definition: every pair is there, none compared, no mean, smallest or largest value
    blank = [x.split("\t") for x in got.splitlines() if x.startswith("blank\t")]
    assert len(blank) == (3 * 2 if two else 6)
    for f in blank:
        assert int(f[5]) > 0 and f[6] == "0" and f[7:] == ["NaN", "NaN", "NaN"], f
    # the two runs of the repeated region are the same lines
    orf = [x for x in got.splitlines() if x.startswith("orf1\t")]
    assert orf[:len(orf) // 2] == orf[len(orf) // 2:]


def test_output_file_stdin_and_the_unknown_id_warning(alignment):
    d = alignment["dir"]
    a = str(d / "a.fasta")
    base = ["--windows", "130", "-m", "raw", "--window-groups", str(d / "labels.tsv")]
    err = []
    got = run(base + [a], stderr=err)
    # (the b records of the label file are in no input here)
    assert err[0] == f"warning: --window-groups: {NB - 1} ids of '{d / 'labels.tsv'}' are not in the input and were skipped\n"
    assert got.splitlines()[0] == "window\tstart\tend\tgroup1\tgroup2\tpairs\tcompared\tmean\tmin\tmax"
    assert len(got.splitlines()) == 1 + 2 * 6
    out = d / "out.tsv"
    assert run(base + ["-o", str(out), a]) == "" and out.read_text() == got
    with open(a, "rb") as fh:
        assert run(base, stdin=fh) == got
    with open(a, "rb") as fh:
        by_record = run(base + ["--window-groups-by", "record"], stdin=fh)
    assert by_record.splitlines()[0] == "sequence\twindow\tstart\tend\tgroup\tcompared\tmean"
    assert len(by_record.splitlines()) == 1 + N * 2 * 3
