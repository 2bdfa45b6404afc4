"""GPU (-m gpu): the command-line tool on the designed set of record_boundary_cases.py (92,700 records, 4,296,598,650
pairs): --max-distance with --sites, --clusters, --summary, --histogram, --pairs and --mst, every line against the set's
closed forms.  This reaches the tool's link store, the --sites batching and the id arena at 92,700 ids of mixed length."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import record_boundary_cases as rbc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


@pytest.fixture(scope="module")
def rs():
    return rbc.record_set()


@pytest.fixture(scope="module")
def fasta(rs, tmp_path_factory):
    path = tmp_path_factory.mktemp("record_boundary") / "set.fasta"
    ids = rs.write_fasta(path)
    return ids, str(path)


def run(args):
    r = subprocess.run([CLI] + args, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def assert_same_lines(got, want):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        assert len(g) == len(w), (len(g), len(w))
        k = next(k for k in range(len(w)) if g[k] != w[k])
        assert g[k] == w[k], k


def test_max_distance_with_sites(rs, fasta):
    ids, path = fasta
    i, j, _ = rs.links_within(1)
    want = "sequence1\tsequence2\tdistance\tsites\n" + "".join(
        f"{ids[a]}\t{ids[b]}\t1\t{rs.site_field(a, b)}\n" for a, b in zip(i.tolist(), j.tolist()))
    assert want.count("\n") == 1 + 81_846
    assert_same_lines(run(["-m", "n", "--max-distance", "1", "--sites", path]), want)


def test_clusters(rs, fasta):
    ids, path = fasta
    labels = rs.clusters(1)
    number, lines = {}, ["sequence\tcluster\n"]
    for r, lab in enumerate(labels.tolist()):
        if lab == r:
            number[r] = len(number) + 1
        lines.append(f"{ids[r]}\t{number[lab]}\n")
    assert len(number) == 18_857
    assert_same_lines(run(["-m", "n", "--clusters", "1", path]), "".join(lines))


def test_summary(rs, fasta):
    ids, path = fasta
    i, j, _ = rs.links_within(1)
    within, sums = rs.within(i, j), rs.sums().astype(np.float64)
    compared = rs.n - 1
    want = "sequence\twithin\tcompared\tmean\n" + "".join(
        f"{ids[r]}\t{int(within[r])}\t{compared}\t{oracle.format_distance(float(sums[r] / compared))}\n" for r in range(rs.n))
    assert_same_lines(run(["-m", "n", "--summary", "1", path]), want)


def test_histogram(rs, fasta):
    _, path = fasta
    hist = np.zeros(32, np.uint64)
    hist[:rbc.BITS + 1] = rs.histogram()
    want = "distance\tpairs\n" + "".join(f"{b}\t{int(c)}\n" for b, c in enumerate(hist)) + "NaN\t0\n"
    assert run(["-m", "n", "--histogram", "1", "--bins", "32", path]) == want


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_pairs(rs, fasta, measure, tmp_path):
    """--pairs FILE naming the pairs at record 65,536 and at offset 2^32 by id, in both orders: a line per line of the
    file, the ids as given"""
    ids, path = fasta
    n, F = rs.n, rbc.FIRST_ROW_PAST_2_32
    pairs = [(65_535, 65_536), (65_536, n - 1), (F - 1, F), (F, n - 1), (n - 2, n - 1)]
    assert rbc.canon(n, *pairs[-1]) == 4_296_598_649 and rbc.canon(n, *pairs[2]) < rbc.TWO32 <= rbc.canon(n, *pairs[3])
    pairs = pairs + [(b, a) for a, b in pairs]
    listed = tmp_path / "pairs.tsv"
    listed.write_text("".join(f"{ids[a]}\t{ids[b]}\n" for a, b in pairs))
    values = rs.values(measure, [a for a, _ in pairs], [b for _, b in pairs]).tolist()
    want = "sequence1\tsequence2\tdistance\n" + "".join(
        f"{ids[a]}\t{ids[b]}\t{oracle.format_distance(v)}\n" for (a, b), v in zip(pairs, values))
    assert_same_lines(run(["-m", measure, "--pairs", str(listed), path]), want)


def test_mst(rs, fasta):
    ids, path = fasta
    edges, values, _ = rs.mst()
    want = "sequence1\tsequence2\tdistance\n" + "".join(
        f"{ids[a]}\t{ids[b]}\t{v}\n" for (a, b), v in zip(edges.tolist(), values.tolist()))
    assert want.count("\n") == rs.n
    assert_same_lines(run(["-m", "n", "--mst", path]), want)
