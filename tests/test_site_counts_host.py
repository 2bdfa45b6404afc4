"""No GPU: dst_site_counts and dst_site_stats are declared, exported and typed as the header's prototypes; the constants are
the header's; dst_site_stats gives, bit for bit, what site_counts_reference's plain loops give on cases written out by hand
and on a random set; the counts tie the columns to the pairs (the sum over sites of D is the sum over pairs of the oracle's
`n`); and the CLI's usage and label-file errors come before any device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distance_amd as da
import oracle
from distance_amd import _lib
from helpers import CODES, random_alignment
from site_counts_reference import CLASSES, NONE, group_sizes, site_counts, site_stats

ERR_ARG, ERR_CAPACITY = 1, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
A, G, C_, T, R, N, GAP, Q = 136, 72, 40, 24, 192, 240, 244, 242


# ---- the symbols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_args", [("dst_site_counts", 8), ("dst_site_stats", 10)])
def test_declared_exported_and_typed(name, n_args):
    assert name in da.declared_symbols() and hasattr(da.load(), name)
    assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert proto and len(proto.group(1).split(",")) == n_args


def test_constants_and_abi():
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+DST_SITE_CLASSES\s+5\b", text) and da.SITE_CLASSES == _lib.SITE_CLASSES == CLASSES == 5
    m = re.search(r"#define\s+DST_SITE_FLUSH_PERIOD\s+(\d+)u", text)
    assert m and int(m.group(1)) == da.SITE_FLUSH_PERIOD
    m = re.search(r"#define\s+DST_SITE_STRIP_RECORDS\s+(\d+)u", text)
    assert m and int(m.group(1)) == da.SITE_STRIP_RECORDS == 256 * da.SITE_FLUSH_PERIOD
    assert re.search(r"#define\s+DST_ABI_VERSION\s+3\b", text) and da.load().dst_abi_version() == 3
    assert C.sizeof(_lib.SiteWindow) == 48 and [f[0] for f in _lib.SiteWindow._fields_] == [
        "records", "sites", "called", "segregating", "theta_sum", "pi_sum"]
    assert hasattr(da.Engine, "site_counts") and callable(da.site_stats)


def test_null_context_is_err_arg():
    out = np.zeros(16, np.uint32)
    assert da.load().dst_site_counts(None, 0, None, 1, 0, 1, out.ctypes.data, 16) == ERR_ARG


# ---- dst_site_stats ----------------------------------------------------------------------------------------------------
def same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (k, got[k], want[k])


def test_hand_written_sites():
    """one group of 6 records; per site the counts (A, T, G, C, ambiguous):
    0: nothing called (m = 0)    1: one A (m = 1)            2: A and T (m = 2, D = 1, 1 pair)
    3: A A (m = 2, D = 0)        4: A T G C (m = 4, D = 6)   5: only ambiguous codes
    6: A A A T T (m = 5, D = 6, 10 pairs)"""
    counts = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [2, 0, 0, 0, 3], [1, 1, 1, 1, 2], [0, 0, 0, 0, 6],
                       [3, 2, 0, 0, 0]], np.uint32).reshape(7, 1, CLASSES)
    windows = [(0, 7), (0, 2), (2, 3), (3, 3), (4, 7), (2, 7), (2, 7), (6, 7), (0, 1)]
    got = da.site_stats(counts, windows, [6])
    same(got, site_stats(counts, windows, [6]))
    assert got["records"][:, 0].tolist() == [6] * 9 and got["sites"][:, 0].tolist() == [7, 2, 1, 0, 3, 5, 5, 1, 1]
    assert got["called"][:, 0].tolist() == [4, 0, 1, 0, 2, 4, 4, 1, 0]
    assert got["segregating"][:, 0].tolist() == [3, 0, 1, 0, 2, 3, 3, 1, 0]
    h1, h3, h4 = 1.0, 1.0 + 1.0 / 2.0 + 1.0 / 3.0, 1.0 + 1.0 / 2.0 + 1.0 / 3.0 + 1.0 / 4.0
    assert got["pi_sum"][0, 0] == ((1.0 / 1.0 + 0.0 / 1.0) + 6.0 / 6.0) + 6.0 / 10.0
    assert got["theta_sum"][0, 0] == (1.0 / h1 + 1.0 / h3) + 1.0 / h4
    assert got["pi_sum"][3, 0] == 0.0 and got["theta_sum"][3, 0] == 0.0 and got["theta_sum"][7, 0] == 1.0 / h4


def test_group_of_size_zero_and_site_begin():
    counts = np.zeros((4, 3, CLASSES), np.uint32)
    counts[:, 0, :4] = [[2, 1, 0, 0], [0, 0, 0, 0], [0, 3, 0, 0], [1, 1, 1, 0]]
    counts[:, 2, :4] = [[1, 0, 0, 0], [0, 0, 1, 1], [5, 5, 5, 5], [0, 0, 0, 2]]
    windows = [(10, 14), (11, 13), (13, 14), (12, 12)]
    got = da.site_stats(counts, windows, [3, 0, 20], site_begin=10)
    same(got, site_stats(counts, windows, [3, 0, 20], site_begin=10))
    assert got["records"].tolist() == [[3, 0, 20]] * 4
    assert not got["called"][:, 1].any() and not got["pi_sum"][:, 1].any() and (got["sites"][:, 1] == [4, 2, 1, 0]).all()


def test_windows_outside_the_range_and_capacity():
    lib = da.load()
    counts = np.ones((5, 2, CLASSES), np.uint32)
    sizes = np.array([5, 5], np.uint64)
    out = (_lib.SiteWindow * 8)()

    def call(wins, begin=20, end=25, cap=8, c=counts, s=sizes, o=out, G=2):
        b, e = np.array([w[0] for w in wins] + [0], np.uint64), np.array([w[1] for w in wins] + [0], np.uint64)
        return lib.dst_site_stats(None if c is None else c.ctypes.data, begin, end, G, b.ctypes.data, e.ctypes.data, len(wins),
                                  None if s is None else s.ctypes.data, None if o is None else C.addressof(o), cap)

    assert call([(20, 25), (22, 22)]) == 0
    for bad in ([(19, 22)], [(20, 26)], [(23, 22)], [(20, 25), (0, 5)], [(25, 26)]):
        assert call(bad) == ERR_ARG
    assert call([(25, 25), (20, 20)]) == 0          # empty windows at the range's ends are inside it
    assert call([(20, 21)] * 4, cap=7) == ERR_CAPACITY and call([(20, 21)] * 4, cap=8) == 0
    assert call([(20, 21)], c=None) == ERR_ARG and call([(20, 21)], s=None) == ERR_ARG and call([(20, 21)], o=None) == ERR_ARG
    assert call([(20, 21)], G=0) == ERR_ARG and call([], begin=5, end=4) == ERR_ARG and call([]) == 0
    with pytest.raises(da.DistanceError) as e:
        da.site_stats(counts, [(0, 6)], sizes)
    assert e.value.status == ERR_ARG


def test_random_set_against_the_reference():
    n, length = 40, 300
    codes = random_alignment(n, length, seed=5, p_ambig=0.1, p_gap=0.2, divergence=0.3)
    g = np.random.default_rng(6).integers(-1, 3, n)
    counts = site_counts(codes, g, 3)
    sizes = group_sizes(g, n, 3)
    assert int(sizes.sum()) == int((g >= 0).sum()) < n
    windows = [(0, 300), (0, 128), (100, 200), (100, 200), (128, 129), (299, 300), (150, 150), (50, 250)]
    same(da.site_stats(counts, windows, sizes), site_stats(counts, windows, sizes))
    part = counts[100:250]
    wins = [(100, 250), (100, 101), (180, 250)]
    same(da.site_stats(part, wins, sizes, site_begin=100), site_stats(counts, wins, sizes))


# ---- columns and pairs --------------------------------------------------------------------------------------------------
def test_sum_of_d_is_the_sum_of_pairwise_n():
    """over {A, C, G, T, N, -, ?} only, a pair differs at a site exactly when both hold a base and the bases differ: the
    sum over sites of D (the pairs of different bases at the site) is the sum over the pairs of the oracle's `n`"""
    n, length = 24, 200
    rng = np.random.default_rng(8)
    codes = np.array([A, C_, G, T, N, GAP, Q], np.uint8)[rng.choice(7, (n, length), p=[.3, .2, .2, .15, .05, .05, .05])]
    g = rng.integers(-1, 3, n)
    counts = site_counts(codes, g, 3).astype(np.int64)
    for a in range(3):
        rows = codes[g == a]
        c = counts[:, a, :4]
        m = c.sum(axis=1)
        d = int(((m * m - (c * c).sum(axis=1)) // 2).sum())
        pairs = oracle.all_pairs_square("n", np.ascontiguousarray(rows))
        assert len(rows) >= 2 and d == int(np.asarray(pairs).sum()), a
        # and pi_sum is that sum with every site divided by its own pairs
        st = da.site_stats(counts.astype(np.uint32), [(0, length)], group_sizes(g, n, 3))
        assert st["called"][0, a] == int((m >= 2).sum())


# ---- the CLI before any device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def files(tmp_path, labels=b"x\tone\ny\ttwo\n"):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACGG\n")
    (tmp_path / "g.tsv").write_bytes(labels)
    (tmp_path / "r.tsv").write_bytes(b"all\t1\t4\n")


def cli(tmp_path, args, labels=b"x\tone\ny\ttwo\n"):
    files(tmp_path, labels)
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")).replace("{g}", str(tmp_path / "g.tsv"))
            .replace("{r}", str(tmp_path / "r.tsv")) for x in args]
    if not any(x.endswith("a.fasta") for x in args):
        args.append(str(tmp_path / "a.fasta"))
    return subprocess.run([CLI] + args, capture_output=True, env=NO_GPU)


def usage(tmp_path, args):
    r = cli(tmp_path, args)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: "), (args, r.stderr)
    return r.stderr.decode()


COUNTS, STATS, SGROUPS = "--site-counts", "--window-site-stats", "--site-groups <FILE>"
OTHERS = [(["--stream", "{b}"], "--stream <stream>"), (["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"),
          (["--representatives", "1"], "--representatives <T>"), (["--max-distance", "4"], "--max-distance <T>"),
          (["--summary", "4"], "--summary <T>"), (["--groups", "{g}"], "--groups <FILE>"), (["--histogram", "2"], "--histogram <W>"),
          (["--matrix", "tsv"], "--matrix <format>"), (["--tree", "nj"], "--tree <method>"), (["--mst"], "--mst"),
          (["--sites"], "--sites"), (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--pairs", "{g}"], "--pairs <FILE>"),
          (["--window-nearest", "2"], "--window-nearest <K>"), (["--window-summary", "1"], "--window-summary <T>"),
          (["--window-summary-by", "record"], "--window-summary-by <what>"), (["--window-groups", "{g}"], "--window-groups <FILE>"),
          (["--window-closest", "2"], "--window-closest <K>"), (["--stream-summary", "1"], "--stream-summary <T>"),
          (["--stream-groups", "{g}"], "--stream-groups <FILE>"), (["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", OTHERS)
def test_usage_errors_with_other_modes(tmp_path, mode, other, first):
    for own, name in ((["--site-counts"], COUNTS), (["--windows", "2", "--window-site-stats"], STATS),
                      (["--regions", "{r}", "--window-site-stats", "--site-groups", "{g}"], STATS)):
        err = usage(tmp_path, own + mode if first else mode + own)
        assert f"the argument '{name}' cannot be used with '{other}'" in err, err
        if "gpus" in other or "devices" in other:
            assert "naming more than one GPU" in err


def test_usage_errors_of_their_own(tmp_path):
    for args, name in ((["--site-counts", "{a}", "{b}"], COUNTS), (["--windows", "2", "--window-site-stats", "{a}", "{b}"], STATS)):
        assert f"the argument '{name}' takes one input alignment, not two" in usage(tmp_path, args)
    for args, name in ((["--site-counts", "--site-counts"], COUNTS), (["--windows", "2", "--window-site-stats", "--window-site-stats"], STATS),
                       (["--site-counts", "--site-groups", "{g}", "--site-groups={g}"], SGROUPS)):
        assert f"the argument '{name}' cannot be used multiple times" in usage(tmp_path, args)
    for args in (["--site-groups", "{g}"], ["--site-groups={g}", "--summary", "2"], ["--windows", "2", "--site-groups", "{g}"]):
        assert f"the argument '{SGROUPS}' requires '--site-counts' or '--window-site-stats'" in usage(tmp_path, args)
    for args in (["--window-site-stats"], ["--window-site-stats", "--site-groups", "{g}"]):
        assert f"the argument '{STATS}' requires '--windows <W>' or '--regions <FILE>'" in usage(tmp_path, args)
    assert f"the argument '{COUNTS}' cannot be used with '{STATS}'" in usage(tmp_path, ["--site-counts", "--windows", "2", "--window-site-stats"])
    for args, other in ((["--site-counts", "--windows", "2"], "--windows <W>"), (["--site-counts", "--regions", "{r}"], "--regions <FILE>")):
        assert f"the argument '{COUNTS}' cannot be used with '{other}'" in usage(tmp_path, args)
    r = cli(tmp_path, ["{a}", "--site-counts", "--site-groups"])
    assert r.returncode == 2 and f"a value is required for '{SGROUPS}' but none was supplied" in r.stderr.decode()
    r = subprocess.run([CLI, "-h"], capture_output=True)
    lines = r.stdout.decode().splitlines()
    for flag, word in (("--site-counts ", "ambiguous, missing"), ("--window-site-stats ", "theta_w, pi"), ("--site-groups <FILE>", "'all'")):
        line = [x for x in lines if x.lstrip().startswith(flag)]
        assert len(line) == 1 and word in line[0], flag


@pytest.mark.parametrize("own", [["--site-counts"], ["--windows", "2", "--window-site-stats"]])
def test_label_file_errors_and_the_device_stage(tmp_path, own):
    def label_error(labels):
        r = cli(tmp_path, own + ["--site-groups", "{g}"], labels)
        err = r.stderr.decode()
        assert r.returncode == 1 and r.stdout == b"" and err.startswith('Error: Message("--site-groups: ') and "no MI355X" not in err, err
        return err

    err = label_error(b"x\tone\n\ny two\n")
    assert "line 3 of" in err and "has no tab" in err
    assert "empty group" in label_error(b"x\tone\ny\t\n")
    assert "gives 'x' the group 'two', line 1 gave it 'one'" in label_error(b"x\tone\nx\ttwo\n")
    assert "more than two fields" in label_error(b"x\tone\tmore\n")
    assert "no record of the first input has a group" in label_error(b"p\tone\nq\ttwo\n")
    r = cli(tmp_path, own + ["--site-groups", str(tmp_path / "nope.tsv")])
    assert r.returncode == 1 and b"NotFound" in r.stderr and b"nope.tsv" in r.stderr
    # valid values pass every check and end at the device; -m is accepted; ids that are in no input give one warning line
    for extra in ([], ["-m", "tn93"], ["-o", str(tmp_path / "out.tsv")]):
        r = cli(tmp_path, own + extra)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, r.stderr
    r = cli(tmp_path, own + ["--site-groups", "{g}"], b"x\tone\r\ny\ttwo\n\nw\tthree\nv\tthree\n")
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
    assert r.stderr.count(b"warning: --site-groups: 2 ids of") == 1 and b"are not in the input and were skipped" in r.stderr
