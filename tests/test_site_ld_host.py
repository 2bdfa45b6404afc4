"""No GPU: dst_site_ld, dst_site_ld_links, dst_ld_finalize and dst_site_major are declared, exported and typed as the header's
prototypes; the constants are the header's; the two host functions give, bit for bit, what site_ld_reference's plain Python
gives on cases written out by hand and on random tallies; and the CLI's usage errors of --ld come before any device is
opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from site_ld_reference import finalize, finalize_one, same_bits, site_major

ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


# ---- the symbols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_args", [("dst_site_ld", 11), ("dst_site_ld_links", 12), ("dst_ld_finalize", 5), ("dst_site_major", 7)])
def test_declared_exported_and_typed(name, n_args):
    assert name in da.declared_symbols() and hasattr(da.load(), name)
    assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert proto and len(proto.group(1).split(",")) == n_args


def test_constants_and_abi():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DST_LD_CHUNK\s+\(1u << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == da.LD_CHUNK == _lib.LD_CHUNK == 1 << 22
    sink = re.search(r"typedef int \(\*dst_ld_sink\)\(([^;]*)\);", text)
    assert sink and len(sink.group(1).split(",")) == 6 and len(_lib.LD_SINK._argtypes_) == 6
    assert re.search(r"#define\s+DST_ABI_VERSION\s+3\b", text) and da.load().dst_abi_version() == 3
    assert "94,906,266" in text   # the bound below which every integer conversion is exact
    for name in ("site_ld", "site_ld_links"):
        assert hasattr(da.Engine, name)
    assert callable(da.ld_finalize) and callable(da.site_major)


def test_null_context_is_err_arg():
    sites, allele, out = np.zeros(2, np.uint32), np.zeros(2, np.uint8), np.zeros(4, np.uint32)
    lib = da.load()
    assert lib.dst_site_ld(None, 0, sites.ctypes.data, allele.ctypes.data, 2, None, 0, 0, 2, out.ctypes.data, 1) == ERR_ARG
    assert lib.dst_site_ld_links(None, 0, sites.ctypes.data, allele.ctypes.data, 2, None, 0, 0.5, 0, None, None, None) == ERR_ARG


# ---- dst_ld_finalize ---------------------------------------------------------------------------------------------------
def check_finalize(t):
    t = np.asarray(t, np.uint32).reshape(-1, 4)
    got, want = da.ld_finalize(t), finalize(t)
    for k in ("r2", "d", "dprime"):
        assert same_bits(got[k], want[k]), (k, got[k], want[k])
    return got


def test_finalize_hand_written():
    got = check_finalize([[0, 0, 0, 0],      # m = 0: everything NaN
                          [5, 0, 2, 0],      # site 1 monomorphic (A = 0): r2, D' NaN, D = 0
                          [5, 2, 5, 2],      # site 2 all minor (B = 0)
                          [4, 2, 2, 2],      # complete LD
                          [4, 2, 2, 0],      # repulsion
                          [8, 4, 4, 3],      # r2 = 0.25 exactly
                          [8, 4, 4, 2]])     # independence
    r2, d, dp = got["r2"], got["d"], got["dprime"]
    assert np.isnan(r2[0]) and np.isnan(d[0]) and np.isnan(dp[0])
    assert np.isnan(r2[1]) and np.isnan(dp[1]) and d[1] == 0.0
    assert np.isnan(r2[2]) and np.isnan(dp[2]) and d[2] == 0.0
    assert r2[3] == 1.0 and dp[3] == 1.0 and d[3] == 0.25
    assert r2[4] == 1.0 and dp[4] == -1.0 and d[4] == -0.25
    assert r2[5] == 0.25 and d[5] == 0.125 and dp[5] == 0.5
    assert r2[6] == 0.0 and d[6] == 0.0 and dp[6] == 0.0
    # NULL outputs are skipped
    t = np.array([[8, 4, 4, 3]], np.uint32)
    one = np.zeros(1)
    assert da.load().dst_ld_finalize(t.ctypes.data, 1, None, None, one.ctypes.data) == 0 and one[0] == 0.5
    assert da.load().dst_ld_finalize(None, 1, one.ctypes.data, None, None) == ERR_ARG
    assert da.load().dst_ld_finalize(None, 0, None, None, None) == 0


def test_finalize_past_2_53():
    """counts near 2^31: m c, a b and m m pass 2^53, so the conversions round"""
    m = 2 ** 31 - 1
    cases = [[m, m // 2, m // 2 + 1, m // 4 + 3], [m, m - 1, m - 2, m - 3], [m, 3, m - 5, 1], [m, m // 3, m // 3, m // 3],
             [m - 7, 1234567891, 987654321, 600000001], [m, 1, 1, 1], [m, m // 2, m // 2, 0]]
    got = check_finalize(cases)
    assert (m * (m // 4 + 3)) > 2 ** 53 and not np.isnan(got["r2"]).any()
    assert float(m * m) != m * m   # (the conversion is not exact here)


def test_finalize_random():
    rng = np.random.default_rng(17)
    rows = []
    for scale in (10, 1000, 10 ** 6, 2 ** 31 - 1):
        for _ in range(2500):
            # a 2 x 2 table of called records: n11 (minor at both), n10, n01, n00
            cells = rng.multinomial(int(rng.integers(0, scale + 1)), rng.dirichlet(np.ones(4) * 0.5))
            n11, n10, n01, n00 = (int(x) for x in cells)
            rows.append([n11 + n10 + n01 + n00, n11 + n10, n11 + n01, n11])
    t = np.array(rows, np.uint32)
    assert len(t) == 10000
    got = check_finalize(t)
    ok = ~np.isnan(got["r2"])
    assert ok.sum() > 5000 and (got["r2"][ok] >= 0).all() and (got["r2"][ok] <= 1.0 + 1e-12).all()
    assert (np.abs(got["dprime"][ok]) <= 1.0 + 1e-12).all()


# ---- dst_site_major ----------------------------------------------------------------------------------------------------
def check_major(counts, g):
    got, want = da.site_major(counts, g), site_major(counts, g)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (got, want)
    return got


def test_site_major_hand_written_and_random():
    counts = np.zeros((7, 2, 5), np.uint32)
    counts[:, 1, :] = [[3, 3, 3, 3, 9],     # a four-way tie: A
                       [0, 0, 0, 0, 4],     # nothing called: A, 0, 0
                       [1, 5, 5, 0, 0],     # T and G tie: T
                       [0, 0, 0, 7, 1],     # only C
                       [2, 0, 9, 9, 0],     # G and C tie: G
                       [2 ** 31, 2 ** 31 - 1, 2 ** 30, 5, 0],
                       [0, 1, 0, 0, 0]]
    allele, major, other = check_major(counts, 1)
    assert allele.tolist() == [0, 0, 1, 3, 2, 0, 1] and major.tolist() == [3, 0, 5, 7, 9, 2 ** 31, 1]
    assert other.tolist() == [9, 0, 6, 0, 11, 2 ** 31 - 1 + 2 ** 30 + 5, 0]
    assert check_major(counts, 0)[1].tolist() == [0] * 7
    rng = np.random.default_rng(3)
    check_major(rng.integers(0, 4, (500, 3, 5)).astype(np.uint32), 2)
    with pytest.raises(da.DistanceError) as e:
        da.site_major(counts, 2)
    assert e.value.status == ERR_ARG
    empty = da.site_major(np.zeros((0, 1, 5), np.uint32))
    assert [len(x) for x in empty] == [0, 0, 0]


# ---- the CLI before any device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def cli(tmp_path, args, labels=b"x\tone\ny\ttwo\n"):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACGG\n")
    (tmp_path / "g.tsv").write_bytes(labels)
    (tmp_path / "r.tsv").write_bytes(b"all\t1\t4\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")).replace("{g}", str(tmp_path / "g.tsv"))
            .replace("{r}", str(tmp_path / "r.tsv")) for x in args]
    if not any(x.endswith("a.fasta") for x in args):
        args.append(str(tmp_path / "a.fasta"))
    return subprocess.run([CLI] + args, capture_output=True, env=NO_GPU)


def usage(tmp_path, args):
    r = cli(tmp_path, args)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: "), (args, r.stderr)
    return r.stderr.decode()


LD, MINC, LGROUPS = "--ld <R2>", "--ld-min-count <C>", "--ld-groups <FILE>"
OTHERS = [(["--stream", "{b}"], "--stream <stream>"), (["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"),
          (["--representatives", "1"], "--representatives <T>"), (["--max-distance", "4"], "--max-distance <T>"),
          (["--summary", "4"], "--summary <T>"), (["--groups", "{g}"], "--groups <FILE>"), (["--histogram", "2"], "--histogram <W>"),
          (["--matrix", "tsv"], "--matrix <format>"), (["--tree", "nj"], "--tree <method>"), (["--mst"], "--mst"),
          (["--sites"], "--sites"), (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--pairs", "{g}"], "--pairs <FILE>"),
          (["--windows", "2"], "--windows <W>"), (["--regions", "{r}"], "--regions <FILE>"),
          (["--window-nearest", "2"], "--window-nearest <K>"), (["--window-summary", "1"], "--window-summary <T>"),
          (["--window-groups", "{g}"], "--window-groups <FILE>"), (["--window-closest", "2"], "--window-closest <K>"),
          (["--stream-summary", "1"], "--stream-summary <T>"), (["--stream-groups", "{g}"], "--stream-groups <FILE>"),
          (["--site-counts"], "--site-counts"), (["--window-site-stats"], "--window-site-stats"),
          (["--site-groups", "{g}"], "--site-groups <FILE>"), (["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", OTHERS)
def test_usage_errors_with_other_modes(tmp_path, mode, other, first):
    own = ["--ld", "0.5"]
    err = usage(tmp_path, own + mode if first else mode + own)
    assert f"the argument '{LD}' cannot be used with '{other}'" in err, err
    if "gpus" in other or "devices" in other:
        assert "naming more than one GPU" in err


def test_usage_errors_of_their_own(tmp_path):
    assert f"the argument '{LD}' takes one input alignment, not two" in usage(tmp_path, ["--ld", "0.5", "{a}", "{b}"])
    for args, name in ((["--ld", "0.5", "--ld=0.2"], LD), (["--ld", "0.5", "--ld-min-count", "2", "--ld-min-count", "3"], MINC),
                       (["--ld", "0.5", "--ld-groups", "{g}", "--ld-groups={g}"], LGROUPS)):
        assert f"the argument '{name}' cannot be used multiple times" in usage(tmp_path, args)
    for args, name in ((["--ld-min-count", "2"], MINC), (["--ld-groups", "{g}"], LGROUPS), (["--ld-groups={g}", "--summary", "2"], LGROUPS),
                       (["--site-counts", "--ld-min-count", "2"], MINC)):
        assert f"the argument '{name}' requires '--ld <R2>'" in usage(tmp_path, args)
    for bad in ("1.5", "-0.1", "2", "inf", "nan", "x", ""):
        assert f"invalid value '{bad}' for '{LD}'" in usage(tmp_path, ["--ld=" + bad])
    for bad in ("0", "-1", "1.5", "x"):
        assert f"invalid value '{bad}' for '{MINC}'" in usage(tmp_path, ["--ld", "0.5", "--ld-min-count=" + bad])
    r = cli(tmp_path, ["{a}", "--ld"])
    assert r.returncode == 2 and f"a value is required for '{LD}' but none was supplied" in r.stderr.decode()
    r = subprocess.run([CLI, "-h"], capture_output=True)
    lines = r.stdout.decode().splitlines()
    for flag, word in (("--ld <R2>", "r2, D, Dprime"), ("--ld-min-count <C>", "[default: 1]"), ("--ld-groups <FILE>", "'all'")):
        line = [x for x in lines if x.lstrip().startswith(flag)]
        assert len(line) == 1 and word in line[0], flag


def test_label_file_errors_and_the_device_stage(tmp_path):
    own = ["--ld", "0.2"]

    def label_error(labels):
        r = cli(tmp_path, own + ["--ld-groups", "{g}"], labels)
        err = r.stderr.decode()
        assert r.returncode == 1 and r.stdout == b"" and err.startswith('Error: Message("--ld-groups: ') and "no MI355X" not in err, err
        return err

    err = label_error(b"x\tone\n\ny two\n")
    assert "line 3 of" in err and "has no tab" in err
    assert "empty group" in label_error(b"x\tone\ny\t\n")
    assert "gives 'x' the group 'two', line 1 gave it 'one'" in label_error(b"x\tone\nx\ttwo\n")
    assert "more than two fields" in label_error(b"x\tone\tmore\n")
    assert "no record of the first input has a group" in label_error(b"p\tone\nq\ttwo\n")
    r = cli(tmp_path, own + ["--ld-groups", str(tmp_path / "nope.tsv")])
    assert r.returncode == 1 and b"NotFound" in r.stderr and b"nope.tsv" in r.stderr
    # accepted command lines pass every check and end at the device; -m is accepted; ids in no input give one warning line
    for extra in ([], ["-m", "tn93"], ["-o", str(tmp_path / "out.tsv")], ["--ld-min-count", "3"], ["--slab-pairs", "5"]):
        r = cli(tmp_path, own + extra)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, r.stderr
    for r2 in ("0", "1", "1e-3", "0.25"):
        r = cli(tmp_path, ["--ld", r2])
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, r.stderr
    r = cli(tmp_path, own + ["--ld-groups", "{g}"], b"x\tone\r\ny\ttwo\n\nw\tthree\nv\tthree\n")
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr
    assert r.stderr.count(b"warning: --ld-groups: 2 ids of") == 1 and b"are not in the input and were skipped" in r.stderr
