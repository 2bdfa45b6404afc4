"""No GPU: dst_ld_band against brute force on designed lists (row_end, the pair count and the 64 x 64 tiles that hold a band
pair); the new symbols are declared, exported and typed as the header's prototypes and the ABI version stays 3; the decay
reference's own pieces (the bins' pairs against brute force, q's rounding) on cases written out by hand; and the CLI's usage
errors of --ld-max-gap / --ld-decay / --ld-bins come before any device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from site_ld_band_reference import band_pairs, band_rows, band_tiles, decay, decay_pairs, q_of

ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


# ---- the symbols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_args", [("dst_ld_band", 6), ("dst_site_ld_band", 12), ("dst_site_ld_links_band", 13), ("dst_site_ld_decay", 13)])
def test_declared_exported_and_typed(name, n_args):
    assert name in da.declared_symbols() and hasattr(da.load(), name)
    assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert proto and len(proto.group(1).split(",")) == n_args


def test_constants_and_abi():
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("DST_LD_SCALE_BITS", da.LD_SCALE_BITS), ("DST_LD_DECAY_MAX_BINS", da.LD_DECAY_MAX_BINS),
                        ("DST_LD_DECAY_LOCAL_BINS", da.LD_DECAY_LOCAL_BINS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u?\b", text)
        assert m and int(m.group(1)) == value, name
    assert da.LD_SCALE_BITS == 30 and da.LD_DECAY_MAX_BINS == 4096
    assert re.search(r"#define\s+DST_ABI_VERSION\s+3\b", text) and da.load().dst_abi_version() == 3
    assert C.sizeof(_lib.LdBin) == 32 and [f[0] for f in _lib.LdBin._fields_] == ["pairs", "defined", "links", "r2_sum"]
    struct = re.search(r"typedef struct \{([^}]*)\} dst_ld_bin;", text)
    assert struct and re.sub(r"\s+", " ", struct.group(1)).strip() == "uint64_t pairs, defined, links; double r2_sum;"
    for name in ("site_ld_band", "site_ld_decay", "site_ld_links"):
        assert hasattr(da.Engine, name)
    assert callable(da.ld_band)


def test_null_context_is_err_arg():
    sites, allele, out = np.zeros(2, np.uint32), np.zeros(2, np.uint8), np.zeros(4, np.uint32)
    bins = (_lib.LdBin * 2)()
    lib = da.load()
    assert lib.dst_site_ld_band(None, 0, sites.ctypes.data, allele.ctypes.data, 2, None, 0, 5, 0, 2, out.ctypes.data, 1) == ERR_ARG
    assert lib.dst_site_ld_links_band(None, 0, sites.ctypes.data, allele.ctypes.data, 2, None, 0, 0.5, 5, 0, None, None, None) == ERR_ARG
    assert lib.dst_site_ld_decay(None, 0, sites.ctypes.data, allele.ctypes.data, 2, None, 0, 0.5, 1, 2, 0, C.addressof(bins), 2) == ERR_ARG


# ---- dst_ld_band -------------------------------------------------------------------------------------------------------
def regular(S, step=3):
    return np.arange(S, dtype=np.uint32) * step + 5


def desert(S):
    """a cluster of (up to) 70 adjacent sites, a desert of 10,000 sites, then the rest two apart"""
    head = min(S, 70)
    return np.concatenate([np.arange(head), 10_070 + 2 * np.arange(S - head)]).astype(np.uint32)


def check_band(sites, max_gap):
    sites = np.asarray(sites, np.uint32)
    row_end, pairs, tiles = da.ld_band(sites, max_gap)
    want = band_rows(sites, max_gap)
    assert row_end.dtype == np.uint32 and np.array_equal(row_end, want), (len(sites), max_gap)
    assert pairs == len(band_pairs(sites, max_gap)) == int((want.astype(np.int64) - np.arange(len(sites)) - 1).sum())
    assert tiles == band_tiles(sites, max_gap), (len(sites), max_gap, tiles)
    assert (np.diff(row_end.astype(np.int64)) >= 0).all() and (row_end > np.arange(len(sites))).all()
    # NULL outputs are skipped
    p, t = C.c_uint64(77), C.c_uint64(77)
    anchor = sites if len(sites) else np.zeros(1, np.uint32)
    assert da.load().dst_ld_band(anchor.ctypes.data, len(sites), max_gap, None, C.byref(p), None) == 0 and p.value == pairs
    assert da.load().dst_ld_band(anchor.ctypes.data, len(sites), max_gap, None, None, C.byref(t)) == 0 and t.value == tiles
    return row_end, pairs, tiles


@pytest.mark.parametrize("S", [0, 1, 2, 63, 64, 65, 129])
def test_band_on_designed_lists(S):
    rng = np.random.default_rng(S)
    lists = [regular(S), desert(S), np.sort(rng.choice(5000, S, replace=False)).astype(np.uint32)]
    for sites in lists:
        s = sites.astype(np.int64)
        span = int(s[-1] - s[0]) if S else 0
        a_gap = int(s[S // 2] - s[S // 3]) if S >= 3 else 1   # exactly a gap of the list
        for max_gap in {0, 1, a_gap, max(a_gap - 1, 0), span, span + 1, 1 << 40, 2 ** 64 - 1}:
            row_end, pairs, tiles = check_band(sites, max_gap)
            if max_gap == 0:
                assert pairs == 0 and tiles == 0
            if max_gap >= span:
                # the whole triangle: every tile on or above the diagonal, but a last diagonal tile of one position (no pair)
                t = (S + 63) // 64
                assert pairs == S * (S - 1) // 2 and tiles == t * (t + 1) // 2 - (S % 64 == 1)


def test_a_row_with_an_empty_band():
    sites = desert(129)
    row_end, pairs, tiles = check_band(sites, 100)
    assert row_end[69] == 70 and row_end[68] == 70 and row_end[0] == 70 and row_end[70] > 71   # the cluster's last row has no pair
    # the cluster fills tile (0, 0) and reaches tile (0, 1); the rest starts in tile row 1
    assert tiles == band_tiles(sites, 100) and tiles >= 4
    lonely = np.array([0, 1000, 2000, 3000], np.uint32)
    assert check_band(lonely, 999)[1:] == (0, 0) and check_band(lonely, 1000)[1:] == (3, 1)


def test_a_band_on_a_tile_edge_and_one_past_it():
    """130 adjacent sites: at max_gap 64 row 63's band ends at position 127, the last of tile column 1; at 65 it reaches
    position 128, the first of tile column 2: one more tile"""
    sites = np.arange(130, dtype=np.uint32)
    on_edge, past = check_band(sites, 64), check_band(sites, 65)
    assert on_edge[0][63] == 128 and past[0][63] == 129
    assert on_edge[2] == 5 and past[2] == 6
    # a diagonal tile alone: gaps inside one tile only
    assert check_band(np.arange(64, dtype=np.uint32), 70)[2] == 1
    # tile row 0 ends exactly at its own edge: rows 0..62 pair inside the tile, row 63's only pair is in tile (0, 1)
    # (tile (1, 1) holds position 64 alone: no pair); with a 66th site it has one
    assert check_band(np.arange(65, dtype=np.uint32), 1)[2] == 2 and check_band(np.arange(66, dtype=np.uint32), 1)[2] == 3


def test_a_tile_row_whose_last_row_alone_has_a_pair():
    """64 sites a thousand apart and a 65th next to the last: at max_gap 1 the only pair is (63, 64), in tile (0, 1); the
    diagonal tile (0, 0) holds none and is not counted.  The same behind a first full tile row, and with a pair inside the
    diagonal tile as well."""
    lonely = np.concatenate([np.arange(64) * 1000, [63001]]).astype(np.uint32)
    assert check_band(lonely, 1)[1:] == (1, 1)
    assert check_band(lonely, 999)[1:] == (1, 1) and check_band(lonely, 1000)[2] == 2
    behind = np.concatenate([np.arange(64), 5000 + np.arange(64) * 1000, [5000 + 63001, 5000 + 63002]]).astype(np.uint32)
    assert check_band(behind, 1)[1:] == (63 + 2, 1 + 1 + 1)   # tiles (0, 0), (1, 2), (2, 2)
    both = lonely.copy()
    both[1] = 1
    assert check_band(both, 1)[1:] == (2, 2)
    for max_gap in (1, 2, 1000, 1001, 70000):
        check_band(behind, max_gap)


def test_a_list_that_does_not_ascend_is_refused():
    for bad in ([3, 3], [1, 2, 2, 4], [5, 4], [0, 10, 9, 20]):
        with pytest.raises(da.DistanceError) as e:
            da.ld_band(bad, 5)
        assert e.value.status == ERR_ARG
    assert da.load().dst_ld_band(None, 3, 5, None, None, None) == ERR_ARG
    assert da.load().dst_ld_band(None, 0, 5, None, None, None) == 0


# ---- the decay reference -------------------------------------------------------------------------------------------------
def test_decay_pairs_against_brute_force():
    for S in (0, 1, 2, 65, 129):
        for sites in (regular(S), desert(S)):
            s = sites.astype(np.int64)
            for width, bins in ((1, 4096), (1, 1), (7, 13), (int(s[-1] - s[0]) + 1 if S else 1, 1)):
                brute = np.zeros(bins, np.uint64)
                for p in range(S):
                    for q in range(p + 1, S):
                        if (s[q] - s[p]) // width < bins:
                            brute[(s[q] - s[p]) // width] += 1
                assert np.array_equal(decay_pairs(sites, width, bins), brute)
                got = decay(sites, np.zeros((S * (S - 1) // 2, 4), np.uint32), width, bins, 0.0)
                assert np.array_equal(got["pairs"], brute) and not got["defined"].any() and got["q"] == [0] * bins
                assert int(brute.sum()) == da.ld_band(sites, width * bins - 1)[1]


def test_q_rounds_to_nearest_even():
    one = 1 << 30
    assert q_of(0.0) == 0 and q_of(1.0) == one and q_of(0.25) == one >> 2
    # products that end in .5: ties go to the even neighbour
    assert q_of(0.5 * 2.0 ** -30) == 0 and q_of(1.5 * 2.0 ** -30) == 2 and q_of(2.5 * 2.0 ** -30) == 2 and q_of(3.5 * 2.0 ** -30) == 4
    assert q_of(float(np.nextafter(0.5 * 2.0 ** -30, 1.0))) == 1 and q_of(float(np.nextafter(1.0, 2.0))) == one
    # {8, 4, 4, 3}: r2 = 0.25 exactly; {4, 2, 2, 2}: 1; {8, 4, 4, 2}: 0; {5, 0, 2, 0}: not defined
    t = np.array([[8, 4, 4, 3], [4, 2, 2, 2], [8, 4, 4, 2], [5, 0, 2, 0], [9, 3, 4, 2], [7, 3, 3, 1]], np.uint32)
    sites = np.array([0, 1, 2, 3], np.uint32)   # 6 pairs: gaps 1, 2, 3, 1, 2, 1
    got = decay(sites, t, 1, 4, 0.25)
    assert got["pairs"].tolist() == [0, 3, 2, 1] and got["defined"].tolist() == [0, 2, 2, 1]
    assert got["links"].tolist() == [0, 1, 1, 0]
    r2 = da.ld_finalize(t)["r2"]
    assert got["q"] == [0, q_of(r2[0]) + q_of(r2[5]), q_of(r2[1]) + q_of(r2[4]), 0]
    assert got["r2_sum"][1] == (q_of(r2[0]) + q_of(r2[5])) / one


# ---- the CLI before any device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def cli(tmp_path, args):
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACGG\n")
    (tmp_path / "g.tsv").write_bytes(b"x\tone\ny\ttwo\n")
    args = [x.replace("{g}", str(tmp_path / "g.tsv")) for x in args]
    return subprocess.run([CLI] + args + [str(tmp_path / "a.fasta")], capture_output=True, env=NO_GPU)


def usage(tmp_path, args):
    r = cli(tmp_path, args)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: "), (args, r.stderr)
    return r.stderr.decode()


LD, GAP, DECAY, BINS = "--ld <R2>", "--ld-max-gap <G>", "--ld-decay <W>", "--ld-bins <B>"


def test_usage_errors(tmp_path):
    own = ["--ld", "0.5"]
    for args, name in ((["--ld-max-gap", "5"], GAP), (["--ld-decay", "5"], DECAY), (["--summary", "2", "--ld-max-gap=5"], GAP),
                       (["--site-counts", "--ld-decay", "5"], DECAY)):
        assert f"the argument '{name}' requires '{LD}'" in usage(tmp_path, args)
    assert f"the argument '{BINS}' requires '{DECAY}'" in usage(tmp_path, own + ["--ld-bins", "9"])
    assert f"the argument '{BINS}' requires '{DECAY}'" in usage(tmp_path, own + ["--ld-max-gap", "4", "--ld-bins", "9"])
    for args in (own + ["--ld-max-gap", "4", "--ld-decay", "2"], own + ["--ld-decay=2", "--ld-bins", "3", "--ld-max-gap=4"]):
        assert f"the argument '{GAP}' cannot be used with '{DECAY}'" in usage(tmp_path, args)
    for args, name in ((own + ["--ld-max-gap", "4", "--ld-max-gap=4"], GAP), (own + ["--ld-decay", "4", "--ld-decay", "5"], DECAY),
                       (own + ["--ld-decay", "4", "--ld-bins", "5", "--ld-bins=5"], BINS)):
        assert f"the argument '{name}' cannot be used multiple times" in usage(tmp_path, args)
    for bad in ("0", "-1", "1.5", "x", ""):
        assert f"invalid value '{bad}' for '{DECAY}'" in usage(tmp_path, own + ["--ld-decay=" + bad])
    for bad in ("0", "4097", "-1", "x"):
        assert f"invalid value '{bad}' for '{BINS}'" in usage(tmp_path, own + ["--ld-decay", "3", "--ld-bins=" + bad])
    for bad in ("-1", "1.5", "x", ""):
        assert f"invalid value '{bad}' for '{GAP}'" in usage(tmp_path, own + ["--ld-max-gap=" + bad])
    # everything --ld refuses stays refused with the new flags
    assert f"the argument '{LD}' cannot be used with '--summary <T>'" in usage(tmp_path, own + ["--ld-max-gap", "3", "--summary", "2"])
    assert f"the argument '{LD}' cannot be used with '--windows <W>'" in usage(tmp_path, own + ["--ld-decay", "3", "--windows", "2"])
    r = subprocess.run([CLI, "--ld", "0.5", "--ld-max-gap"], capture_output=True, env=NO_GPU)
    assert r.returncode == 2 and f"a value is required for '{GAP}' but none was supplied" in r.stderr.decode()


def test_help_and_the_device_stage(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True)
    lines = r.stdout.decode().splitlines()
    for flag, word in ((GAP, "site2 - site1 <= G"), (DECAY, "group, gap"), (BINS, "[default: 256]")):
        line = [x for x in lines if x.lstrip().startswith(flag)]
        assert len(line) == 1 and word in line[0], flag
    # accepted command lines pass every check and end at the device
    for extra in (["--ld-max-gap", "0"], ["--ld-max-gap", "7", "--ld-min-count", "2"], ["--ld-decay", "3"], ["--ld-decay", "3", "--ld-bins", "4096"],
                  ["--ld-decay", "1", "--ld-bins", "1", "--ld-groups", "{g}", "--slab-pairs", "5"], ["--ld-max-gap", "2", "-o", str(tmp_path / "o.tsv")]):
        r = cli(tmp_path, ["--ld", "0.2"] + extra)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (extra, r.stderr)
