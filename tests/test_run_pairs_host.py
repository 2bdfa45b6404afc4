"""CPU: the host side of dst_run_pairs and of `distance --pairs FILE`: the declaration, the export and the signature, the ABI
version, the NULL-context status, the constants, the lane-group rule; the pair file's errors (exit 1, the line named, no GPU
looked at) and the usage errors (exit 2)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import distance_amd as da
from distance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1
FASTA = b">x\nACGT\n>y\nACGA\n>z\nAAAA\n>z\nACGT\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def test_declared_and_exported():
    assert "dst_run_pairs" in da.declared_symbols() and "dst_run_pairs_lanes" in da.declared_symbols()
    assert hasattr(da.load(), "dst_run_pairs") and hasattr(da.load(), "dst_run_pairs_lanes")
    assert "dst_run_pairs" in _lib._SIGS and len(_lib._SIGS["dst_run_pairs"][1]) == 14
    assert hasattr(da.Engine, "run_pairs")


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_null_context_is_err_arg():
    one = (C.c_uint32 * 1)(0)
    val = (C.c_uint64 * 1)(0)
    assert da.load().dst_run_pairs(None, 2, 1, 0, 1, C.addressof(one), C.addressof(one), 1, 0, 0, C.addressof(val), None, 1,
                                   None) == ERR_ARG


def test_constants_match_header():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DST_RUN_PAIRS_BATCH\s+\(1u\s*<<\s*(\d+)\)", text)
    assert m and (1 << int(m.group(1))) == da.RUN_PAIRS_BATCH == _lib.RUN_PAIRS_BATCH == 2 ** 20
    for name, value in (("AUTO", _lib.PAIRS_AUTO), ("DIRECT", _lib.PAIRS_DIRECT), ("SWEEP", _lib.PAIRS_SWEEP)):
        m = re.search(rf"#define\s+DST_PAIRS_{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert (_lib.PAIRS_AUTO, _lib.PAIRS_DIRECT, _lib.PAIRS_SWEEP) == (0, 1, 2)
    fields = re.search(r"typedef struct \{([^}]*)\} dst_pairs_info;", text).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f[0] for f in _lib.PairsInfo._fields_]


def test_lanes_per_pair_rule():
    """the smallest power of two that covers the 128-site chunks, at most 64"""
    lanes = da.load().dst_run_pairs_lanes
    for length, want in ((0, 1), (1, 1), (128, 1), (129, 2), (256, 2), (257, 4), (1000, 8), (1024, 8), (1025, 16), (2049, 32),
                         (4096, 32), (4097, 64), (8192, 64), (8193, 64), (30000, 64), (2 ** 32 - 1, 64)):
        assert lanes(length) == want, length


def run_cli(tmp_path, pairs, args=(), fasta=FASTA, second=None):
    (tmp_path / "a.fasta").write_bytes(fasta)
    (tmp_path / "pairs.tsv").write_bytes(pairs)
    argv = [CLI, "--pairs", str(tmp_path / "pairs.tsv"), *args, str(tmp_path / "a.fasta")]
    if second is not None:
        (tmp_path / "b.fasta").write_bytes(second)
        argv.append(str(tmp_path / "b.fasta"))
    return subprocess.run(argv, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


FILE_ERRORS = [
    (b"x\ty\nxy\n", "line 2", "has no tab"),
    (b"x\ty\n\nx\ty\tz\n", "line 3", "more than two fields"),
    (b"\ty\n", "line 1", "empty id"),
    (b"x\t\n", "line 1", "empty id"),
    (b"x\ty\r\ny\tw\r\n", "line 2", "'w', which is not in the input"),
    (b"q\ty\n", "line 1", "'q', which is not in the input"),
    (b"\n\nx\tz\n", "line 3", "'z', which 2 records of the input carry"),
]


@pytest.mark.parametrize("pairs, line, what", FILE_ERRORS)
def test_pair_file_errors(tmp_path, pairs, line, what):
    r = run_cli(tmp_path, pairs)
    err = r.stderr.decode()
    assert r.returncode == 1 and r.stdout == b"", err
    assert "--pairs: " + line + " of " in err and what in err, err
    assert "HIP device" not in err


def test_pair_file_errors_with_two_inputs(tmp_path):
    """id1 is looked up in the first input, id2 in the second"""
    second = b">p\nACGT\n>x\nACGA\n"
    r = run_cli(tmp_path, b"x\tp\ny\tx\np\tx\n", second=second)
    assert r.returncode == 1 and "line 3" in r.stderr.decode() and "'p', which is not in the first input" in r.stderr.decode()
    r = run_cli(tmp_path, b"x\tp\nx\ty\n", second=second)
    assert r.returncode == 1 and "line 2" in r.stderr.decode() and "'y', which is not in the second input" in r.stderr.decode()
    r = run_cli(tmp_path, b"z\tp\n", second=second)
    assert r.returncode == 1 and "'z', which 2 records of the first input carry" in r.stderr.decode()


def test_a_good_file_reaches_the_device_check(tmp_path):
    for args, second in (((), None), (("--sites",), None), (("-m", "tn93", "--slab-pairs", "10"), None),
                         (("-o", str(tmp_path / "out.tsv")), b">p\nACGT\n")):
        pairs = b"x\ty\ny\tx\n\nx\tx\n" if second is None else b"x\tp\n"
        r = run_cli(tmp_path, pairs, args, second=second)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)


USAGE = [
    (["-s", "{a}"], "'--pairs <FILE>' cannot be used with '--stream <stream>'"),
    (["--mst"], "'--pairs <FILE>' cannot be used with '--mst'"),
    (["--max-distance", "3"], "'--pairs <FILE>' cannot be used with '--max-distance <T>'"),
    (["--nearest", "2"], "'--pairs <FILE>' cannot be used with '--nearest <k>'"),
    (["--clusters", "2"], "'--pairs <FILE>' cannot be used with '--clusters <T>'"),
    (["--matrix", "tsv"], "'--pairs <FILE>' cannot be used with '--matrix <format>'"),
    (["--tree", "nj"], "'--pairs <FILE>' cannot be used with '--tree <method>'"),
    (["--windows", "2"], "'--pairs <FILE>' cannot be used with '--windows <W>'"),
    (["--summary", "2"], "'--pairs <FILE>' cannot be used with '--summary <T>'"),
    (["--groups", "{p}"], "'--pairs <FILE>' cannot be used with '--groups <FILE>'"),
    (["--gpus", "2"], "'--pairs <FILE>' cannot be used with '--gpus <n>' naming more than one GPU"),
    (["--devices", "0,1"], "'--pairs <FILE>' cannot be used with '--devices <list>' naming more than one GPU"),
    (["--pairs", "{p}"], "'--pairs <FILE>' cannot be used multiple times"),
]


@pytest.mark.parametrize("args, message", USAGE)
def test_usage_errors(tmp_path, args, message):
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{p}", str(tmp_path / "pairs.tsv")) for x in args]
    r = run_cli(tmp_path, b"x\ty\n", args)
    assert r.returncode == 2 and r.stdout == b"", r.stderr
    assert r.stderr.decode().startswith("error: the argument " + message), r.stderr


def test_pairs_needs_a_value_and_help_lists_it(tmp_path):
    (tmp_path / "a.fasta").write_bytes(FASTA)
    r = subprocess.run([CLI, str(tmp_path / "a.fasta"), "--pairs"], capture_output=True)
    assert r.returncode == 2 and b"a value is required for '--pairs <FILE>'" in r.stderr
    r = subprocess.run([CLI, "-h"], capture_output=True)
    line = [x for x in r.stdout.decode().splitlines() if x.lstrip().startswith("--pairs <FILE>")]
    assert r.returncode == 0 and len(line) == 1 and "id1<TAB>id2" in line[0]
