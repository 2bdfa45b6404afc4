"""CPU: the summary-stream additions without a GPU.  The C ABI: exported, declared, ABI version unchanged, a NULL context
or stream refused, the `what` bits and the tile constants the same in the header, csrc/dst_internal.h and _lib.py; the
Python surface; and every usage error of `--stream-summary` / `--stream-histogram`, which parse_args reports (exit 2,
`error: ...`, nothing on stdout) before any GPU work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import distance_amd as da

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
NEW = ("dst_stream_open_summary", "dst_stream_summary_batch", "dst_stream_summary_result")
ERR_ARG = 1
SUMMARY, FOR, HIST, BINS = "--stream-summary <T>", "--stream-summary-for <side>", "--stream-histogram <W>", "--stream-bins <B>"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def test_symbols_are_declared_and_exported():
    lib = da.load()
    declared = da.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_abi_version_is_unchanged():
    assert da.load().dst_abi_version() == 3


def test_null_context_and_stream_are_argument_errors():
    lib = da.load()
    h = C.c_void_p(1)
    assert lib.dst_stream_open_summary(None, 2, 5.0, 1, 0, 1.0, 8, 3, 0, C.byref(h)) == ERR_ARG
    assert lib.dst_stream_open_summary(None, 2, 5.0, 1, 0, 1.0, 8, 3, 0, None) == ERR_ARG
    n, wp, sp, dp = C.c_size_t(7), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.dst_stream_summary_batch(None, C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp)) == ERR_ARG
    assert lib.dst_stream_summary_batch(None, None, None, None, None) == ERR_ARG
    tot, records = da._lib.SummaryTotals(), C.c_uint64(7)
    assert lib.dst_stream_summary_result(None, None, None, None, None, 0, C.byref(tot), C.byref(records)) == ERR_ARG
    assert lib.dst_stream_summary_result(None, None, None, None, None, 0, None, None) == ERR_ARG


def test_what_bits_and_tile_constants_agree():
    header = open(da._lib.HEADER_PATH).read()
    loaded = re.search(r"#define DST_STREAM_SUMMARY_LOADED\s+(\d+)\b", header)
    streamed = re.search(r"#define DST_STREAM_SUMMARY_STREAMED\s+(\d+)\b", header)
    assert loaded and streamed
    assert (int(loaded.group(1)), int(streamed.group(1))) == (1, 2) == (da._lib.STREAM_SUMMARY_LOADED, da._lib.STREAM_SUMMARY_STREAMED)
    internal = open(os.path.join(ROOT, "distance_amd", "csrc", "dst_internal.h")).read()
    rows = re.search(r"constexpr uint32_t kStreamSummaryRows = (\d+);", internal)
    cols = re.search(r"constexpr uint32_t kStreamSummaryCols = (\d+);", internal)
    assert rows and cols
    assert int(rows.group(1)) == da._lib.STREAM_SUMMARY_ROWS >= 1
    assert int(cols.group(1)) == da._lib.STREAM_SUMMARY_COLS >= 1


def test_python_surface():
    assert hasattr(da.Engine, "summary_stream") and issubclass(da.SummaryStream, da.engine.Stream)
    assert "SummaryStream" in da.__all__
    for name in ("pop", "result", "summary_batch", "buffer", "submit", "push", "in_flight", "to_nibbles", "close"):
        assert hasattr(da.SummaryStream, name), name
    p = inspect.signature(da.Engine.summary_stream).parameters
    assert list(p)[1:] == ["measure", "max_records", "threshold", "loaded", "streamed", "bins", "width", "depth", "nibbles"]
    assert (p["threshold"].default, p["loaded"].default, p["streamed"].default, p["bins"].default, p["width"].default,
            p["depth"].default, p["nibbles"].default) == (0.0, True, False, 0, 1.0, 3, False)


# ---- the command line ---------------------------------------------------------------------------------------------------
def launch(tmp_path, args):
    for name in ("a", "b", "c"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.format(a=tmp_path / "a.fasta", b=tmp_path / "b.fasta", c=tmp_path / "c.fasta") for x in args]
    return subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=60)


def run(tmp_path, args):
    r = launch(tmp_path, args)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


STREAMED = ["-i", "{a}", "-s", "{b}"]
BOTH = [(["--stream-summary", "3"], SUMMARY), (["--stream-histogram", "2"], HIST)]


def test_help_lists_the_four_flags():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = [x.lstrip() for x in r.stdout.decode().splitlines()]
    for flag in (SUMMARY, FOR, HIST, BINS):
        at = [x for x in lines if x.startswith(flag + " ")]
        assert len(at) == 1, flag
    assert "Stream mode only" in [x for x in lines if x.startswith(SUMMARY + " ")][0]


@pytest.mark.parametrize("mode, shown", BOTH)
def test_needs_a_stream(tmp_path, mode, shown):
    assert f"'{shown}' requires '--stream <stream>'" in run(tmp_path, mode + ["{a}"])
    assert f"'{shown}' requires '--stream <stream>'" in run(tmp_path, ["{a}", "{b}"] + mode)


@pytest.mark.parametrize("mode, shown", BOTH)
def test_two_loaded_files(tmp_path, mode, shown):
    err = run(tmp_path, mode + ["-i", "{a}", "{c}", "-s", "{b}"])
    assert f"'{shown}' takes one loaded alignment, not two" in err


@pytest.mark.parametrize("mode, shown", BOTH)
@pytest.mark.parametrize("gpus, named", [(["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")])
def test_more_than_one_gpu(tmp_path, gpus, named, mode, shown):
    assert f"'{shown}' cannot be used with '{named}'" in run(tmp_path, mode + gpus + STREAMED)
    assert f"'{shown}' cannot be used with '{named}'" in run(tmp_path, gpus + STREAMED + mode)


def test_each_other(tmp_path):
    err = run(tmp_path, ["--stream-summary", "3", "--stream-histogram", "2"] + STREAMED)
    assert f"the argument '{SUMMARY}' cannot be used with '{HIST}'" in err
    err = run(tmp_path, ["--stream-summary", "3", "--stream-bins", "4"] + STREAMED)
    assert f"the argument '{BINS}' requires '{HIST}'" in err
    err = run(tmp_path, ["--stream-histogram", "3", "--stream-summary-for", "loaded"] + STREAMED)
    assert f"the argument '{FOR}' requires '{SUMMARY}'" in err


OTHERS = [(["--nearest", "2"], "--nearest <k>"), (["--closest", "2"], "--closest <k>"), (["--within", "2"], "--within <T>"),
          (["--clusters", "3"], "--clusters <T>"), (["--representatives", "3"], "--representatives <T>"),
          (["--max-distance", "4"], "--max-distance <T>"), (["--summary", "5"], "--summary <T>"),
          (["--groups", "{a}"], "--groups <FILE>"), (["--histogram", "2"], "--histogram <W>"), (["--bins", "8"], "--bins <B>"),
          (["--matrix", "tsv"], "--matrix <format>"), (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"),
          (["--seed", "5"], "--seed <S>"), (["--mst"], "--mst"), (["--sites"], "--sites"),
          (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--windows", "2"], "--windows <W>"),
          (["--regions", "{a}"], "--regions <FILE>"), (["--pairs", "{a}"], "--pairs <FILE>"),
          (["--closest-for", "loaded"], "--closest-for <side>"), (["--per-record"], "--per-record"),
          (["--groups-within", "1"], "--groups-within <T>"), (["--step", "1"], "--step <S>"),
          (["--window-nearest", "1"], "--window-nearest <K>"), (["--window-closest", "1"], "--window-closest <K>"),
          (["--window-summary", "1"], "--window-summary <T>"), (["--window-summary-by", "record"], "--window-summary-by <what>"),
          (["--window-groups", "{a}"], "--window-groups <FILE>"), (["--window-groups-within", "1"], "--window-groups-within <T>"),
          (["--window-groups-by", "record"], "--window-groups-by <what>")]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("other, named", OTHERS)
@pytest.mark.parametrize("mode, shown", BOTH)
def test_no_other_output_mode_or_modifier(tmp_path, mode, shown, other, named, first):
    err = run(tmp_path, (mode + other if first else other + mode) + STREAMED)
    assert f"the argument '{shown}' cannot be used with '{named}'" in err


@pytest.mark.parametrize("mode, shown", BOTH)
def test_repeated_flag(tmp_path, mode, shown):
    assert f"the argument '{shown}' cannot be used multiple times" in run(tmp_path, mode + mode + STREAMED)


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("5x", "not a number"),
                                        ("", "not a number"), (" 5", "not a number"),
                                        ("-1", "the threshold must not be negative"),
                                        ("-inf", "the threshold must not be negative")])
def test_invalid_thresholds(tmp_path, value, why):
    err = run(tmp_path, [f"--stream-summary={value}"] + STREAMED)
    assert f"invalid value '{value}' for '{SUMMARY}': {why}" in err, err


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"),
                                        ("0", "the bin width must be above 0 and below 2^25"),
                                        ("-1", "the bin width must be above 0 and below 2^25"),
                                        ("inf", "the bin width must be above 0 and below 2^25"),
                                        ("33554432", "the bin width must be above 0 and below 2^25"),
                                        ("1e-12", "the bin width must be above 0 and below 2^25")])
def test_invalid_widths(tmp_path, value, why):
    err = run(tmp_path, [f"--stream-histogram={value}"] + STREAMED)
    assert f"invalid value '{value}' for '{HIST}': {why}" in err, err


@pytest.mark.parametrize("measure", ["n", "n_high"])
def test_integer_measures_want_an_integer_width(tmp_path, measure):
    err = run(tmp_path, ["--stream-histogram", "0.5", "-m", measure] + STREAMED)
    assert f"invalid value for '{HIST}': the bin width must be an integer with '--measure {measure}'" in err


@pytest.mark.parametrize("value", ["0", "4097", "x", "-1"])
def test_invalid_bins(tmp_path, value):
    err = run(tmp_path, ["--stream-histogram", "1", f"--stream-bins={value}"] + STREAMED)
    assert f"invalid value '{value}' for '{BINS}'" in err, err


def test_invalid_side(tmp_path):
    err = run(tmp_path, ["--stream-summary", "1", "--stream-summary-for", "both"] + STREAMED)
    assert f"invalid value 'both' for '{FOR}'" in err and "[possible values: loaded, streamed]" in err


@pytest.mark.parametrize("flag, shown", [("--stream-summary", SUMMARY), ("--stream-summary-for", FOR),
                                         ("--stream-histogram", HIST), ("--stream-bins", BINS)])
def test_value_is_required(tmp_path, flag, shown):
    assert f"a value is required for '{shown}' but none was supplied" in run(tmp_path, STREAMED + [flag])


def test_modifiers_without_their_mode(tmp_path):
    assert f"the argument '{FOR}' requires '{SUMMARY}'" in run(tmp_path, ["--stream-summary-for", "streamed"] + STREAMED)
    assert f"the argument '{BINS}' requires '{HIST}'" in run(tmp_path, ["--stream-bins", "16"] + STREAMED)


def test_valid_lines_reach_the_gpu_stage(tmp_path):
    """Lines that parse end at the device check without a device: exit 1, not 2."""
    for args in (["--stream-summary", "0"], ["--stream-summary=inf", "--stream-summary-for", "streamed", "-m", "tn93"],
                 ["--stream-summary", "1e3", "--stream-summary-for=loaded", "-o", "{c}.out"],
                 ["--stream-histogram", "0.5"], ["--stream-histogram=2", "--stream-bins", "4096", "-m", "n"],
                 ["--stream-histogram", "1", "--slab-pairs", "100"]):
        r = launch(tmp_path, args + STREAMED)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)


def test_summary_and_histogram_still_refuse_a_stream(tmp_path):
    assert "the argument '--summary <T>' cannot be used with '--stream <stream>'" in run(tmp_path, ["--summary", "5"] + STREAMED)
    assert "the argument '--histogram <W>' cannot be used with '--stream <stream>'" in run(tmp_path, ["--histogram", "5"] + STREAMED)
