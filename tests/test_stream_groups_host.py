"""CPU: the group-summary-stream additions without a GPU.  The C ABI: exported with the documented argument types, ABI
version unchanged, a NULL context or stream refused, the `what` bits and the tile constants the same in the header,
csrc/dst_internal.h and _lib.py; the Python surface; every usage error of `--stream-groups`, which parse_args reports (exit
2, `error: ...`, nothing on stdout), and every error of its FILE, which is read before any GPU is opened."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import distance_amd as da

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1
GROUPS, BY, WITHIN = "--stream-groups <FILE>", "--stream-groups-by <what>", "--stream-groups-within <T>"
VP = C.c_void_p
SIGNATURES = {
    "dst_stream_open_group_summary": [VP, C.c_int, C.c_double, C.c_int, VP, C.c_uint32, C.c_uint32, C.c_size_t, C.c_int, C.c_int,
                                      C.POINTER(VP)],
    "dst_stream_group_labels": [VP, C.POINTER(VP)],
    "dst_stream_group_summary_batch": [VP, C.POINTER(C.c_size_t), C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)],
    "dst_stream_group_summary_result": [VP, VP, C.c_size_t, VP, VP, VP, C.c_size_t, C.POINTER(C.c_uint64)],
}


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def test_symbols_are_declared_exported_and_typed():
    lib = da.load()
    declared = da.declared_symbols()
    header = " ".join(open(da._lib.HEADER_PATH).read().split())
    for name, argtypes in SIGNATURES.items():
        assert name in declared, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert f"int {name}(dst_" in header, name
    # the header's parameter lists, in the documented order
    assert ("int dst_stream_open_group_summary(dst_ctx *ctx, int measure, double threshold, int what, const uint32_t *loaded_group, "
            "uint32_t n_loaded_groups, uint32_t n_streamed_groups, size_t max_records, int depth, int wire, dst_stream **stream);") in header
    assert "int dst_stream_group_labels(dst_stream *stream, uint32_t **labels);" in header
    assert ("int dst_stream_group_summary_batch(dst_stream *stream, size_t *n_records, const uint32_t **within, "
            "const uint32_t **summable, const double **sum);") in header
    assert ("int dst_stream_group_summary_result(dst_stream *stream, dst_group_cell *cells, size_t cells_cap, uint32_t *rec_within, "
            "uint32_t *rec_summable, double *rec_sum, size_t rec_cap, uint64_t *records);") in header


def test_abi_version_is_unchanged():
    assert da.load().dst_abi_version() == 3


def test_null_context_and_stream_are_argument_errors():
    lib = da.load()
    h = C.c_void_p(1)
    assert lib.dst_stream_open_group_summary(None, 2, 5.0, 1, None, 1, 1, 8, 3, 0, C.byref(h)) == ERR_ARG
    assert lib.dst_stream_open_group_summary(None, 2, 5.0, 1, None, 1, 1, 8, 3, 0, None) == ERR_ARG
    n, wp, sp, dp, records = C.c_size_t(7), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(7)
    assert lib.dst_stream_group_labels(None, C.byref(wp)) == ERR_ARG
    assert lib.dst_stream_group_summary_batch(None, C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp)) == ERR_ARG
    assert lib.dst_stream_group_summary_batch(None, None, None, None, None) == ERR_ARG
    assert lib.dst_stream_group_summary_result(None, None, 0, None, None, None, 0, C.byref(records)) == ERR_ARG


def test_what_bits_and_tile_constants_agree():
    header = open(da._lib.HEADER_PATH).read()
    loaded = re.search(r"#define DST_STREAM_GROUPS_LOADED\s+(\d+)\b", header)
    streamed = re.search(r"#define DST_STREAM_GROUPS_STREAMED\s+(\d+)\b", header)
    assert loaded and streamed
    assert (int(loaded.group(1)), int(streamed.group(1))) == (1, 2) == (da._lib.STREAM_GROUPS_LOADED, da._lib.STREAM_GROUPS_STREAMED)
    internal = open(os.path.join(ROOT, "distance_amd", "csrc", "dst_internal.h")).read()
    rows = re.search(r"constexpr uint32_t kStreamGroupRows = (\d+);", internal)
    cols = re.search(r"constexpr uint32_t kStreamGroupCols = (\d+);", internal)
    assert rows and cols
    assert int(rows.group(1)) == da._lib.STREAM_GROUPS_ROWS >= 1
    assert int(cols.group(1)) == da._lib.STREAM_GROUPS_COLS >= 1


def test_python_surface():
    assert hasattr(da.Engine, "group_summary_stream") and issubclass(da.GroupSummaryStream, da.engine.Stream)
    assert "GroupSummaryStream" in da.__all__
    for name in ("pop", "result", "group_summary_batch", "labels", "buffer", "submit", "push", "in_flight", "to_nibbles", "close"):
        assert hasattr(da.GroupSummaryStream, name), name
    p = inspect.signature(da.Engine.group_summary_stream).parameters
    assert list(p)[1:] == ["measure", "max_records", "loaded_groups", "n_loaded_groups", "n_streamed_groups", "threshold", "loaded",
                           "streamed", "depth", "nibbles"]
    assert (p["loaded_groups"].default, p["n_loaded_groups"].default, p["n_streamed_groups"].default, p["threshold"].default,
            p["loaded"].default, p["streamed"].default, p["depth"].default, p["nibbles"].default) == \
        (None, None, 1, float("inf"), False, False, 3, False)
    assert list(inspect.signature(da.GroupSummaryStream.push).parameters)[1:] == ["codes", "counts", "groups"]


# ---- the command line ---------------------------------------------------------------------------------------------------
def launch(tmp_path, args):
    for name in ("a", "b", "c"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    (tmp_path / "g.tsv").write_bytes(b"x\tone\ny\ttwo\n")
    args = [x.format(a=tmp_path / "a.fasta", b=tmp_path / "b.fasta", c=tmp_path / "c.fasta", g=tmp_path / "g.tsv") for x in args]
    return subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"), timeout=60)


def run(tmp_path, args):
    r = launch(tmp_path, args)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


STREAMED = ["-i", "{a}", "-s", "{b}"]
MODE = ["--stream-groups", "{g}"]


def test_help_lists_the_three_flags():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = [x.lstrip() for x in r.stdout.decode().splitlines()]
    for flag in (GROUPS, BY, WITHIN):
        at = [x for x in lines if x.startswith(flag + " ")]
        assert len(at) == 1, flag
    assert "Stream mode only" in [x for x in lines if x.startswith(GROUPS + " ")][0]


def test_needs_a_stream(tmp_path):
    assert f"'{GROUPS}' requires '--stream <stream>'" in run(tmp_path, MODE + ["{a}"])
    assert f"'{GROUPS}' requires '--stream <stream>'" in run(tmp_path, ["{a}", "{b}"] + MODE)


def test_two_loaded_files(tmp_path):
    assert f"'{GROUPS}' takes one loaded alignment, not two" in run(tmp_path, MODE + ["-i", "{a}", "{c}", "-s", "{b}"])


@pytest.mark.parametrize("gpus, named", [(["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")])
def test_more_than_one_gpu(tmp_path, gpus, named):
    assert f"'{GROUPS}' cannot be used with '{named}'" in run(tmp_path, MODE + gpus + STREAMED)
    assert f"'{GROUPS}' cannot be used with '{named}'" in run(tmp_path, gpus + STREAMED + MODE)


OTHERS = [(["--nearest", "2"], "--nearest <k>"), (["--closest", "2"], "--closest <k>"), (["--within", "2"], "--within <T>"),
          (["--clusters", "3"], "--clusters <T>"), (["--representatives", "3"], "--representatives <T>"),
          (["--max-distance", "4"], "--max-distance <T>"), (["--summary", "5"], "--summary <T>"),
          (["--groups", "{g}"], "--groups <FILE>"), (["--histogram", "2"], "--histogram <W>"), (["--bins", "8"], "--bins <B>"),
          (["--matrix", "tsv"], "--matrix <format>"), (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"),
          (["--seed", "5"], "--seed <S>"), (["--mst"], "--mst"), (["--sites"], "--sites"),
          (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--windows", "2"], "--windows <W>"),
          (["--regions", "{a}"], "--regions <FILE>"), (["--pairs", "{a}"], "--pairs <FILE>"),
          (["--closest-for", "loaded"], "--closest-for <side>"), (["--per-record"], "--per-record"),
          (["--groups-within", "1"], "--groups-within <T>"), (["--step", "1"], "--step <S>"),
          (["--window-nearest", "1"], "--window-nearest <K>"), (["--window-closest", "1"], "--window-closest <K>"),
          (["--window-summary", "1"], "--window-summary <T>"), (["--window-summary-by", "record"], "--window-summary-by <what>"),
          (["--window-groups", "{g}"], "--window-groups <FILE>"), (["--window-groups-within", "1"], "--window-groups-within <T>"),
          (["--window-groups-by", "record"], "--window-groups-by <what>"),
          (["--stream-summary", "1"], "--stream-summary <T>"), (["--stream-summary-for", "loaded"], "--stream-summary-for <side>"),
          (["--stream-histogram", "1"], "--stream-histogram <W>"), (["--stream-bins", "4"], "--stream-bins <B>")]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("other, named", OTHERS)
def test_no_other_output_mode_or_modifier(tmp_path, other, named, first):
    err = run(tmp_path, (MODE + other if first else other + MODE) + STREAMED)
    assert f"the argument '{GROUPS}' cannot be used with '{named}'" in err


def test_repeated_flag(tmp_path):
    assert f"the argument '{GROUPS}' cannot be used multiple times" in run(tmp_path, MODE + MODE + STREAMED)
    err = run(tmp_path, MODE + ["--stream-groups-within", "1", "--stream-groups-within", "2"] + STREAMED)
    assert f"the argument '{WITHIN}' cannot be used multiple times" in err


def test_modifiers_without_their_mode(tmp_path):
    assert f"the argument '{BY}' requires '{GROUPS}'" in run(tmp_path, ["--stream-groups-by", "loaded"] + STREAMED)
    assert f"the argument '{WITHIN}' requires '{GROUPS}'" in run(tmp_path, ["--stream-groups-within", "1"] + STREAMED)
    assert f"the argument '{BY}' requires '{GROUPS}'" in run(tmp_path, ["--stream-groups-by", "cell", "{a}", "{b}"])


def test_invalid_values(tmp_path):
    err = run(tmp_path, MODE + ["--stream-groups-by", "both"] + STREAMED)
    assert f"invalid value 'both' for '{BY}'" in err and "[possible values: cell, streamed, loaded]" in err
    for value, why in (("abc", "not a number"), ("nan", "not a number"), ("-1", "the threshold must not be negative")):
        err = run(tmp_path, MODE + [f"--stream-groups-within={value}"] + STREAMED)
        assert f"invalid value '{value}' for '{WITHIN}': {why}" in err, err
    for flag, shown in (("--stream-groups", GROUPS), ("--stream-groups-by", BY), ("--stream-groups-within", WITHIN)):
        assert f"a value is required for '{shown}' but none was supplied" in run(tmp_path, STREAMED + [flag])


@pytest.mark.parametrize("text, line, why", [(b"x\tone\ny two\n", 2, "has no tab: expected 'id<TAB>group'"),
                                             (b"x\tone\n\ny\t\n", 3, "has an empty group"),
                                             (b"x\tone\ty\n", 1, "has more than two fields"),
                                             (b"x\tone\ny\ttwo\nx\tthree\n", 3, "gives 'x' the group 'three', line 1 gave it 'one'")])
@pytest.mark.parametrize("by", ["cell", "streamed", "loaded"])
def test_file_errors_name_the_line_before_any_gpu_is_opened(tmp_path, by, text, line, why):
    bad = tmp_path / "bad.tsv"
    bad.write_bytes(text)
    r = launch(tmp_path, ["--stream-groups", str(bad), "--stream-groups-by", by] + STREAMED)
    err = r.stderr.decode()
    assert r.returncode == 1 and r.stdout == b"", err
    assert f"--stream-groups: line {line} of '{bad}' {why}" in err, err
    assert "HIP device" not in err
    # ... and they are --groups' errors
    g = launch(tmp_path, ["--groups", str(bad), "{a}", "{b}"])
    assert g.returncode == 1 and g.stderr.decode().replace("--groups", "--stream-groups") == err


def test_a_missing_file_and_no_loaded_label(tmp_path):
    r = launch(tmp_path, ["--stream-groups", str(tmp_path / "none.tsv")] + STREAMED)
    assert r.returncode == 1 and b"HIP device" not in r.stderr and r.stdout == b""
    other = tmp_path / "other.tsv"
    other.write_bytes(b"z\tone\n")
    for by in ("cell", "streamed"):
        r = launch(tmp_path, ["--stream-groups", str(other), "--stream-groups-by", by] + STREAMED)
        assert r.returncode == 1 and b"--stream-groups: no record of the loaded input has a group in" in r.stderr, r.stderr
        assert b"HIP device" not in r.stderr
    r = launch(tmp_path, ["--stream-groups", str(other), "--stream-groups-by", "loaded"] + STREAMED)      # needs no loaded labels
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr


def test_valid_lines_reach_the_gpu_stage(tmp_path):
    """Lines that parse end at the device check without a device: exit 1, not 2."""
    for args in (MODE, MODE + ["--stream-groups-by", "cell", "-m", "tn93"], MODE + ["--stream-groups-by=streamed", "-o", "{c}.out"],
                 MODE + ["--stream-groups-by", "loaded", "--stream-groups-within", "inf"],
                 MODE + ["--stream-groups-within=0.5", "--slab-pairs", "100", "-m", "n"]):
        r = launch(tmp_path, args + STREAMED)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)


def test_the_existing_command_lines_parse_as_before(tmp_path):
    assert "the argument '--groups <FILE>' cannot be used with '--stream <stream>'" in run(tmp_path, ["--groups", "{g}"] + STREAMED)
    for args in (["--groups", "{g}", "{a}", "{b}"], ["--groups", "{g}", "--per-record", "--groups-within", "1", "{a}"],
                 ["--stream-summary", "1", "--stream-summary-for", "streamed"] + STREAMED,
                 ["--stream-histogram", "1", "--stream-bins", "8"] + STREAMED,
                 ["--windows", "2", "--window-groups", "{g}", "--window-groups-by", "record", "{a}"],
                 ["--regions", "{a}", "--window-groups", "{g}", "{b}"]):
        r = launch(tmp_path, args)
        if "--regions" in args:      # (the region file is a FASTA here: its own format error, not a usage error)
            assert r.returncode == 1
            continue
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)
