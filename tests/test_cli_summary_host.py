"""CPU: the `--summary`, `--histogram` and `--bins` surface of the `distance` CLI without a GPU: the help lines and every
usage error, which parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
SUMMARY, HISTOGRAM, BINS = "--summary <T>", "--histogram <W>", "--bins <B>"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    if not any(x.endswith("a.fasta") for x in args):
        args.append(str(tmp_path / "a.fasta"))
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


def test_help_lists_the_modes():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    line = [x for x in lines if "--summary <T>" in x]
    assert len(line) == 1 and "within distance T" in line[0] and "mean distance" in line[0]
    line = [x for x in lines if "--histogram <W>" in x]
    assert len(line) == 1 and "histogram of the pairwise distances" in line[0]
    line = [x for x in lines if "--bins <B>" in x]
    assert len(line) == 1 and "[default: 256]" in line[0]


MODES = [(["-s", "{b}"], "--stream <stream>"), (["--stream", "{b}"], "--stream <stream>"),
         (["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"),
         (["--matrix", "tsv"], "--matrix <format>"), (["--matrix", "phylip"], "--matrix <format>"),
         (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"),
         (["--tree", "nj", "--bootstrap", "5"], "--tree <method>"), (["--mst"], "--mst"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--max-distance", "4"], "--max-distance <T>"),
         (["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")]
OWN = [(["--summary", "5"], ["--summary=5"], SUMMARY), (["--histogram", "2"], ["--histogram=2"], HISTOGRAM),
       (["--histogram", "2", "--bins", "16"], ["--bins=16", "--histogram=2"], HISTOGRAM)]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", MODES)
@pytest.mark.parametrize("own", OWN, ids=["summary", "histogram", "histogram-bins"])
def test_usage_errors(tmp_path, own, mode, other, first):
    args = own[0] + mode if first else mode + own[1]
    err = run(tmp_path, args)
    assert f"the argument '{own[2]}' cannot be used with '{other}'" in err, err


@pytest.mark.parametrize("args", [["--summary", "5", "--histogram", "2"], ["--histogram=2", "--summary=5"],
                                  ["--bins", "8", "--summary", "5", "--histogram", "2"]])
def test_with_each_other(tmp_path, args):
    err = run(tmp_path, args)
    assert f"the argument '{SUMMARY}' cannot be used with '{HISTOGRAM}'" in err, err


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("5x", "not a number"),
                                        ("", "not a number"), ("-1", "the threshold must not be negative"),
                                        ("-inf", "the threshold must not be negative")])
def test_invalid_thresholds(tmp_path, value, why):
    err = run(tmp_path, [f"--summary={value}"])
    assert f"invalid value '{value}' for '{SUMMARY}': {why}" in err, err


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("2x", "not a number"), ("", "not a number"),
                                        ("0", "the bin width must be above 0 and below 2^25"),
                                        ("-0.5", "the bin width must be above 0 and below 2^25"),
                                        ("inf", "the bin width must be above 0 and below 2^25"),
                                        ("33554432", "the bin width must be above 0 and below 2^25"),
                                        ("1e-12", "the bin width must be above 0 and below 2^25")])
def test_invalid_widths(tmp_path, value, why):
    err = run(tmp_path, [f"--histogram={value}"])
    assert f"invalid value '{value}' for '{HISTOGRAM}': {why}" in err, err


@pytest.mark.parametrize("measure", ["n", "n_high"])
def test_integer_measures_take_an_integer_width(tmp_path, measure):
    for args in (["-m", measure, "--histogram", "0.5"], ["--histogram=2.5", "-m", measure]):
        err = run(tmp_path, args)
        assert f"invalid value for '{HISTOGRAM}': the bin width must be an integer with '--measure {measure}'" in err, err


@pytest.mark.parametrize("value, why", [("0", "0 is not in 1..=4096"), ("4097", "4097 is not in 1..=4096"),
                                        ("x", "invalid digit found in string"), ("-3", "invalid digit found in string"),
                                        ("1.5", "invalid digit found in string")])
def test_invalid_bins(tmp_path, value, why):
    err = run(tmp_path, ["--histogram", "1", f"--bins={value}"])
    assert f"invalid value '{value}' for '{BINS}': {why}" in err, err


@pytest.mark.parametrize("args", [["--bins", "16"], ["--bins=16", "--summary", "3"], ["--bins", "16", "--clusters", "3"]])
def test_bins_requires_histogram(tmp_path, args):
    err = run(tmp_path, args)
    assert f"the argument '{BINS}' requires '{HISTOGRAM}'" in err, err


@pytest.mark.parametrize("flag, name", [("--summary", SUMMARY), ("--histogram", HISTOGRAM), ("--bins", BINS)])
def test_value_is_required(tmp_path, flag, name):
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n")
    r = subprocess.run([CLI, str(tmp_path / "a.fasta"), flag], capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and r.stdout == b""
    assert f"a value is required for '{name}' but none was supplied" in r.stderr.decode()


@pytest.mark.parametrize("flag, name", [("--summary", SUMMARY), ("--histogram", HISTOGRAM)])
def test_repeated_flag(tmp_path, flag, name):
    err = run(tmp_path, [flag, "5", flag, "6"])
    assert f"the argument '{name}' cannot be used multiple times" in err


def test_valid_values_reach_the_gpu_stage(tmp_path):
    """Valid values parse: without a device the run ends at the device check, exit 1, not 2."""
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    for args in (["--summary", "0"], ["--summary", "0.5"], ["--summary", "inf"], ["--histogram", "0.001"], ["--histogram", "1e-3", "--bins", "4096"],
                 ["-m", "n", "--histogram", "2", "--bins=1"], ["-m", "n_high", "--histogram", "1e1"],
                 ["--summary", "3", "--slab-pairs", "5", "{a}", "{a}"]):
        args = [x.replace("{a}", str(tmp_path / "a.fasta")) for x in args]
        if not any(x.endswith("a.fasta") for x in args):
            args.append(str(tmp_path / "a.fasta"))
        r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)
