"""CPU: the `--within` surface of the `distance` CLI without a GPU: the help line and every usage error, which
parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
FLAG = "--within <T>"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def launch(tmp_path, args):
    for name in ("a", "b", "c"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.format(a=tmp_path / "a.fasta", b=tmp_path / "b.fasta", c=tmp_path / "c.fasta") for x in args]
    return subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def run(tmp_path, args):
    r = launch(tmp_path, args)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


STREAMED = ["-i", "{a}", "-s", "{b}"]


def test_help_line_follows_closest_for():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    at = [n for n, x in enumerate(lines) if x.lstrip().startswith(FLAG)]
    assert len(at) == 1, at
    assert lines[at[0] - 1].lstrip().startswith("--closest-for <side>")
    assert "Stream mode only" in lines[at[0]] and "within distance T" in lines[at[0]]


def test_within_needs_a_stream(tmp_path):
    assert f"'{FLAG}' requires '--stream <stream>'" in run(tmp_path, ["--within", "3", "{a}"])
    assert f"'{FLAG}' requires '--stream <stream>'" in run(tmp_path, ["{a}", "{b}", "--within=3"])


def test_two_loaded_files(tmp_path):
    err = run(tmp_path, ["--within", "3", "-i", "{a}", "{c}", "-s", "{b}"])
    assert f"'{FLAG}' takes one loaded alignment, not two" in err
    err = run(tmp_path, ["-s", "{b}", "{a}", "{c}", "--within=3"])
    assert f"'{FLAG}' takes one loaded alignment, not two" in err


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("gpus, named", [(["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")])
def test_more_than_one_gpu(tmp_path, gpus, named, first):
    err = run(tmp_path, (["--within", "3"] + gpus if first else gpus + ["--within=3"]) + STREAMED)
    assert f"'{FLAG}' cannot be used with '{named}'" in err


MODES = [(["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"), (["--matrix", "tsv"], "--matrix <format>"),
         (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"), (["--mst"], "--mst"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--max-distance", "4"], "--max-distance <T>"),
         (["--histogram", "2"], "--histogram <W>"), (["--summary", "5"], "--summary <T>")]


@pytest.mark.parametrize("with_stream", [True, False])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", MODES)
def test_no_other_output_mode(tmp_path, mode, other, first, with_stream):
    args = (["--within", "3"] + mode if first else mode + ["--within=3"]) + (STREAMED if with_stream else ["{a}"])
    err = run(tmp_path, args)
    assert f"the argument '{FLAG}' cannot be used with '{other}'" in err


@pytest.mark.parametrize("first", [True, False])
def test_closest_and_within_name_each_other(tmp_path, first):
    args = (["--within", "3", "--closest", "2"] if first else ["--closest=2", "--within=3"]) + STREAMED
    err = run(tmp_path, args)
    assert "cannot be used with" in err and "'--closest <k>'" in err and f"'{FLAG}'" in err


def test_sites_keeps_its_own_message(tmp_path):
    assert "the argument '--sites' requires '--max-distance <T>' or '--mst'" in run(tmp_path, ["--sites", "--within", "2", "{a}"])
    assert "the argument '--sites' cannot be used with '--stream <stream>'" in run(tmp_path, ["--within", "2", "--sites"] + STREAMED)


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("5x", "not a number"),
                                        ("", "not a number"), (" 5", "not a number"),
                                        ("-1", "the threshold must not be negative"),
                                        ("-inf", "the threshold must not be negative")])
def test_invalid_values(tmp_path, value, why):
    err = run(tmp_path, [f"--within={value}"] + STREAMED)
    assert f"invalid value '{value}' for '{FLAG}': {why}" in err, err


def test_value_is_required(tmp_path):
    err = run(tmp_path, STREAMED + ["--within"])
    assert f"a value is required for '{FLAG}' but none was supplied" in err


@pytest.mark.parametrize("first", [True, False])
def test_repeated_flag(tmp_path, first):
    args = ["--within", "5", "--within", "6"] + STREAMED if first else STREAMED + ["--within=5", "--within=6"]
    assert f"the argument '{FLAG}' cannot be used multiple times" in run(tmp_path, args)


def test_valid_values_reach_the_gpu_stage(tmp_path):
    """0, a fraction, an exponent and inf parse: without a device the run ends at the device check, exit 1, not 2."""
    for v in ("0", "0.5", "1e3", "inf"):
        for args in (["--within", v] + STREAMED, STREAMED + ["-m", "n", f"--within={v}"]):
            r = launch(tmp_path, args)
            assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (v, r.stderr)


def test_max_distance_still_refuses_a_stream(tmp_path):
    err = run(tmp_path, ["--max-distance", "5"] + STREAMED)
    assert "the argument '--max-distance <T>' cannot be used with '--stream <stream>'" in err
