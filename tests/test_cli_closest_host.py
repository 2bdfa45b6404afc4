"""CPU: the `--closest` / `--closest-for` surface of the `distance` CLI without a GPU: the help lines and every usage
error, which parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
CLOSEST, SIDE = "--closest <k>", "--closest-for <side>"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(tmp_path, args):
    for name in ("a", "b", "c"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.format(a=tmp_path / "a.fasta", b=tmp_path / "b.fasta", c=tmp_path / "c.fasta") for x in args]
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


STREAMED = ["-i", "{a}", "-s", "{b}"]


def test_help_names_both_flags():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    at = {flag: [n for n, x in enumerate(lines) if x.lstrip().startswith(flag)] for flag in ("--nearest <k>", CLOSEST, SIDE)}
    assert all(len(v) == 1 for v in at.values()), at
    assert at["--nearest <k>"][0] < at[CLOSEST][0] < at[SIDE][0]          # after --nearest
    assert "1-256" in lines[at[CLOSEST][0]] and "[default: loaded]" in lines[at[SIDE][0]]


def test_closest_needs_a_stream(tmp_path):
    assert "'--closest <k>' requires '--stream <stream>'" in run(tmp_path, ["--closest", "3", "{a}"])
    assert "'--closest <k>' requires '--stream <stream>'" in run(tmp_path, ["--closest=3", "{a}", "{b}"])


@pytest.mark.parametrize("k", ["0", "257", "1000", "-1", "x", ""])
def test_k_outside_1_to_256(tmp_path, k):
    err = run(tmp_path, ["--closest=" + k] + STREAMED)
    assert "--closest <k>" in err


def test_closest_for(tmp_path):
    assert "'--closest-for <side>' requires '--closest <k>'" in run(tmp_path, ["--closest-for", "loaded"] + STREAMED)
    assert "'--closest-for <side>' requires '--closest <k>'" in run(tmp_path, ["--closest-for=streamed", "{a}"])
    err = run(tmp_path, ["--closest", "3", "--closest-for", "both"] + STREAMED)
    assert "invalid value 'both' for '--closest-for <side>'" in err and "loaded, streamed" in err
    assert "a value is required for '--closest-for <side>'" in run(tmp_path, STREAMED + ["--closest", "3", "--closest-for"])


@pytest.mark.parametrize("gpus, named", [(["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")])
def test_more_than_one_gpu(tmp_path, gpus, named):
    err = run(tmp_path, ["--closest", "3"] + gpus + STREAMED)
    assert f"'--closest <k>' cannot be used with '{named}'" in err


def test_two_loaded_files(tmp_path):
    err = run(tmp_path, ["--closest", "3", "-i", "{a}", "{c}", "-s", "{b}"])
    assert "'--closest <k>' takes one loaded alignment, not two" in err
    err = run(tmp_path, ["--closest", "3", "-s", "{b}", "{a}", "{c}"])
    assert "'--closest <k>' takes one loaded alignment, not two" in err


MODES = [(["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"), (["--matrix", "tsv"], "--matrix <format>"),
         (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"), (["--mst"], "--mst"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--max-distance", "4"], "--max-distance <T>"),
         (["--histogram", "2"], "--histogram <W>"), (["--summary", "5"], "--summary <T>")]


@pytest.mark.parametrize("with_stream", [True, False])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", MODES)
def test_no_other_output_mode(tmp_path, mode, other, first, with_stream):
    args = (["--closest", "3"] + mode if first else mode + ["--closest=3"]) + (STREAMED if with_stream else ["{a}"])
    err = run(tmp_path, args)
    assert f"the argument '--closest <k>' cannot be used with '{other}'" in err


def test_nearest_still_refuses_a_stream(tmp_path):
    err = run(tmp_path, ["--nearest", "3"] + STREAMED)
    assert "the argument '--nearest <k>' cannot be used with '--stream <stream>'" in err
