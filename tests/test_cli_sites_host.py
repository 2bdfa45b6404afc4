"""CPU: the `--sites` surface of the `distance` CLI without a GPU: the help line and every usage error, which parse_args
reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


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


def test_help_lists_sites():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--sites" in x]
    assert len(line) == 1 and "X<pos>Y" in line[0] and "fourth field" in line[0]


def test_sites_alone_is_a_usage_error(tmp_path):
    assert "the argument '--sites' requires '--max-distance <T>' or '--mst'" in run(tmp_path, ["--sites"])
    assert "the argument '--sites' requires '--max-distance <T>' or '--mst'" in run(tmp_path, ["-m", "n", "--sites", "{a}", "{b}"])


MODES = [(["-s", "{b}"], "--stream <stream>"), (["--nearest", "2"], "--nearest <k>"),
         (["-s", "{b}", "--closest", "2"], "--stream <stream>"), (["--clusters", "3"], "--clusters <T>"),
         (["--matrix", "tsv"], "--matrix <format>"), (["--matrix", "phylip"], "--matrix <format>"),
         (["--tree", "nj"], "--tree <method>"), (["--tree", "nj", "--bootstrap", "5"], "--tree <method>"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--summary", "2"], "--summary <T>"),
         (["--histogram", "1"], "--histogram <W>")]


@pytest.mark.parametrize("with_mode", [[], ["--max-distance", "5"], ["--mst"]])
@pytest.mark.parametrize("mode, other", MODES)
def test_other_output_modes(tmp_path, mode, other, with_mode):
    err = run(tmp_path, ["--sites"] + with_mode + mode)
    assert f"the argument '--sites' cannot be used with '{other}'" in err, err


def test_the_two_modes_still_exclude_each_other_and_more_than_one_gpu(tmp_path):
    assert "the argument '--max-distance <T>' cannot be used with '--mst'" in run(tmp_path, ["--sites", "--mst", "--max-distance", "1"])
    assert "the argument '--mst' takes one input alignment, not two" in run(tmp_path, ["--sites", "--mst", "{a}", "{b}"])
    assert "the argument '--max-distance <T>' cannot be used with '--gpus <n>'" in run(tmp_path, ["--sites", "--max-distance=1", "--gpus", "2"])
    assert "the argument '--mst' cannot be used with '--devices <list>'" in run(tmp_path, ["--mst", "--sites", "--devices", "0,1"])


def test_sites_takes_no_value(tmp_path):
    assert "unexpected argument '--sites=1' found" in run(tmp_path, ["--mst", "--sites=1"])


def test_valid_uses_reach_the_gpu_stage(tmp_path):
    """with either mode the run ends at the device check (exit 1), not at the arguments (exit 2)"""
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    a, b = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    for args in (["--mst", "--sites", a], ["--sites", "--max-distance", "3", a], ["--max-distance=3", "--sites", a, b]):
        r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)
