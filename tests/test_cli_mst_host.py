"""CPU: the `--mst` surface of the `distance` CLI without a GPU: the help line and every usage error, which parse_args
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


def test_help_lists_mst():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--mst" in x]
    assert len(line) == 1 and "minimum spanning tree" in line[0]


@pytest.mark.parametrize("args, other", [
    (["--mst", "{b}"], None), (["--mst", "-i", "{a}", "{b}"], None),
    (["--mst", "-s", "{b}"], "--stream <stream>"), (["--mst", "--stream", "{b}"], "--stream <stream>"),
    (["--mst", "--nearest", "2"], "--nearest <k>"), (["--nearest", "2", "--mst"], "--nearest <k>"),
    (["--mst", "--clusters", "3"], "--clusters <T>"), (["--clusters", "3", "--mst"], "--clusters <T>"),
    (["--mst", "--matrix", "tsv"], "--matrix <format>"), (["--mst", "--matrix", "phylip"], "--matrix <format>"),
    (["--mst", "--tree", "nj"], "--tree <method>"), (["--tree", "nj", "--mst"], "--tree <method>"),
    (["--mst", "--bootstrap", "5"], "--bootstrap <B>"),
    (["--mst", "--gpus", "2"], "--gpus <n>"), (["--mst", "--devices", "0,1"], "--devices <list>"),
])
def test_usage_errors(tmp_path, args, other):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    if "-i" not in args:
        args.append(str(tmp_path / "a.fasta"))
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    if other is None:
        assert b"the argument '--mst' takes one input alignment, not two" in r.stderr, r.stderr
    else:
        assert f"the argument '--mst' cannot be used with '{other}'".encode() in r.stderr, r.stderr


def test_mst_takes_no_value(tmp_path):
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    r = subprocess.run([CLI, "--mst=1", str(tmp_path / "a.fasta")], capture_output=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: ")
