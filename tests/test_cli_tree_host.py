"""CPU: the `--tree nj` surface of the `distance` CLI without a GPU: the help line and every usage error, which
parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def test_help_lists_tree():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--tree" in x]
    assert len(line) == 1 and "<method>" in line[0] and "nj" in line[0]
    for other in ("--matrix", "--clusters", "--nearest"):
        assert other not in line[0]


@pytest.mark.parametrize("args", [
    ["--tree"], ["--tree", "upgma", "{a}"], ["--tree", "NJ", "{a}"], ["--tree=", "{a}"],
    ["--tree", "nj", "{a}", "{b}"], ["--tree", "nj", "-i", "{a}", "{b}"],
    ["--tree", "nj", "-i", "{a}", "-s", "{b}"], ["-i", "{a}", "--stream", "{b}", "--tree", "nj"],
    ["--tree", "nj", "--nearest", "2", "{a}"], ["--nearest", "2", "--tree", "nj", "{a}"],
    ["--tree", "nj", "--clusters", "3", "{a}"], ["--clusters", "3", "--tree=nj", "{a}"],
    ["--tree", "nj", "--matrix", "tsv", "{a}"], ["--matrix", "phylip", "--tree", "nj", "{a}"],
    ["--tree", "nj", "--gpus", "2", "{a}"], ["--tree", "nj", "--devices", "0,1", "{a}"],
])
def test_usage_errors(tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACCA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
