"""CPU: the `--clusters T` surface of the `distance` CLI without a GPU: the help line and every usage error, which
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


def test_help_lists_clusters():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--clusters" in x]
    assert len(line) == 1 and "<T>" in line[0]


@pytest.mark.parametrize("args", [
    ["--clusters", "x"], ["--clusters", "nan"], ["--clusters", "NaN"], ["--clusters", "-1"], ["--clusters", "-inf"],
    ["--clusters", ""], ["--clusters", "3x"], ["--clusters", " 3"], ["--clusters=1,5"], ["--clusters"],
    ["--clusters", "3", "{b}"], ["--clusters", "3", "-i", "{a}", "{b}"],
    ["--clusters", "3", "-s", "{b}"], ["--clusters", "3", "--nearest", "2"], ["--nearest", "2", "--clusters", "3"],
    ["--clusters", "3", "--gpus", "2"], ["--clusters", "3", "--devices", "0,1"],
])
def test_usage_errors(tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    if "-i" not in args:
        args.append(str(tmp_path / "a.fasta"))
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
