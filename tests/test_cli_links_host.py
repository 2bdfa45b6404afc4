"""CPU: the `--max-distance` surface of the `distance` CLI without a GPU: the help line and every usage error, which
parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
FLAG = "--max-distance <T>"


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


def test_help_lists_max_distance():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--max-distance" in x]
    assert len(line) == 1 and "pairs within distance T" in line[0]


MODES = [(["-s", "{b}"], "--stream <stream>"), (["--stream", "{b}"], "--stream <stream>"),
         (["--nearest", "2"], "--nearest <k>"), (["--clusters", "3"], "--clusters <T>"),
         (["--matrix", "tsv"], "--matrix <format>"), (["--matrix", "phylip"], "--matrix <format>"),
         (["--tree", "nj"], "--tree <method>"), (["--bootstrap", "5"], "--bootstrap <B>"),
         (["--tree", "nj", "--bootstrap", "5"], "--tree <method>"), (["--mst"], "--mst"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--gpus", "2"], "--gpus <n>"),
         (["--devices", "0,1"], "--devices <list>")]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", MODES)
def test_usage_errors(tmp_path, mode, other, first):
    args = ["--max-distance", "5"] + mode if first else mode + ["--max-distance=5"]
    err = run(tmp_path, args)
    assert f"the argument '{FLAG}' cannot be used with '{other}'" in err, err


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("5x", "not a number"),
                                        ("", "not a number"), ("-1", "the threshold must not be negative"),
                                        ("-inf", "the threshold must not be negative")])
def test_invalid_values(tmp_path, value, why):
    err = run(tmp_path, [f"--max-distance={value}"])
    assert f"invalid value '{value}' for '{FLAG}': {why}" in err, err


def test_value_is_required(tmp_path):
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n")
    r = subprocess.run([CLI, str(tmp_path / "a.fasta"), "--max-distance"], capture_output=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and r.stdout == b""
    assert f"a value is required for '{FLAG}' but none was supplied" in r.stderr.decode()


def test_repeated_flag(tmp_path):
    err = run(tmp_path, ["--max-distance", "5", "--max-distance", "6"])
    assert f"the argument '{FLAG}' cannot be used multiple times" in err


def test_valid_values_reach_the_gpu_stage(tmp_path):
    """0, a fraction, an exponent and inf parse: without a device the run ends at the device check, exit 1, not 2."""
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    for v in ("0", "0.5", "1e3", "inf"):
        r = subprocess.run([CLI, "--max-distance", v, str(tmp_path / "a.fasta")], capture_output=True,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (v, r.stderr)
