"""CPU: the `--dendrogram` surface of the `distance` CLI without a GPU: the help line and every usage error, which
parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
FLAG = "--dendrogram <linkage>"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def run(tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    if "-i" not in args:
        args.append(str(tmp_path / "a.fasta"))
    return subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_help_lists_dendrogram():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    line = [x for x in lines if "--dendrogram" in x]
    assert len(line) == 1 and all(w in line[0] for w in ("average", "weighted", "complete", "UPGMA", "Newick"))
    tree = [x for x in lines if x.lstrip().startswith("--tree")]
    assert len(tree) == 1 and "nj" in tree[0] and "upgma" not in tree[0].lower()


@pytest.mark.parametrize("args, other", [
    (["--dendrogram", "average", "{b}"], None), (["--dendrogram", "complete", "-i", "{a}", "{b}"], None),
    (["--dendrogram", "average", "-s", "{b}"], "--stream <stream>"),
    (["--dendrogram=weighted", "--stream", "{b}"], "--stream <stream>"),
    (["--dendrogram", "average", "--nearest", "2"], "--nearest <k>"),
    (["--nearest", "2", "--dendrogram", "average"], "--nearest <k>"),
    (["--dendrogram", "complete", "--clusters", "3"], "--clusters <T>"),
    (["--clusters", "3", "--dendrogram", "complete"], "--clusters <T>"),
    (["--dendrogram", "average", "--matrix", "tsv"], "--matrix <format>"),
    (["--dendrogram", "average", "--matrix", "phylip"], "--matrix <format>"),
    (["--dendrogram", "average", "--tree", "nj"], "--tree <method>"),
    (["--tree", "nj", "--dendrogram", "weighted"], "--tree <method>"),
    (["--tree", "nj", "--bootstrap", "5", "--dendrogram", "average"], "--tree <method>"),
    (["--dendrogram", "average", "--mst"], "--mst"), (["--mst", "--dendrogram", "average"], "--mst"),
    (["--dendrogram", "average", "--gpus", "2"], "--gpus <n>"),
    (["--dendrogram", "average", "--devices", "0,1"], "--devices <list>"),
])
def test_usage_errors(tmp_path, args, other):
    r = run(tmp_path, args)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    if other is None:
        assert f"the argument '{FLAG}' takes one input alignment, not two".encode() in r.stderr, r.stderr
    else:
        assert f"the argument '{FLAG}' cannot be used with '{other}'".encode() in r.stderr, r.stderr


def test_bootstrap_and_seed_still_ask_for_tree_nj(tmp_path):
    r = run(tmp_path, ["--dendrogram", "average", "--bootstrap", "5"])
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: ")
    assert b"requires '--tree nj'" in r.stderr
    r = run(tmp_path, ["--dendrogram", "average", "--seed", "5"])
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: ")
    assert b"'--seed <S>' requires '--bootstrap <B>'" in r.stderr


@pytest.mark.parametrize("args", [["--dendrogram", "upgma"], ["--dendrogram", "single"], ["--dendrogram", "AVERAGE"],
                                  ["--dendrogram="], ["--dendrogram", "ward"]])
def test_unknown_linkage_lists_values(tmp_path, args):
    r = run(tmp_path, args)
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: invalid value "), r.stderr
    assert b"[possible values: average, weighted, complete]" in r.stderr


def test_missing_value():
    r = subprocess.run([CLI, "--dendrogram"], capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: ")


def test_tree_upgma_is_still_a_usage_error(tmp_path):
    r = run(tmp_path, ["--tree", "upgma"])
    assert r.returncode == 2 and r.stdout == b"" and r.stderr.startswith(b"error: invalid value 'upgma'")
    assert b"[possible values: nj]" in r.stderr
