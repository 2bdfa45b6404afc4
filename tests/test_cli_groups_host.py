"""CPU: the `--groups`, `--groups-within` and `--per-record` surface of the `distance` CLI without a GPU: the help lines,
every usage error, which parse_args reports (exit 2, `error: ...`, nothing on stdout) before any GPU work, and the label
file's errors (exit 1), which are reported before the device is looked at."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
GROUPS, WITHIN, PER_RECORD = "--groups <FILE>", "--groups-within <T>", "--per-record"
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def files(tmp_path, labels=b"x\tone\ny\ttwo\n"):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACGG\n")
    (tmp_path / "g.tsv").write_bytes(labels)


def run(tmp_path, args):
    files(tmp_path)
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")).replace("{g}", str(tmp_path / "g.tsv"))
            for x in args]
    if not any(x.endswith("a.fasta") for x in args):
        args.append(str(tmp_path / "a.fasta"))
    r = subprocess.run([CLI] + args, capture_output=True, env=NO_GPU)
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
    return r.stderr.decode()


def test_help_lists_the_mode():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    line = [x for x in lines if "--groups <FILE>" in x]
    assert len(line) == 1 and "id<TAB>group" in line[0] and "1024 groups" in line[0] and "12th decimal" in line[0]
    line = [x for x in lines if "--groups-within <T>" in x]
    assert len(line) == 1 and "'within' column" in line[0]
    line = [x for x in lines if "--per-record" in x]
    assert len(line) == 1 and "one line per record" in line[0]


MODES = [(["-s", "{b}"], "--stream <stream>"), (["--stream", "{b}"], "--stream <stream>"),
         (["--nearest", "2"], "--nearest <k>"), (["--closest", "2"], "--closest <k>"), (["--within", "2"], "--within <T>"),
         (["--clusters", "3"], "--clusters <T>"), (["--matrix", "tsv"], "--matrix <format>"),
         (["--matrix", "phylip"], "--matrix <format>"), (["--tree", "nj"], "--tree <method>"),
         (["--bootstrap", "5"], "--bootstrap <B>"), (["--tree", "nj", "--bootstrap", "5"], "--tree <method>"), (["--mst"], "--mst"),
         (["--dendrogram", "average"], "--dendrogram <linkage>"), (["--max-distance", "4"], "--max-distance <T>"),
         (["--max-distance", "4", "--sites"], "--max-distance <T>"), (["--sites"], "--sites"),
         (["--summary", "4"], "--summary <T>"), (["--histogram", "2"], "--histogram <W>"),
         (["--gpus", "2"], "--gpus <n>"), (["--devices", "0,1"], "--devices <list>")]
OWN = [["--groups", "{g}"], ["--groups={g}", "--groups-within", "2"], ["--per-record", "--groups", "{g}"]]


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("mode, other", MODES)
@pytest.mark.parametrize("own", OWN, ids=["groups", "groups-within", "per-record"])
def test_usage_errors(tmp_path, own, mode, other, first):
    err = run(tmp_path, own + mode if first else mode + own)
    assert f"the argument '{GROUPS}' cannot be used with '{other}'" in err, err
    if "gpus" in other or "devices" in other:
        assert "naming more than one GPU" in err


@pytest.mark.parametrize("args, name", [(["--groups-within", "2"], WITHIN), (["--groups-within=inf", "--summary", "2"], WITHIN),
                                        (["--per-record"], PER_RECORD), (["--per-record", "--clusters", "3"], PER_RECORD)])
def test_modifiers_require_groups(tmp_path, args, name):
    err = run(tmp_path, args)
    assert f"the argument '{name}' requires '{GROUPS}'" in err, err


@pytest.mark.parametrize("value, why", [("abc", "not a number"), ("nan", "not a number"), ("5x", "not a number"),
                                        ("", "not a number"), ("-1", "the threshold must not be negative"),
                                        ("-inf", "the threshold must not be negative")])
def test_invalid_thresholds(tmp_path, value, why):
    err = run(tmp_path, ["--groups", "{g}", f"--groups-within={value}"])
    assert f"invalid value '{value}' for '{WITHIN}': {why}" in err, err


@pytest.mark.parametrize("flag, name", [("--groups", GROUPS), ("--groups-within", WITHIN)])
def test_value_is_required(tmp_path, flag, name):
    files(tmp_path)
    r = subprocess.run([CLI, str(tmp_path / "a.fasta"), flag], capture_output=True, env=NO_GPU)
    assert r.returncode == 2 and r.stdout == b""
    assert f"a value is required for '{name}' but none was supplied" in r.stderr.decode()


@pytest.mark.parametrize("args, name", [(["--groups", "{g}", "--groups={g}"], GROUPS),
                                        (["--groups", "{g}", "--groups-within", "1", "--groups-within=2"], WITHIN)])
def test_repeated_flag(tmp_path, args, name):
    err = run(tmp_path, args)
    assert f"the argument '{name}' cannot be used multiple times" in err


def label_error(tmp_path, labels, extra=()):
    files(tmp_path, labels)
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "a.fasta")] + list(extra), capture_output=True, env=NO_GPU)
    assert r.returncode == 1 and r.stdout == b"", r.stderr
    err = r.stderr.decode()
    assert err.startswith('Error: Message("--groups: '), err
    assert "no MI355X" not in err
    return err


def test_label_file_errors(tmp_path):
    assert "line 3 of" in label_error(tmp_path, b"x\tone\n\ny two\n") and "has no tab" in label_error(tmp_path, b"x\tone\n\ny two\n")
    err = label_error(tmp_path, b"x\tone\ny\t\n")
    assert "line 2 of" in err and "empty group" in err
    err = label_error(tmp_path, b"x\tone\ny\ttwo\n\nx\tone\nx\ttwo\n")
    assert "line 5 of" in err and "gives 'x' the group 'two', line 1 gave it 'one'" in err
    err = label_error(tmp_path, b"x\tone\tmore\n")
    assert "line 1 of" in err and "more than two fields" in err
    err = label_error(tmp_path, b"p\tone\nq\ttwo\n")
    assert "no record of the first input has a group" in err


def test_label_file_errors_two_inputs(tmp_path):
    files(tmp_path, b"x\tone\n")
    (tmp_path / "b.fasta").write_bytes(b">p\nACGT\n>q\nACGA\n")
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")],
                       capture_output=True, env=NO_GPU)
    assert r.returncode == 1 and b"no record of the second input has a group" in r.stderr


def test_more_than_1024_groups(tmp_path):
    n = 1026
    (tmp_path / "a.fasta").write_bytes(b"".join(b">r%d\nACGT\n" % k for k in range(n)))
    # the file lists the records backwards: numbering follows the records, so r1024's line (line 2) starts group 1025
    (tmp_path / "g.tsv").write_bytes(b"".join(b"r%d\tg%d\n" % (k, k) for k in reversed(range(n))))
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "a.fasta")], capture_output=True, env=NO_GPU)
    assert r.returncode == 1 and r.stdout == b""
    err = r.stderr.decode()
    assert "line 2 of" in err and "starts group 1025 of the first input: more than 1024 groups" in err, err
    # 1,024 groups pass the label checks and reach the device stage
    (tmp_path / "g.tsv").write_bytes(b"".join(b"r%d\tg%d\n" % (k, k % 1024) for k in range(n)))
    r = subprocess.run([CLI, "--groups", str(tmp_path / "g.tsv"), str(tmp_path / "a.fasta")], capture_output=True, env=NO_GPU)
    assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr


def test_missing_label_file(tmp_path):
    files(tmp_path)
    r = subprocess.run([CLI, "--groups", str(tmp_path / "nope.tsv"), str(tmp_path / "a.fasta")], capture_output=True, env=NO_GPU)
    assert r.returncode == 1 and b"NotFound" in r.stderr and b"nope.tsv" in r.stderr


def test_valid_values_reach_the_gpu_stage(tmp_path):
    """Valid values parse and the labels check out: without a device the run ends at the device check, exit 1, not 2; ids of
    the file that are not in the input are skipped with one warning line."""
    files(tmp_path, b"x\tone\r\ny\ttwo\n\nw\tthree\nv\tthree\n")
    for args in (["--groups", "{g}"], ["--groups={g}", "--groups-within", "0"], ["--groups", "{g}", "--groups-within=inf", "--per-record"],
                 ["-m", "tn93", "--groups", "{g}", "--slab-pairs", "5", "{a}", "{b}"], ["--groups", "{g}", "-o", str(tmp_path / "out.tsv")]):
        args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")).replace("{g}", str(tmp_path / "g.tsv"))
                for x in args]
        if not any(x.endswith("a.fasta") for x in args):
            args.append(str(tmp_path / "a.fasta"))
        r = subprocess.run([CLI] + args, capture_output=True, env=NO_GPU)
        assert r.returncode == 1 and b"no MI355X / HIP device visible" in r.stderr, (args, r.stderr)
        assert r.stderr.count(b"warning: --groups: 2 ids of") == 1 and b"are not in the input and were skipped" in r.stderr
