"""The usage surface of the `distance` CLI as a list of cases: plain Python, no GPU.

parse_args decides everything a case observes before any thread starts, so the outcome of a case is deterministic: the
exit code, the length of stdout and the first line of stderr.  `cases()` lists the argument vectors, `run_all(cli)` runs
them (HIP_VISIBLE_DEVICES=-1: a case that passes the parser stops at the device check, exit 1) and
tools/record_cli_usage.py stores the outcomes of a known-good binary in tests/cli_usage_outcomes.json, which
test_cli_usage_table_host.py holds every later binary to.

Two families:
  * subsets: one loaded file plus every subset of size 0-3 of the 26 argument groups below, in the groups' order (both
    --matrix forms together are skipped: the scan keeps the last, which the value cases pin).  These pin the table of
    output modes: which flag is named, by which mode, and in which order the checks speak.
  * values: for every flag that takes a value (all but --input, whose value count is its own rule, and the
    --host-selftest hook), each of VALUE_WORDS as `--flag=word`, alone and after a pair of modes that refuse each other
    (a bad value is reported in argv order, ahead of any conflict); the flag last without a value; the flag twice.
"""
import hashlib
import itertools
import json
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

FASTA = b">x\nACGT\n>y\nACGA\n"
LABELS = b"x\tg1\ny\tg2\n"
TMP_TOKEN = "{tmp}"

GROUPS = (
    ("-s", "{b}"), ("{c}",), ("--nearest", "2"), ("--closest", "2"), ("--closest-for", "streamed"), ("--within", "3"),
    ("--clusters", "3"), ("--max-distance", "4"), ("--summary", "5"), ("--histogram", "2"), ("--bins", "8"),
    ("--groups", "{g}"), ("--groups-within", "2"), ("--per-record",), ("--matrix", "tsv"), ("--matrix", "phylip"),
    ("--tree", "nj"), ("--bootstrap", "5"), ("--seed", "7"), ("--mst",), ("--sites",), ("--dendrogram", "average"),
    ("--gpus", "2"), ("--devices", "0,1"), ("--slab-pairs", "100"), ("-m", "n"),
)

VALUE_WORDS = ("", "abc", "nan", "5x", " 5", "-1", "-inf", "0", "0.5", "1e3", "inf", "257", "4097", "10001",
               "99999999999999999999")

# flag -> two different values it accepts (the repeat case)
VALUE_FLAGS = {
    "--stream": ("{b}", "{c}"), "--measure": ("n", "raw"), "--output": ("out1.tsv", "out2.tsv"), "--threads": ("2", "3"),
    "--batchsize": ("2", "3"), "--gpus": ("1", "2"), "--devices": ("0", "1"), "--slab-pairs": ("100", "200"),
    "--nearest": ("2", "3"), "--closest": ("2", "3"), "--closest-for": ("loaded", "streamed"), "--within": ("3", "4"),
    "--clusters": ("3", "4"), "--max-distance": ("4", "5"), "--summary": ("5", "6"), "--groups": ("{g}", "{b}"),
    "--groups-within": ("2", "3"), "--histogram": ("2", "3"), "--bins": ("8", "9"), "--matrix": ("tsv", "phylip"),
    "--tree": ("nj", "nj"), "--bootstrap": ("5", "6"), "--seed": ("7", "8"), "--dendrogram": ("average", "complete"),
}
CONFLICT = ("--nearest", "2", "--clusters", "3")   # '--clusters <T>' cannot be used with '--nearest <k>'


def subset_cases():
    out = []
    for size in range(4):
        for subset in itertools.combinations(range(len(GROUPS)), size):
            chosen = [GROUPS[k] for k in subset]
            if ("--matrix", "tsv") in chosen and ("--matrix", "phylip") in chosen:
                continue
            out.append(["{a}"] + [word for group in chosen for word in group])
    return out


def value_cases():
    out = []
    for flag, (v1, v2) in VALUE_FLAGS.items():
        for word in VALUE_WORDS:
            out.append(["{a}", f"{flag}={word}"])
            out.append(["{a}", *CONFLICT, f"{flag}={word}"])
        out.append(["{a}", flag])
        out.append(["{a}", flag, v1, flag, v2])
    return out


def cases():
    return subset_cases() + value_cases()


def cases_digest(case_list):
    return hashlib.sha256(json.dumps(case_list).encode()).hexdigest()


def run_case(cli, tmp, args):
    """(exit code, len(stdout), first line of stderr with the temporary directory as a token)"""
    paths = {name: os.path.join(tmp, f"{name}.fasta") for name in "abc"}
    paths["g"] = os.path.join(tmp, "labels.tsv")
    argv = [cli] + [word.format(**paths) if "{" in word else word for word in args]
    # relative words are read by --stream / --groups and written by --output: the writers get a directory of their own
    cwd = os.path.join(tmp, "written" if any(word.startswith("--output") for word in args) else "empty")
    r = subprocess.run(argv, stdin=subprocess.DEVNULL, capture_output=True, cwd=cwd,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    first = r.stderr.decode(errors="replace").split("\n", 1)[0].replace(tmp, TMP_TOKEN)
    return [r.returncode, len(r.stdout), first]


def run_all(cli, case_list=None, workers=8):
    case_list = cases() if case_list is None else case_list
    with tempfile.TemporaryDirectory(prefix="cli_usage_") as tmp:
        tmp = os.path.realpath(tmp)
        for name in "abc":
            with open(os.path.join(tmp, f"{name}.fasta"), "wb") as fh:
                fh.write(FASTA)
        with open(os.path.join(tmp, "labels.tsv"), "wb") as fh:
            fh.write(LABELS)
        for name in ("written", "empty"):
            os.mkdir(os.path.join(tmp, name))
        with ThreadPoolExecutor(workers) as pool:
            return list(pool.map(lambda args: run_case(cli, tmp, args), case_list))


def pack(outcomes):
    """The fixture's form: every message once, every distinct outcome once, an index per case."""
    messages = sorted({o[2] for o in outcomes})
    at = {m: k for k, m in enumerate(messages)}
    distinct = sorted({(o[0], o[1], at[o[2]]) for o in outcomes})
    where = {o: k for k, o in enumerate(distinct)}
    return {"messages": messages, "outcomes": [list(o) for o in distinct],
            "cases": [where[(o[0], o[1], at[o[2]])] for o in outcomes]}


def unpack(fixture):
    return [[fixture["outcomes"][k][0], fixture["outcomes"][k][1], fixture["messages"][fixture["outcomes"][k][2]]]
            for k in fixture["cases"]]
