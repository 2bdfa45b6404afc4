"""GPU (-m gpu): `distance --stream-groups FILE [--stream-groups-by cell|streamed|loaded] [--stream-groups-within T]` with
`-i loaded.fasta -s big.fasta`, end to end.  The yardstick is the loaded-set form of the same question: `--groups FILE
big.fasta loaded.fasta` for the cells, the same with `--per-record` for the streamed side, byte for byte; the loaded side is
`--groups FILE --per-record loaded.fasta big.fasta` for `-m n` and, for every measure, the lines formatted from
GroupSummaryStream.result() the way test_gpu_cli_groups.py forms its expected lines.  Every mode also with -o, `-s -` and
DISTANCE_WIRE=codes; --slab-pairs bounds the batches at 17 records, so the 70 streamed records come in five."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from helpers import random_alignment, to_fasta_bytes
from test_gpu_cli_groups import records_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
N_L, N_S, L = 40, 70, 300
SMALL = ["--slab-pairs", str(17 * N_L)]
ABSENT = 3                                            # ids of the label file that neither input carries
WARNING = f"warning: --stream-groups: {ABSENT} ids of "


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def launch(args, stdin=None, wire=None):
    env = {k: v for k, v in os.environ.items() if k != "DISTANCE_WIRE"}
    if wire:
        env["DISTANCE_WIRE"] = wire
    return subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env)


def run(args, stdin=None, wire=None):
    r = launch(args, stdin, wire)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def fasta(prefix, codes):
    return b"".join(b">" + f"{prefix}{r}".encode() + b" description\n" + to_fasta_bytes(row) + b"\n" for r, row in enumerate(codes))


def loaded_label(r):
    return None if r % 8 == 4 else ("north", "south", "east")[r % 3]


def streamed_label(r):
    """the streamed groups appear in the order west, north, up, down: `north` names a loaded group too"""
    return None if r % 9 == 5 else ("west", "north", "up", "down")[(r // 3) % 4]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_groups")
    both = random_alignment(N_L + N_S, L, seed=441)   # upper-case FASTA with IUPAC codes and gaps
    loaded, streamed = both[:N_L], both[N_L:]
    streamed[40] = streamed[7]                        # equal records across batches ...
    streamed[41] = loaded[3]                          # ... a streamed record equal to a loaded one: min 0
    streamed[50] = 240                                # ... and an all-N record on either side: NaN
    loaded[9] = 240
    (d / "a.fasta").write_bytes(fasta("a", loaded))
    (d / "b.fasta").write_bytes(fasta("b", streamed))
    lines = [f"a{r}\t{loaded_label(r)}\n" for r in range(N_L) if loaded_label(r)]
    lines += [f"b{r}\t{streamed_label(r)}\n" for r in range(N_S) if streamed_label(r)]
    lines += [f"nobody{k}\tnorth\n" for k in range(ABSENT)]
    (d / "g.tsv").write_text("".join(reversed(lines)))   # the file's order is not the records'
    return str(d / "a.fasta"), str(d / "b.fasta"), str(d / "g.tsv"), d, loaded, streamed


def within_of(measure):
    return "3" if measure in da.INT_MEASURES else "0.03"


@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("measure", ALL)
def test_cells_are_the_groups_of_the_two_loaded_files(files, measure, within):
    a, b, g = files[:3]
    T = within_of(measure)
    want = run(["-m", measure, "--groups", g] + (["--groups-within", T] if within else []) + [b, a])
    lines = want.splitlines()
    assert lines[0] == "group1\tgroup2\tpairs\tcompared" + ("\twithin" if within else "") + "\tmean\tmin\tmax"
    assert [x.split("\t")[:2] for x in lines[1:4]] == [["west", "north"], ["west", "south"], ["west", "east"]] and len(lines) == 13
    got = run(["-m", measure, "--stream-groups", g] + (["--stream-groups-within", T] if within else []) + SMALL + ["-i", a, "-s", b])
    assert got == want


@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("measure", ALL)
def test_streamed_side_is_per_record_of_the_two_loaded_files(files, measure, within):
    a, b, g = files[:3]
    T = within_of(measure)
    want = run(["-m", measure, "--groups", g, "--per-record"] + (["--groups-within", T] if within else []) + [b, a])
    lines = want.splitlines()
    assert lines[0] == "sequence\tgroup\tcompared" + ("\twithin" if within else "") + "\tmean" and len(lines) == 1 + 3 * N_S
    assert lines[1].startswith("b0\tnorth\t") and lines[3 * 5 + 1].startswith("b5\tnorth\t")       # b5 has no label: a row all the same
    got = run(["-m", measure, "--stream-groups", g, "--stream-groups-by", "streamed"] +
              (["--stream-groups-within", T] if within else []) + SMALL + ["-i", a, "-s", b])
    assert got == want


@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("measure", ALL)
def test_loaded_side(files, measure, within):
    a, b, g, _, loaded, streamed = files
    T = within_of(measure)
    names = ["west", "north", "up", "down"]
    sg = np.array([-1 if streamed_label(r) is None else names.index(streamed_label(r)) for r in range(N_S)])
    with da.Engine(0) as eng:
        eng.upload(0, loaded)
        with eng.group_summary_stream(measure, N_S, n_streamed_groups=4, threshold=float(T) if within else float("inf"),
                                      loaded=True) as st:
            st.push(streamed, groups=sg)
            st.pop()
            res = st.result()
    want = records_text([f"a{r}" for r in range(N_L)], res, names, within)
    mode = ["--stream-groups", g, "--stream-groups-by", "loaded"] + (["--stream-groups-within", T] if within else [])
    assert run(["-m", measure] + mode + SMALL + ["-i", a, "-s", b]) == want
    assert want.count("\n") == 1 + 4 * N_L and "a4\twest\t" in want                                # a4 has no label: a row all the same
    if measure == "n":
        assert want == run(["-m", "n", "--groups", g, "--per-record"] + (["--groups-within", T] if within else []) + [a, b])


@pytest.mark.parametrize("by", ["cell", "streamed", "loaded"])
def test_output_file_stdin_wire_and_batch_bounds(files, by):
    a, b, g, d = files[:4]
    base = ["-m", "k80", "--stream-groups", g, f"--stream-groups-by={by}", "--stream-groups-within=0.03"]
    want = run(base + SMALL + ["-i", a, "-s", b])
    assert want.count("\n") == {"cell": 13, "streamed": 1 + 3 * N_S, "loaded": 1 + 4 * N_L}[by]
    assert run(base + SMALL + ["-i", a, "-s", b], wire="codes") == want
    assert run(base + ["--slab-pairs", str(3 * N_L), "-i", a, "-s", b]) == want
    assert run(base + ["-i", a, "-s", b]) == want                                  # one batch
    with open(b, "rb") as fh:
        assert run(base + SMALL + [a, "-s", "-"], stdin=fh.read()) == want
    out = d / f"{by}.tsv"
    assert run(base + SMALL + ["-o", str(out), "-i", a, "-s", b]) == ""
    assert out.read_text() == want


@pytest.mark.parametrize("by", ["cell", "streamed", "loaded"])
def test_the_warning_counts_the_ids_on_neither_side(files, by):
    a, b, g, d = files[:4]
    r = launch(["--stream-groups", g, "--stream-groups-by", by] + SMALL + ["-i", a, "-s", b])
    assert r.returncode == 0 and r.stderr.count(b"warning:") == 1 and r.stderr.decode().count(WARNING) == 1, r.stderr
    full = d / "full.tsv"
    full.write_text("".join(x for x in open(g) if not x.startswith("nobody")))
    r = launch(["--stream-groups", str(full), "--stream-groups-by", by] + SMALL + ["-i", a, "-s", b])
    assert r.returncode == 0 and b"warning:" not in r.stderr, r.stderr


def test_a_1025th_streamed_group_names_the_record(tmp_path):
    n = 1030
    codes = random_alignment(n + 2, 40, seed=442)
    (tmp_path / "a.fasta").write_bytes(fasta("a", codes[:2]))
    (tmp_path / "b.fasta").write_bytes(fasta("b", codes[2:]))
    (tmp_path / "g.tsv").write_text("a0\tzero\n" + "".join(f"b{r}\tgroup{r}\n" for r in range(n)))
    args = ["--stream-groups", str(tmp_path / "g.tsv"), "-i", str(tmp_path / "a.fasta"), "-s", str(tmp_path / "b.fasta")]
    r = launch(args)
    assert r.returncode == 1, r.stderr
    assert b"--stream-groups: the streamed record 'b1024' starts group 1025 of the stream: more than 1024 groups" in r.stderr, r.stderr
    # by streamed: no streamed labels are needed, and none is counted
    r = launch(args + ["--stream-groups-by", "streamed"])
    assert r.returncode == 0 and r.stdout.count(b"\n") == 1 + n, r.stderr
    # 1,024 groups are fine
    (tmp_path / "g.tsv").write_text("a0\tzero\n" + "".join(f"b{r}\tgroup{r % 1024}\n" for r in range(n)))
    r = launch(args)
    assert r.returncode == 0 and r.stdout.count(b"\n") == 1 + 1024, r.stderr
