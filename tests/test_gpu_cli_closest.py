"""GPU (-m gpu): `distance --closest K [--closest-for loaded|streamed] -i loaded.fasta -s big.fasta` end to end — every
line is byte for byte the line the full `-s` run prints for that pair, and the lines are the expected ones in the expected
order (tests/closest_reference.py on the plain stream's values), with both wire formats, from a file and from stdin."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import oracle
from closest_reference import expected_for_loaded, expected_for_streamed, plain_truth
from helpers import random_alignment, to_fasta_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
HEADER = "sequence1\tsequence2\tdistance\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def fasta(prefix, seqs):
    ids = [f"{prefix}{r}" for r in range(len(seqs))]
    return ids, b"".join(b">" + i.encode() + b" description\n" + s + b"\n" for i, s in zip(ids, seqs))


def run(args, stdin=None, wire=None):
    env = {k: v for k, v in os.environ.items() if k != "DISTANCE_WIRE"}
    if wire:
        env["DISTANCE_WIRE"] = wire
    r = subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def expected_text(full_text, lids, sids, index, side):
    """the full run's lines of the chosen pairs, in the documented order"""
    lines = full_text.splitlines(keepends=True)
    assert lines[0] == HEADER and len(lines) == 1 + len(lids) * len(sids)
    by_pair = {}
    for line in lines[1:]:
        a, b, _ = line.split("\t")
        by_pair[a, b] = line
    out = [HEADER]
    if side == "loaded":
        out += [by_pair[lids[i], sids[int(o)]] for i in range(len(lids)) for o in index[i]]
    else:
        out += [by_pair[lids[int(j)], sids[s]] for s in range(len(sids)) for j in index[s]]
    return "".join(out)


def check(tmp_path, measure, side, k, loaded_seqs, streamed_seqs, slab_pairs, wires=(None, "codes"), sources=("file", "stdin")):
    lids, ltext = fasta("a", loaded_seqs)
    sids, stext = fasta("b", streamed_seqs)
    (tmp_path / "a.fasta").write_bytes(ltext)
    (tmp_path / "b.fasta").write_bytes(stext)
    a, b = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    common = ["-m", measure, "--slab-pairs", str(slab_pairs), "-i", a]
    full = run(common + ["-s", b])
    # the order is that of the device's values: the plain stream with the counts the CLI hands over (upper case only)
    enc = [oracle.encode_count_bases(s) for s in streamed_seqs]
    codes, counts = np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]).astype(np.uint32)
    with da.Engine(0) as eng:
        eng.upload(0, np.stack([oracle.encode(s) for s in loaded_seqs]))
        S, T = plain_truth(eng, measure, codes, counts if measure == "tn93" else None, max_records=64)
    index = (expected_for_loaded if side == "loaded" else expected_for_streamed)(S, T, k)[0]
    want = expected_text(full, lids, sids, index, side)
    flags = ["--closest", str(k)] + ([] if side == "loaded" else ["--closest-for", "streamed"])
    for wire in wires:
        for source in sources:
            if source == "file":
                got = run(common + flags + ["-s", b], wire=wire)
            else:
                got = run(common + flags + ["-s", "-"], stdin=stext, wire=wire)
            assert got == want, (measure, side, wire, source)
    return want


def letters(codes):
    return [to_fasta_bytes(r) for r in codes]


@pytest.mark.parametrize("measure", ["raw", "tn93"])
@pytest.mark.parametrize("side", ["loaded", "streamed"])
def test_lines_are_the_full_runs_in_the_expected_order(tmp_path, side, measure):
    loaded = random_alignment(70, 500, seed=131)
    streamed = random_alignment(150, 500, seed=132)
    streamed[40] = streamed[7]                        # ties across batches (16 records each) ...
    streamed[41] = loaded[3]                          # ... and a streamed record equal to a loaded one
    want = check(tmp_path, measure, side, 4, letters(loaded), letters(streamed), slab_pairs=70 * 16)
    assert want.count("\n") == 1 + (70 if side == "loaded" else 150) * 4


@pytest.mark.parametrize("side", ["loaded", "streamed"])
def test_fewer_records_than_k(tmp_path, side):
    loaded = random_alignment(3 if side == "streamed" else 20, 200, seed=133)
    streamed = random_alignment(3 if side == "loaded" else 20, 200, seed=134)
    want = check(tmp_path, "raw", side, 5, letters(loaded), letters(streamed), slab_pairs=1 << 22, wires=(None,), sources=("file",))
    assert want.count("\n") == 1 + 20 * 3             # k_used = 3 on either side


@pytest.mark.parametrize("side", ["loaded", "streamed"])
def test_lower_case_streamed_letters_with_tn93(tmp_path, side):
    """the caller's base counts see upper-case letters only (src/fastaio.rs:136-142): the lines are still the full run's"""
    loaded = random_alignment(20, 300, seed=135, p_ambig=0, p_gap=0)
    streamed = random_alignment(30, 300, seed=136, p_ambig=0, p_gap=0)
    seqs = letters(streamed)
    seqs = [s[:100].lower() + s[100:] if r % 2 else s for r, s in enumerate(seqs)]
    check(tmp_path, "tn93", side, 3, letters(loaded), seqs, slab_pairs=20 * 8, wires=(None,), sources=("file",))
