"""Host side of the window-closest stream (dst_stream_open_window_closest / --window-closest): the symbols, the designed
set held to its design with the oracle, and the CLI's usage errors before any device is opened.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import to_fasta_bytes
from window_closest_cases import (ALL_N, COPIES_OF_LOADED_0, CUTS, DUPLICATES, L, LOADED_SIZES, MAX_RECORDS, N_CODE, N_STREAMED,
                                  TIE_CUT, WINDOWS, batch_of, batches, loaded_set, reference, sorted_keys, streamed_set)
from window_nearest_reference import keys, take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
ERR_ARG = 1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed():
    lib = da.load()
    for name, n_args in (("dst_stream_open_window_closest", 11), ("dst_stream_window_closest_result", 7)):
        assert name in da.declared_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == n_args and _lib._SIGS[name][0] is C.c_int
    assert hasattr(da.Engine, "window_closest_stream") and issubclass(da.WindowClosestStream, da.engine.Stream)
    for method in ("push", "pop", "next_index", "result"):
        assert callable(getattr(da.WindowClosestStream, method))


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_null_arguments_are_err_arg():
    lib = da.load()
    w = np.zeros(1, np.uint64)
    h = C.c_void_p()
    assert lib.dst_stream_open_window_closest(None, 2, 3, w.ctypes.data, w.ctypes.data, 1, 0, 4, 3, 0, C.byref(h)) == ERR_ARG
    idx, ku = np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    assert lib.dst_stream_window_closest_result(None, idx.ctypes.data, None, None, None, 4, ku.ctypes.data_as(_lib._u32p)) == ERR_ARG


# ---- the designed set -----------------------------------------------------------------------------------------------------
def test_the_set_is_what_the_design_says():
    loaded, streamed = loaded_set(), streamed_set()
    assert loaded.shape == (9, L) and streamed.shape == (N_STREAMED, L) and L == 300 and LOADED_SIZES == (1, 8, 9)
    assert WINDOWS.tolist() == [[0, 300], [5, 133], [128, 256], [130, 131], [7, 7], [299, 300], [5, 133], [0, 128]]
    assert (streamed[ALL_N] == N_CODE).all()
    for at in COPIES_OF_LOADED_0:
        assert np.array_equal(streamed[at], loaded[0])
    for a, b in DUPLICATES:
        assert np.array_equal(streamed[a], streamed[b])
    for cut in CUTS:
        assert sum(cut) == N_STREAMED and max(cut) <= MAX_RECORDS
        # at least one pair of exact duplicates falls in different batches of every cut
        assert any(batch_of(cut, a) != batch_of(cut, b) for a, b in DUPLICATES), cut
    assert batches(TIE_CUT) == [(0, 64), (64, 129), (129, 300)]
    assert all(batch_of(TIE_CUT, a) != batch_of(TIE_CUT, b) for a, b in DUPLICATES[:3])


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_the_reference_meets_the_designed_edges(measure):
    loaded, streamed = loaded_set(), streamed_set()
    index, payloads = reference(measure, loaded, streamed, 3)
    assert index.shape == (9, len(WINDOWS), 3)
    # the empty window lists ordinals 0, 1, 2
    assert (index[:, 4] == np.array([0, 1, 2], np.uint32)).all()
    # a list whose 3rd and 4th candidates are at equal key, in different batches of the cut [64, 65, 171]
    order, kk = sorted_keys(payloads)
    tie = kk[:, :, 2] == kk[:, :, 3]
    split = np.vectorize(lambda a, b: batch_of(TIE_CUT, a) != batch_of(TIE_CUT, b))(order[:, :, 2], order[:, :, 3])
    assert (tie & split).any()
    # ... the designed one: loaded record 0 over the whole width, its four copies at distance 0
    assert order[0, 0, :4].tolist() == list(COPIES_OF_LOADED_0) and index[0, 0].tolist() == list(COPIES_OF_LOADED_0[:3])
    assert (keys(take(payloads, index))[0, 0] == keys(np.zeros(1, payloads.dtype))[0]).all()
    # the all-N record sorts last for raw (NaN); for n it is as near as a record can be
    if measure == "raw":
        assert np.isnan(payloads[:, :, ALL_N]).all()
        assert (keys(payloads)[:, :, ALL_N] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        # (a one-site window has other records without a value, at later ordinals; over the longer windows it is the only one)
        assert (order[[0, 1, 2, 6, 7]][:, :, -1] == ALL_N).all()
    else:
        assert not payloads[:, :, ALL_N].any()
    # every prefix of the loaded set reads the same rows
    for n in LOADED_SIZES:
        assert np.array_equal(reference(measure, loaded[:n], streamed, 3)[0], index[:n])


# ---- the CLI's refusals, before any device is opened ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_closest_host")
    codes = loaded_set()[:3, :40]
    fasta = d / "a.fasta"
    fasta.write_bytes(b"".join(b">r%d\n%s\n" % (k, to_fasta_bytes(r)) for k, r in enumerate(codes)))
    good = d / "good.tsv"
    good.write_bytes(b"g1\t1\t40\n\ng2\t7\t7\n")
    return d, str(fasta), str(good)


def run_cli(args, stdin=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI] + args, input=stdin, capture_output=True, env=env, timeout=60)


def refused(args, message):
    r = run_cli(args)
    first = r.stderr.decode().splitlines()[0]
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, first)
    assert first.startswith("error: " + message), (args, first)


def test_usage_refusals(files):
    _, fasta, good = files
    mine = "the argument '--window-closest <K>' "
    stream = ["-i", fasta, "-s", fasta]
    cases = [
        (["--window-closest", "3"] + stream, mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--window-closest", "3", fasta], mine + "requires '--windows <W>' or '--regions <FILE>'"),
        (["--windows", "5", "--window-closest", "3", fasta], mine + "requires '--stream <stream>'"),
        (["--regions", good, "--window-closest", "3", fasta], mine + "requires '--stream <stream>'"),
        (["--windows", "5", "--window-closest", "3", "-i", fasta, fasta, "-s", fasta], mine + "takes one loaded alignment, not two"),
        (["--windows", "5", "--window-closest", "3", "-s", fasta, fasta, fasta], mine + "takes one loaded alignment, not two"),
        (["--windows", "5", "--window-closest", "0"] + stream, "invalid value '0' for '--window-closest <K>': 0 is not in 1..=256"),
        (["--windows", "5", "--window-closest", "257"] + stream, "invalid value '257' for '--window-closest <K>': 257 is not in 1..=256"),
        (["--regions", good, "--window-closest", "x"] + stream, "invalid value 'x' for '--window-closest <K>'"),
        (["--windows", "5", "--window-closest", "-1"] + stream, "invalid value '-1' for '--window-closest <K>'"),
        (["--windows", "5", "--window-closest", "3", "--window-closest", "3"] + stream, mine + "cannot be used multiple times"),
        (["--windows", "5", "--window-closest", "3", "--gpus", "2"] + stream, mine + "cannot be used with '--gpus <n>' naming more than one GPU"),
        (["--regions", good, "--window-closest", "3", "--devices", "0,1"] + stream,
         mine + "cannot be used with '--devices <list>' naming more than one GPU"),
        (["--window-closest"], "a value is required for '--window-closest <K>' but none was supplied"),
        (["--windows", "5", "--regions", good, "--window-closest", "3"] + stream,
         "the argument '--windows <W>' cannot be used with '--regions <FILE>'"),
        (["--step", "2", "--regions", good, "--window-closest", "3"] + stream, "the argument '--step <S>' requires '--windows <W>'"),
    ]
    others = [["--window-nearest", "2"], ["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"],
              ["--clusters", "1"], ["--representatives", "1"], ["--max-distance", "1"], ["--summary", "1"], ["--groups", good],
              ["--groups-within", "1"], ["--per-record"], ["--histogram", "1"], ["--bins", "4"], ["--matrix", "tsv"], ["--tree", "nj"],
              ["--bootstrap", "2"], ["--seed", "2"], ["--mst"], ["--sites"], ["--dendrogram", "average"], ["--pairs", good]]
    for other in others:
        for windows in (["--windows", "5"], ["--regions", good]):
            cases.append((windows + ["--window-closest", "3"] + other + stream, mine + f"cannot be used with '{other[0]}"))
            cases.append((other + windows + ["--window-closest", "3"] + stream, mine + f"cannot be used with '{other[0]}"))
    for args, message in cases:
        refused(args, message)


def test_the_existing_refusals_stay(files):
    _, fasta, good = files
    refused(["--windows", "5", "-s", fasta, fasta], "the argument '--windows <W>' cannot be used with '--stream <stream>'")
    refused(["--regions", good, "--stream", fasta, fasta], "the argument '--regions <FILE>' cannot be used with '--stream <stream>'")
    refused(["--windows", "5", "--window-nearest", "3", "-s", fasta, fasta],
            "the argument '--window-nearest <K>' cannot be used with '--stream <stream>'")


@pytest.mark.parametrize("args", [["--windows", "10", "--step", "5", "--window-closest", "2"],
                                  ["--window-closest", "256", "--regions", None, "-m", "tn93"],
                                  ["--windows", "10", "--window-closest=1", "--slab-pairs", "1", "-o", "out.tsv"]])
def test_an_accepted_line_ends_at_the_missing_device(files, args):
    d, fasta, good = files
    args = [good if a is None else str(d / a) if a == "out.tsv" else a for a in args]
    r = run_cli(args + ["-i", fasta, "-s", fasta])
    assert r.returncode == 1 and r.stdout == b"" and b"no MI355X / HIP device visible" in r.stderr
    r = run_cli(args + [fasta, "-s", "-"], stdin=open(fasta, "rb").read())
    assert r.returncode == 1 and r.stdout == b"" and b"no MI355X / HIP device visible" in r.stderr


def test_help_names_the_flag():
    r = run_cli(["--help"])
    lines = [x for x in r.stdout.decode().splitlines() if x.lstrip().startswith("--window-closest <K>")]
    assert r.returncode == 0 and len(lines) == 1 and "1-256" in lines[0] and "--stream" in lines[0]
