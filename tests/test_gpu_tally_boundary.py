"""GPU (-m gpu): the 16-bit tally boundary, 65,534 / 65,535 / 65,536 / 65,537 sites, on every path and every reader of
the packed form.

Up to 65,535 sites the consensus pair kernel keeps two tallies in one 32-bit word, adds the hybrid path's hot tallies as
uint16, offers DST_OUT_TALLY16, and the text kernels read 16-bit tallies; from 65,536 on everything is one tally per
word.  The designed sets of tally_boundary_cases.py (whose saturated patterns test_tally_boundary_host.py asserts on the
oracle alone) put 0, 32,768, L - 32,768 and L itself into every tally slot: at 65,535 sites the packed halves are all
ones, low halves overflow into high halves before the corrections bring them back, high halves borrow.

Exact everywhere: tallies and integer measures over the whole triangle against the oracle, bit for bit; f64 distances by
test_gpu_fuzz._close (1e-12 absolute, relative above 1e-3; NaN and inf in the same places); da.finalize of the device
tallies equal to the oracle's value.  What the engine's own rules fix, and the assertions follow:
  * dst_launch_info.wide describes the consensus / hybrid kernels; a dense launch reports 0 at any width.
  * run records are made by the fused preparation only (dst_set_prep_threshold(0) here): under the default preparation
    of a set this small the lists are built at the first run and keep every entry, run_records() is (0, 0).
  * DST_PATH_AUTO keeps a launch below the preparation threshold on the dense kernels: "auto" with the default
    preparation runs dense; with the fused preparation the cost model chooses.
  * the hybrid path needs hot columns: it runs kind "hot" (floor(L / 2) hot columns: the most it admits)."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import distance_amd as da
import nj_reference as R
import oracle
import tally_boundary_cases as tb
from test_gpu_clusters import reference as cluster_reference
from test_gpu_fuzz import _close
from test_gpu_matrix import diag_text, matrix_text
from test_gpu_nearest import canon, expected_square

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
FAMILY_OF = {"n": "n_high", "n_high": "n_high", "raw": "raw", "jc69": "raw", "k80": "k80", "tn93": "tn93"}
THREADS = min(16, len(os.sched_getaffinity(0)))
ERR_ARG = 1
PATH_KINDS = {"dense": ("plain",), "consensus": ("plain", "runs"), "hybrid": ("hot",), "auto": ("plain", "runs")}


@functools.lru_cache(maxsize=None)
def case(L, kind):
    """the designed set and the oracle's answers for it, computed once per (L, kind): tallies and distances of the whole
    triangle, and of the set against its named records (both orders)"""
    codes, names = tb.boundary_alignment(L, kind)
    n = len(codes)
    iu = np.triu_indices(n, 1)                     # canonical order
    small_idx = tb.extremes(names) + names["majority"][:3]
    small = np.ascontiguousarray(codes[small_idx])
    c = SimpleNamespace(L=L, kind=kind, codes=codes, names=names, n=n, small=small, small_idx=small_idx)
    c.tal = {f: oracle.tallies_rect(f, codes, codes, threads=THREADS)[iu] for f in set(FAMILY_OF.values())}
    c.dist = {m: oracle.all_pairs_square(m, codes, threads=THREADS) for m in ALL}
    c.counts = oracle.count_bases_matrix(codes)
    c.rect_tal = {f: oracle.tallies_rect(f, codes, small, threads=THREADS) for f in set(FAMILY_OF.values())}
    c.rect_tal_t = {f: oracle.tallies_rect(f, small, codes, threads=THREADS) for f in set(FAMILY_OF.values())}
    c.rect_dist = {m: oracle.all_pairs_rect(m, codes, small, threads=THREADS) for m in ALL}
    c.rect_dist_t = {m: oracle.all_pairs_rect(m, small, codes, threads=THREADS) for m in ALL}
    c.ij = np.stack(iu, axis=1)
    c.finalised = set()
    # run records the fused preparation makes: records with four or more whole 128-site chunks of N
    nch = -(-L // 128)
    padded = np.full((n, nch * 128), tb.N, np.uint8)
    padded[:, :L] = codes
    c.n_run = int(((padded == tb.N).reshape(n, nch, 128).all(axis=2).sum(axis=1) >= 4).sum())
    # the sets are what the host test says they are: the top of every family is L itself
    assert all(int(c.tal[f].max()) == L for f in c.tal)
    return c


def same_values(measure, got, want, what):
    """integers exactly; f64 by the criterion of test_gpu_fuzz"""
    assert got.shape == want.shape, what
    if measure in da.INT_MEASURES:
        assert got.dtype == np.int64 and np.array_equal(got, want.astype(np.int64)), what
        return
    g, w = got.ravel(), want.ravel()
    bad = [k for k in range(len(w)) if not _close(float(g[k]), float(w[k]))]
    assert not bad, (what, bad[:3], [(float(g[k]), float(w[k])) for k in bad[:3]])


def same_tallies(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.nonzero((got.astype(np.uint64) != want).any(axis=-1).ravel())[0]
    assert not len(bad), (what, bad[:3], got.reshape(-1, got.shape[-1])[bad[:3]], want.reshape(-1, want.shape[-1])[bad[:3]])


def check_host_finalisation(c, measure, tl):
    """da.finalize of the device tallies == the oracle's value of the pair, every pair (once per set and measure: the
    device tallies have just been shown to be the oracle's, whatever path wrote them)"""
    if (measure,) in c.finalised:
        return
    want = c.dist[measure]
    for k, (i, j) in enumerate(c.ij):
        host = da.finalize(measure, tl[k], c.counts[i], c.counts[j])
        ref = float(want[k])
        assert host == ref or (math.isnan(host) and math.isnan(ref)), (c.L, c.kind, measure, int(i), int(j), host, ref)
    for a, b in (("ts_all", "ts_all_copy"), ("ts_all", "tv_all"), ("pur", "pur_ts"), ("first_half", "second_half")):
        i, j = sorted((c.names[a], c.names[b]))
        ref = oracle.pair_distance(FAMILY_OF[measure] if measure == "n" else measure, c.codes[i], c.codes[j])
        assert ref == want[tb.pair_index(c.n, i, j)] or (math.isnan(ref) and math.isnan(want[tb.pair_index(c.n, i, j)]))
    c.finalised.add((measure,))


def expected_path(path, fused, last):
    if path != "auto":
        return path
    return last if fused and last in ("dense", "consensus", "hybrid") else "dense"


def check_launch(eng, c, path, fused, what):
    li, last = eng.last_launch(), eng.last_path()
    assert last == expected_path(path, fused, last) and li["path"] == last, (what, last, li)
    assert li["wide"] == (last != "dense" and c.L >= 65536), (what, li)
    assert li["pairs"] > 0


@pytest.mark.parametrize("fused", [False, True], ids=["default_prep", "fused_prep"])
@pytest.mark.parametrize("path", list(PATH_KINDS))
@pytest.mark.parametrize("L", tb.WIDTHS)
def test_whole_triangle_rectangles_and_row_ranges(L, path, fused):
    for kind in PATH_KINDS[path]:
        c = case(L, kind)
        n = c.n
        with da.Engine(0) as eng:
            if fused:
                eng.set_prep_threshold(0.0)
            eng.set_path(path)
            eng.upload(0, c.codes)
            if path != "dense":
                # (the named N records are run records too: all_n, one_site, last_site_only and the two halves)
                assert eng.run_records()[0] == (c.n_run if fused else 0), (L, path, kind, eng.run_records(), c.n_run)
                assert c.n_run >= (10 if kind == "runs" else 5)
            cuts = da.partition_square(n, 3)
            for m in ALL:
                what = (L, path, fused, kind, m)
                # a. tallies: the whole triangle, every pair
                tl = eng.run_square(m, tallies=True)
                check_launch(eng, c, path, fused, what)
                li = eng.last_launch()
                if li["path"] == "consensus" and fused:
                    assert li["run_records"], what
                same_tallies(tl, c.tal[FAMILY_OF[m]], what)
                # b. distances
                got = eng.run_square(m)
                check_launch(eng, c, path, fused, what)
                same_values(m, got, c.dist[m], what)
                check_host_finalisation(c, m, tl)
                # e. three row ranges give the same bytes, wherever the extremes land
                parts_t = np.concatenate([eng.run_square(m, cuts[k], cuts[k + 1], tallies=True) for k in range(3)])
                parts_d = np.concatenate([eng.run_square(m, cuts[k], cuts[k + 1]) for k in range(3)])
                assert parts_t.tobytes() == tl.tobytes() and parts_d.tobytes() == got.tobytes(), what
            # a. the rectangle in both slot orders: the set against its named records
            eng.upload(1, c.small)
            for m in ALL:
                what = (L, path, fused, kind, m, "rect")
                f = FAMILY_OF[m]
                same_tallies(eng.run_rect(m, 0, 1, tallies=True), c.rect_tal[f], what)
                if path in ("dense", "consensus"):
                    check_launch(eng, c, path, fused, what)
                same_values(m, eng.run_rect(m, 0, 1), c.rect_dist[m], what)
                same_tallies(eng.run_rect(m, 1, 0, tallies=True), c.rect_tal_t[f], what)
                if path in ("dense", "consensus"):
                    check_launch(eng, c, path, fused, what)
                same_values(m, eng.run_rect(m, 1, 0), c.rect_dist_t[m], what)
            # ... and the square job still answers the same afterwards
            same_tallies(eng.run_square("tn93", tallies=True), c.tal["tn93"], (L, path, fused, kind, "after rect"))


@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("L", tb.WIDTHS)
def test_the_16_bit_output_form_ends_at_65535_sites(L, path):
    """c. DST_OUT_TALLY16 into host and into device memory, and dst_finalize_device of it: the 32-bit tallies and the
    direct run's bits up to 65,535 sites (0xFFFF entries included); refused with the argument error from 65,536 on"""
    import torch
    c = case(L, "hot" if path == "hybrid" else "plain")
    n = c.n
    pairs = n * (n - 1) // 2
    dev = torch.device("cuda", 0)
    with da.Engine(0) as eng:
        eng.set_path(path)
        eng.upload(0, c.codes)
        for m in ALL:
            w = da.tally_width(m)
            want = c.tal[FAMILY_OF[m]]
            d_t = torch.zeros(pairs * w, dtype=torch.int16, device=dev)
            if L > 65535:
                with pytest.raises(da.DistanceError) as e:
                    eng.run_square(m, tallies16=True)
                assert e.value.status == ERR_ARG, (L, path, m)
                with pytest.raises(da.DistanceError) as e:
                    eng.run_square_device(m, 0, n, d_t.data_ptr(), pairs * w * 2, out_kind=da.OUT_TALLY16)
                assert e.value.status == ERR_ARG, (L, path, m)
                same_tallies(eng.run_square(m, tallies=True), want, (L, path, m, "after the refusal"))   # still usable
                assert eng.last_path() == path
                continue
            t16 = eng.run_square(m, tallies16=True)
            assert eng.last_path() == path and eng.last_launch()["out_kind"] == da.OUT_TALLY16
            assert t16.dtype == np.uint16 and np.array_equal(t16.astype(np.uint64), want), (L, path, m)
            assert (t16 == L).any() and (L != 65535 or (t16 == 0xFFFF).sum() == (want == 0xFFFF).sum() > 0), (L, path, m)
            direct = eng.run_square(m)
            eng.run_square_device(m, 0, n, d_t.data_ptr(), pairs * w * 2, out_kind=da.OUT_TALLY16)
            torch.cuda.synchronize()
            assert np.array_equal(d_t.cpu().numpy().view(np.uint16).reshape(pairs, w), t16), (L, path, m)
            for rb, re in ((0, n), (37, 151)):
                lo, hi = da.square_row_start(n, rb), da.square_row_start(n, re)
                d_in = torch.from_numpy(t16[lo:hi].view(np.int16).copy()).to(dev)
                d_o = torch.empty(hi - lo, dtype=torch.float64, device=dev)
                eng.finalize_device(m, rb, re, d_in.data_ptr(), d_o.data_ptr(), d_o.numel() * 8, tally_kind=da.OUT_TALLY16)
                torch.cuda.synchronize()
                out = d_o.cpu().numpy()
                if m in da.INT_MEASURES:
                    out = out.view(np.int64)
                assert np.array_equal(out, direct[lo:hi], equal_nan=True), (L, path, m, rb)


def text_cells(text, n):
    vals = [line.rsplit(b"\t", 1)[1] for line in text.split(b"\n")[:-1]]
    iu = np.triu_indices(n, 1)
    assert len(vals) == len(iu[0])
    cells = np.empty((n, n), dtype=object)
    for i, j, v in zip(iu[0], iu[1], vals):
        cells[i, j] = v
        cells[j, i] = v
    return cells


def same_bits(got, want):
    """f64 / int64 payloads: the same bits, any NaN for a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float64:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.mark.parametrize("path", ["dense", "consensus"])
@pytest.mark.parametrize("L", [65535, 65536])
def test_every_reader_of_the_tallies(L, path):
    """d. the text kernels (which read 16-bit tallies up to 65,535 sites), nearest, clusters, nj and the stream pipeline
    on the last narrow and the first wide width"""
    c = case(L, "plain")
    n, codes = c.n, c.codes
    ids = ["b%d" % k for k in range(n)]
    with da.Engine(0) as eng:
        eng.set_path(path)
        eng.upload(0, codes)
        eng.set_ids(0, ids)
        # the long text and the matrix against the oracle's text of the oracle's values
        for m in ("n_high", "raw", "jc69", "k80", "tn93"):
            want = oracle.tsv_square(m, c.dist[m], ids, threads=THREADS)
            got = eng.text_square(m, 0, n, capacity=len(want) + (1 << 16))
            assert eng.last_path() == path
            assert got == want, (L, path, m, "text_square")
            cells = text_cells(want, n)
            for i in range(n):
                cells[i, i] = diag_text(m, codes[i])
            assert eng.text_matrix(m, capacity=n * n * 24 + (1 << 16)) == matrix_text(cells, ids), (L, path, m, "text_matrix")
            assert eng.last_path() == path
        # nearest: ascending by (key of the value, index), ties by index; raw's values are the oracle's bits, tn93's the
        # engine's own (within 1e-12 of the oracle above); the tallies the oracle's
        for m in ("raw", "tn93"):
            vals = c.dist[m] if m == "raw" else eng.run_square(m)
            idx, got, gt = eng.nearest(m, 8, tallies=True)
            assert eng.last_path() == path
            assert np.array_equal(idx, expected_square(vals, n, 8)), (L, path, m)
            at = canon(n, np.repeat(np.arange(n), 8).reshape(n, 8), idx)
            assert same_bits(got, vals[at]), (L, path, m)
            same_tallies(gt, c.tal[m][at], (L, path, m, "nearest"))
        # clusters: the threshold separates the saturated pairs (n_high = L) from the rest
        nh = c.dist["n_high"].astype(np.int64)
        assert (nh == L).any() and (nh == L).sum() < len(nh) and nh.max() == L
        for t in (L - 1, L):
            want_labels, want_links = cluster_reference("n_high", nh, n, float(t))
            labels, links = eng.clusters("n_high", float(t))
            assert np.array_equal(labels, want_labels) and links == want_links == int((nh <= t).sum()), (L, path, t)
        # nj: every n_high is finite, the whole set
        parent, length = eng.nj("n_high")
        want_parent, want_length = R.nj(R.square(n, nh))
        assert np.array_equal(parent, want_parent), (L, path)
        assert np.array_equal(length.view(np.uint64), want_length.view(np.uint64)), (L, path)
        # the stream: the named records as the batch against the loaded set, bytes and nibbles, tallies and distances
        for m in ("n_high", "raw", "tn93"):
            for nibbles in (False, True):
                with eng.stream(m, max_records=len(c.small), depth=2, tallies=True, nibbles=nibbles) as st:
                    st.push(c.small)
                    tl = st.pop()
                same_tallies(tl, c.rect_tal[m].transpose(1, 0, 2), (L, path, m, nibbles, "stream tallies"))
                with eng.stream(m, max_records=len(c.small), depth=2, nibbles=nibbles) as st:
                    st.push(c.small)
                    d = st.pop()
                same_values(m, d, np.ascontiguousarray(c.rect_dist[m].T), (L, path, m, nibbles, "stream"))
