"""GPU (-m gpu): dst_text_matrix / Engine.text_matrix, the distance matrix formatted on the device.

The expected text is built from the long-format text of the same set (text_square / text_rect, byte-identical to the
reference elsewhere): cell (i, j) of the square is the canonical pair (min, max)'s value, the diagonal the measure of a
record against itself (oracle.pair_distance, formatted by da.format_distance).  Every measure on every path, symmetry,
row ranges, tiny sets, NaN / inf, 32-bit tallies, forced near ties, the rectangle, every error, the run-record state a
rectangle leaves behind, and rows of the full 50,000 x 30,000 size."""
import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import KNOWN, random_alignment
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
SEP = {"tsv": b"\t", "phylip": b" "}
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6   # include/distance_hip.h


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


def ids_of(n, prefix="r"):
    return ["%s%d" % (prefix, k) for k in range(n)]


def diag_text(m, a):
    v = oracle.pair_distance("n_high" if m == "n" else m, a, a)
    return da.format_distance(m, v).encode()


def square_cells(eng, m, codes):
    """n x n cells (bytes) from the long text of the square and the oracle's diagonal"""
    n = len(codes)
    cells = np.empty((n, n), dtype=object)
    if n > 1:
        txt = eng.text_square(m, 0, n, capacity=max(1 << 20, n * n * 64))
        vals = [line.rsplit(b"\t", 1)[1] for line in txt.split(b"\n")[:-1]]
        iu = np.triu_indices(n, 1)
        assert len(vals) == len(iu[0])
        for i, j, v in zip(iu[0], iu[1], vals):
            cells[i, j] = v
            cells[j, i] = v
    for i in range(n):
        cells[i, i] = diag_text(m, codes[i])
    return cells


def matrix_text(cells, ids, style="tsv", rows=None):
    sep = SEP[style]
    rows = range(cells.shape[0]) if rows is None else rows
    return b"".join(ids[i].encode() + b"".join(sep + c for c in cells[i]) + b"\n" for i in rows)


def parse(text, style="tsv"):
    return [line.split(SEP[style]) for line in text.split(b"\n")[:-1]]


def test_square_every_measure_dense_and_consensus(eng):
    n, L = 240, 1_600
    codes = random_alignment(n, L, seed=11)
    codes[3, :] = 240                          # no resolved site: NaN for raw, also on the diagonal
    codes[4, :] = 136                          # A everywhere ...
    codes[5, :] = 136
    codes[5, : 3 * L // 4] = 40                # ... against 3/4 of the sites C: jc69 saturates (inf)
    ids = ids_of(n)
    for path in ("dense", "consensus"):
        eng.set_path("auto")
        eng.upload(0, codes)
        eng.set_ids(0, ids)
        eng.set_path(path)
        for m in ALL:
            cells = square_cells(eng, m, codes)
            got = eng.text_matrix(m)
            assert eng.last_path() == path, (path, m)
            assert got == matrix_text(cells, ids), (path, m)
            # symmetric byte for byte
            f = [row[1:] for row in parse(got)]
            assert all(f[i][j] == f[j][i] for i in range(n) for j in range(i)), (path, m)
            assert eng.text_matrix(m, style="phylip") == matrix_text(cells, ids, "phylip"), (path, m)
        raw = parse(eng.text_matrix("raw"))
        assert raw[3][1 + 3] == b"NaN" and raw[3][1 + 7] == b"NaN" and raw[0][1 + 0] == b"0.000000000000"
        assert parse(eng.text_matrix("jc69"))[4][1 + 5] == b"inf"
    eng.set_path("auto")


@pytest.mark.parametrize("kind", ["clade", "runs"])
def test_hybrid_and_run_records(eng, kind):
    n, L = 600, 4_000
    codes = synth.alignment(synth.SEED ^ 3, n, L)
    if kind == "clade":
        r = synth.root(synth.SEED, L)
        codes = synth.records(synth.SEED, r, 0, n)
        synth.apply_clades(codes, r, *synth.clade_plan(synth.SEED, n, L))
        path = "hybrid"
    else:
        synth.apply_nruns(codes, synth.nrun_plan(17, n, L, 0.2, 0.4))
        path = "consensus"
    ids = ids_of(n, "h")
    with da.Engine(0) as ref:   # the expected cells from the dense path
        ref.set_path("dense")
        ref.upload(0, codes)
        ref.set_ids(0, ids)
        want = {m: matrix_text(square_cells(ref, m, codes), ids) for m in ("n", "raw", "tn93")}
    eng.set_prep_threshold(0)
    try:
        eng.set_path("auto")
        eng.upload(0, codes)
        eng.set_ids(0, ids)
        eng.set_path(path)
        if kind == "runs":
            assert eng.run_records()[0] > 0
        for m, w in want.items():
            assert eng.text_matrix(m) == w, (kind, m)
            assert eng.last_path() == path
    finally:
        eng.set_prep_threshold(2e10)
        eng.set_path("auto")


def test_row_ranges_concatenate(eng):
    n, L = 700, 900
    codes = random_alignment(n, L, seed=5)
    ids = ids_of(n, "seq_")
    eng.set_path("auto")
    eng.upload(0, codes)
    eng.set_ids(0, ids)
    for m in ("raw", "k80"):
        whole = eng.text_matrix(m)
        assert whole == matrix_text(square_cells(eng, m, codes), ids)
        for cuts in ([0, 1, 2, 255, 256, 257, 511, 699, 700], [0, 350, 700], [0, 699, 700]):
            parts = [eng.text_matrix(m, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
            assert b"".join(parts) == whole, (m, cuts)
        assert eng.text_matrix(m, 10, 10) == b""


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_sets(eng, n):
    codes = random_alignment(n, 300, seed=n)
    if n == 2:
        codes[1, :] = 240
    ids = ids_of(n)
    eng.upload(0, codes)
    eng.set_ids(0, ids)
    for m in ALL:
        assert eng.text_matrix(m) == matrix_text(square_cells(eng, m, codes), ids), m
    if n == 2:
        assert parse(eng.text_matrix("raw"))[1] == [b"r1", b"NaN", b"NaN"]


def test_wide_alignment_32_bit_tallies(eng):
    n, L = 70, 70_000
    codes = random_alignment(n, L, seed=9)
    ids = ids_of(n, "w")
    eng.upload(0, codes)
    eng.set_ids(0, ids)
    for m in ("jc69", "k80", "tn93"):
        assert eng.text_matrix(m) == matrix_text(square_cells(eng, m, codes), ids), m


def test_forced_near_ties_of_jc69(eng):
    """pairs (0, k) whose host value lies within a few ulp of a rounding boundary of the 12th decimal (as in
    test_gpu_text_identity): every one is noted, in both triangles, and printed as the host prints it"""
    cand = []
    for d in range(2_000, 3_000):
        nn = np.arange(1, int(0.7 * d))
        v = -0.75 * np.log(1.0 - (4.0 / 3.0) * (nn / float(d)))
        scaled = v * 1e12
        frac = np.abs(scaled - np.floor(scaled) - 0.5)
        for k in np.nonzero(frac < scaled * 2.0 ** -49)[0]:
            cand.append((int(nn[k]), d))
    assert len(cand) >= 20
    cand = cand[:400]
    L = 3_000
    rng = np.random.default_rng(1)
    root = rng.choice(np.array(KNOWN, np.uint8), size=L)
    codes = np.tile(root, (len(cand) + 1, 1))
    for k, (nn, d) in enumerate(cand, start=1):
        codes[k, :nn] = np.where(root[:nn] == 136, 72, 136)
        codes[k, d:] = 240
    ids = ids_of(len(codes), "t")
    eng.set_path("auto")
    eng.upload(0, codes)
    eng.set_ids(0, ids)
    tl = eng.run_square("jc69", 0, 1, tallies=True)
    host = oracle.finalize_square("jc69", tl, len(codes), None, 0, 1)
    row0 = [oracle.format_distance(float(v)).encode() for v in host]
    near0, _ = eng.text_stats()
    top = min(60, len(codes))
    got = parse(eng.text_matrix("jc69", 0, top))
    near1, _ = eng.text_stats()
    assert got[0][2:] == row0[:len(got[0]) - 2]
    assert [got[k][1] for k in range(1, top)] == row0[:top - 1]
    assert near1 - near0 >= 2 * (top - 1)
    full = eng.text_matrix("jc69")
    assert full == matrix_text(square_cells(eng, "jc69", codes), ids)


def test_rectangle_against_text_rect(eng):
    n0, n1, L = 130, 410, 2_000
    a = random_alignment(n0, L, seed=21)
    b = random_alignment(n1, L, seed=22)
    ia, ib = ids_of(n0, "a"), ids_of(n1, "b")
    eng.upload(0, a)
    eng.upload(1, b)
    eng.set_ids(0, ia)
    eng.set_ids(1, ib)
    for m in ALL:
        long = eng.text_rect(m, 0, 1, 0, n0)
        vals = [line.rsplit(b"\t", 1)[1] for line in long.split(b"\n")[:-1]]
        cells = np.array(vals, dtype=object).reshape(n0, n1)
        assert eng.text_matrix(m, square=False, row_slot=0, col_slot=1) == matrix_text(cells, ia), m
        long_t = eng.text_rect(m, 1, 0, 0, n1)
        vals_t = [line.rsplit(b"\t", 1)[1] for line in long_t.split(b"\n")[:-1]]
        cells_t = np.array(vals_t, dtype=object).reshape(n1, n0)
        assert eng.text_matrix(m, 5, 17, square=False, row_slot=1, col_slot=0) == matrix_text(cells_t, ib, rows=range(5, 17))


def test_errors():
    codes = random_alignment(20, 200, seed=1)
    with da.Engine(0) as e:
        with pytest.raises(da.DistanceError):                 # no set
            e.text_matrix("raw", 0, 1)
        e.upload(0, codes)
        with pytest.raises(da.DistanceError):                 # no ids
            e.text_matrix("raw")
        e.set_ids(0, ids_of(20))
        assert e.text_matrix("raw", capacity=1 << 16)
        lib = da.load()
        import ctypes as C
        buf = C.create_string_buffer(1 << 16)
        n = C.c_size_t(0)

        def call(m=2, sq=1, rs=0, cs=1, rb=0, re=20, st=0, cap=1 << 16):
            return lib.dst_text_matrix(e._h, m, sq, rs, cs, rb, re, st, C.addressof(buf), cap, C.byref(n))

        ok = call()
        assert ok == 0 and n.value > 0
        assert call(cap=10) == ERR_CAPACITY
        assert call(m=9) == ERR_ARG
        assert call(st=2) == ERR_ARG
        assert call(rb=5, re=4) == ERR_ARG
        assert call(re=21) == ERR_ARG
        assert call(sq=0, rs=0, cs=0) == ERR_ARG
        assert call(sq=0, rs=2, cs=0) == ERR_ARG
        assert call(sq=0, rs=0, cs=1) == ERR_STATE            # slot 1 not uploaded
        e.upload(1, random_alignment(7, 200, seed=2))
        assert call(sq=0, rs=1, cs=0, re=7) == ERR_STATE      # slot 1's ids not given
        e.set_ids(1, ids_of(7, "x"))
        assert call(sq=0, rs=1, cs=0, re=7) == 0
        assert call(rb=0, re=70_000) == ERR_ARG


def test_rectangle_leaves_run_records_usable(eng):
    """a stripped run-record set as the ROW set of a rectangle, then a square run on it: the dense kernels' bits"""
    n, L = 2_500, 6_000
    codes = synth.alignment(synth.SEED ^ 41, n, L)
    synth.apply_nruns(codes, synth.nrun_plan(41, n, L, 0.2, 0.4))
    other = synth.alignment(synth.SEED ^ 42, 50, L)
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, codes)
        want = {m: ref.run_square(m) for m in ("raw", "tn93")}
    eng.set_prep_threshold(0)
    try:
        eng.set_path("auto")
        eng.upload(0, codes)
        eng.upload(1, other)
        eng.set_ids(0, ids_of(n))
        eng.set_ids(1, ids_of(50, "o"))
        eng.set_path("consensus")
        assert eng.run_records()[0] > 0
        assert eng.text_matrix("raw", square=False, row_slot=0, col_slot=1)
        assert eng.last_path() == "consensus"
        for m, w in want.items():
            assert np.array_equal(eng.run_square(m), w, equal_nan=True), m
    finally:
        eng.set_prep_threshold(2e10)
        eng.set_path("auto")


def test_full_size_rows():
    n, L = 50_000, 30_000
    codes = synth.alignment(synth.SEED ^ 7, n, L)
    ids = ids_of(n, "s")
    with da.Engine(0) as e:
        e.upload(0, codes)
        e.set_ids(0, ids)
        # the long text of the pairs of a few rows: row r against every column is (j, r) for j < r and (r, j) above
        for rb, re in ((0, 1), (24_999, 25_000), (49_999, 50_000), (31_000, 31_300)):
            got = parse(e.text_matrix("raw", rb, re, capacity=(re - rb) * n * 20 + (1 << 20)))
            assert len(got) == re - rb
            e.upload(1, np.ascontiguousarray(codes[rb:re]))
            e.set_ids(1, ids[rb:re])
            long = e.text_rect("raw", 1, 0, 0, re - rb, capacity=(re - rb) * n * 40 + (1 << 20))
            vals = [line.rsplit(b"\t", 1)[1] for line in long.split(b"\n")[:-1]]
            for k in range(re - rb):
                row = vals[k * n:(k + 1) * n]
                assert got[k][0] == ids[rb + k].encode()
                assert got[k][1:] == row, (rb + k)
                assert got[k][1 + rb + k] == b"0.000000000000"
