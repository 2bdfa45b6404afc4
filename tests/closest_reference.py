"""What a closest stream must answer, from a plain stream's own results (tests/test_gpu_closest.py, test_gpu_cli_closest.py).

The truth is the matrix S[streamed][loaded] of the plain dst_stream (DST_OUT_DISTANCE payloads and DST_OUT_TALLY words of
the same batches); record i of the loaded set keeps the k smallest (key, ordinal) of column i.  keys / smallest restate the
documented order of dst_nearest (tests/test_gpu_nearest.py)."""
import numpy as np


def keys(vals: np.ndarray) -> np.ndarray:
    """The documented sort key of DST_OUT_DISTANCE payloads: int64 v ^ 2^63; f64 the order-preserving flip, NaN ~0 (after
    +inf), -0.0 the key of +0.0."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def smallest(key_row: np.ndarray, k: int) -> np.ndarray:
    """Positions of the k smallest (key, position) of one row, in that order."""
    idx = np.arange(len(key_row))
    k = min(k, len(idx))
    if k == 0:
        return idx[:0]
    kth = np.partition(key_row, k - 1)[k - 1]
    cand = np.nonzero(key_row <= kth)[0]
    return cand[np.lexsort((cand, key_row[cand]))][:k]


def cuts_of(n: int, size: int) -> list[int]:
    """n records in batches of `size` (the last one short)"""
    return [min(size, n - b) for b in range(0, n, size)]


def plain_truth(eng, measure, streamed, counts=None, max_records=200, nibbles=False):
    """(S values [streamed][loaded], S tallies [streamed][loaded][W]) from the plain stream, in batches of max_records"""
    out = []
    for tallies in (False, True):
        got = []
        with eng.stream(measure, max_records=max_records, depth=2, tallies=tallies, nibbles=nibbles) as st:
            for b0 in range(0, len(streamed), max_records):
                st.push(streamed[b0:b0 + max_records], None if counts is None else counts[b0:b0 + max_records])
                got.append(st.pop())
        out.append(np.concatenate(got))
    return out[0], out[1]


def expected_for_loaded(S_vals, S_tal, k, ordinals=None):
    """(index, values, tallies) [loaded][k_used]: per column the k smallest (key, ordinal); `ordinals` (ascending) names
    the rows, default 0 .. n_streamed - 1"""
    n_s, n_l = S_vals.shape
    kk = keys(S_vals)
    ku = min(k, n_s)
    pos = np.array([smallest(np.ascontiguousarray(kk[:, i]), ku) for i in range(n_l)], np.int64).reshape(n_l, ku)
    cols = np.arange(n_l)[:, None]
    index = pos.astype(np.uint32) if ordinals is None else np.asarray(ordinals, np.uint64)[pos].astype(np.uint32)
    return index, S_vals[pos, cols], S_tal[pos, cols]


def expected_for_streamed(S_vals, S_tal, k):
    """(index, values, tallies) [streamed][k_used]: per row the k smallest (key, loaded index)"""
    n_s, n_l = S_vals.shape
    kk = keys(S_vals)
    ku = min(k, n_l)
    pos = np.array([smallest(kk[r], ku) for r in range(n_s)], np.int64).reshape(n_s, ku)
    rows = np.arange(n_s)[:, None]
    return pos.astype(np.uint32), S_vals[rows, pos], S_tal[rows, pos]


def run_closest(eng, measure, k, streamed, cuts, counts=None, max_records=200, depth=3, nibbles=False, side="loaded",
                first_index=None, tallies=True):
    """Push `streamed` cut into batches of the sizes `cuts` through a closest stream, popping as the ring fills.
    side="loaded": result(tallies); side="streamed": the batches' (index, values, tallies) concatenated."""
    got = []
    with eng.closest_stream(measure, k, max_records, side=side, depth=depth, nibbles=nibbles) as st:
        if first_index is not None:
            st.next_index(first_index)
        b0 = 0
        for size in cuts:
            if st.in_flight() == depth - 1:
                got.append(st.pop())
            st.push(streamed[b0:b0 + size], None if counts is None else counts[b0:b0 + size])
            b0 += size
        assert b0 == len(streamed)
        while st.in_flight():
            got.append(st.pop())
        if side == "loaded":
            assert got == list(cuts)
            return st.result(tallies=tallies)
    return tuple(np.concatenate([g[a] for g in got]) for a in range(3))


def bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def assert_same(got, want, what=""):
    """(index, values, tallies) triples, bit for bit"""
    names = ("index", "values", "tallies")
    for g, w, name in zip(got, want, names):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name)


def special_values_set():
    """40 x 400: ten copies of a root (zeros; jc69 / k80 give -0.0), ten records that differ from it at exactly 300 sites
    (raw 0.75: jc69 +inf), five records without a resolved site (all N: raw NaN against everyone), fifteen ordinary ones"""
    rng = np.random.default_rng(91)
    L = 400
    root = rng.choice(np.array([136, 72, 40, 24], np.uint8), size=L)
    alt = np.array([{136: 72, 72: 136, 40: 24, 24: 40}[int(c)] for c in root], np.uint8)
    codes = np.tile(root, (40, 1))
    codes[10:20, :300] = alt[:300]
    codes[20:25] = 240
    m = rng.random((15, L)) < 0.05
    codes[25:][m] = rng.choice(np.array([136, 72, 40, 24], np.uint8), size=int(m.sum()))
    return codes
