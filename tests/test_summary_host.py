"""CPU: the host side of dst_summary: the declaration and the export, the ABI version, the constants in the header and in
Python, the NULL-context status, and the numpy / Python-integer restatement of the definition (summary_reference) on
hand-made values: NaN, +-inf, -0.0, the 2^25 limit, a tie of rint, bin edges, one bin, and a brute-force double loop."""
import math
import re

import numpy as np

import distance_amd as da
from distance_amd import _lib
from summary_reference import bin_index, fixed_point, hist_of, summary, width_q

ERR_ARG = 1
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -37   # one unit of the fixed-point scale


def test_declared_and_exported():
    assert "dst_summary" in da.declared_symbols()
    lib = da.load()
    assert hasattr(lib, "dst_summary")
    assert "dst_summary" in _lib._SIGS and len(_lib._SIGS["dst_summary"][1]) == 15
    assert hasattr(da.Engine, "summary")


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_constants_match_header():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DST_SUMMARY_SCALE_BITS\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SUMMARY_SCALE_BITS == da.SUMMARY_SCALE_BITS == 37
    m = re.search(r"#define\s+DST_SUMMARY_MAX_BINS\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SUMMARY_MAX_BINS == da.SUMMARY_MAX_BINS == 4096
    fields = re.search(r"typedef struct dst_summary_totals \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", fields) == [("uint64_t", "pairs"), ("uint64_t", "nan_pairs"), ("uint64_t", "summable_pairs"),
                                                      ("uint64_t", "links"), ("double", "sum")]
    assert [f[0] for f in _lib.SummaryTotals._fields_] == ["pairs", "nan_pairs", "summable_pairs", "links", "sum"]


def test_null_context_is_err_arg():
    lib = da.load()
    assert lib.dst_summary(None, 2, 1, 0, 1, 1.0, 0, 0, 1.0, None, None, None, None, 0, None) == ERR_ARG


def test_special_values():
    below = math.nextafter(2.0 ** 25, 0.0)
    v = np.array([NAN, INF, -INF, -0.0, 0.0, below, 2.0 ** 25, -below, -(2.0 ** 25), 0.25])
    ok, q = fixed_point("raw", v)
    assert list(ok) == [False, False, False, True, True, True, False, True, False, True]
    assert q[3] == 0 and q[4] == 0 and q[5] == 2 ** 62 - 2 ** 9 and q[7] == -q[5] and q[9] == 2 ** 35
    b = bin_index("raw", v, 8, 0.125)
    assert list(b) == [-1, 7, 0, 0, 0, 7, 7, 0, 0, 2]
    # a 2 x 5 rectangle of them: record 0 = the first five, record 1 the rest
    w = summary("raw", v.reshape(2, 5), 2, 5, False, 0.0, bins=8, width=0.125)
    assert w["pairs"] == 10 and w["nan_pairs"] == 1 and w["summable_pairs"] == 5
    assert list(w["summable"]) == [2, 3] and list(w["within"]) == [3, 2]   # -inf, -0.0, 0.0 | -below, -2^25
    assert w["links"] == 5 and int(w["hist"].sum()) == 9 and list(w["hist"]) == [5, 0, 1, 0, 0, 0, 0, 3]
    assert w["sum"][0] == 0.0 and w["sum"][1] == 0.25 and w["total_sum"] == 0.25   # below - below + 0.25
    # every partner NaN: summable 0, sum 0
    w = summary("jc69", np.array([NAN, NAN, 1.0]), 3, 3, True, INF)
    assert list(w["summable"]) == [0, 1, 1] and list(w["within"]) == [0, 1, 1] and list(w["sum"]) == [0.0, 1.0, 1.0]
    assert w["nan_pairs"] == 2 and w["links"] == 1


def test_rint_ties_and_rounding():
    # v * 2^37 = k + 1/2: to the even neighbour
    for k, want in ((0, 0), (1, 2), (2, 2), (3, 4), (-1, 0), (-2, -2), (-3, -2)):
        ok, q = fixed_point("raw", np.array([(k + 0.5) * U]))
        assert ok[0] and q[0] == want, (k, q)
    ok, q = fixed_point("tn93", np.array([0.3]))
    assert q[0] == round(0.3 * 2 ** 37) and abs(q[0] * U - 0.3) <= U / 2
    # the sum is exact in integers and rounded once: 2^53 + 1 units is a tie of the conversion, to even
    vals = np.array([2.0 ** 16, U])   # q = 2^53 and 1
    w = summary("raw", vals, 1, 2, False, 0.0)
    assert w["sum"][0] == math.ldexp(float(2 ** 53), -37) and w["summable"][0] == 2
    w = summary("raw", np.array([2.0 ** 16, 3 * U]), 1, 2, False, 0.0)   # 2^53 + 3: the tie goes up to 2^53 + 4
    assert w["sum"][0] == math.ldexp(float(2 ** 53 + 4), -37)
    # integers: the payload itself, sums beyond 2^53 rounded once
    big = np.array([2 ** 53, 1, 2], np.int64)
    w = summary("n", big, 1, 3, False, 5)
    assert w["sum"][0] == float(2 ** 53 + 3) == float(2 ** 53 + 4) and list(w["within"]) == [2]
    # sums past the int64 range (the Python-integer branch of the reference)
    w = summary("n", np.array([2 ** 62, 2 ** 62, 2 ** 62 + 2 ** 9], np.int64), 1, 3, False, 0)
    assert w["sum"][0] == float(3 * 2 ** 62 + 2 ** 9) == w["total_sum"] and w["summable"][0] == 3


def test_bin_edges():
    W = 0.01
    wq = width_q("raw", W)
    assert wq == int(np.rint(W * 2.0 ** 37)) and width_q("n", 3.0) == 3
    for k in (0, 1, 7, 49, 63, 64, 1000):
        at, under = k * wq * U, (k * wq - 1) * U   # exactly k width_q, and one unit below
        b = bin_index("raw", np.array([at, under]), 64, W)
        assert b[0] == min(k, 63) and b[1] == min(max(k - 1, 0), 63), (k, b)
    assert list(bin_index("raw", np.array([-U, -0.5, -0.0]), 64, W)) == [0, 0, 0]
    b = bin_index("n", np.array([0, 2, 3, 5, 6, 1000], np.int64), 3, 3.0)
    assert list(b) == [0, 0, 1, 1, 2, 2]
    assert list(bin_index("n_high", np.array([0, 1, 4094, 4095, 4096, 10 ** 9], np.int64), 4096, 1.0)) == [0, 1, 4094, 4095, 4095, 4095]
    # one bin: everything that is not NaN
    v = np.array([NAN, -1.0, 0.0, 5.0, INF, 1e7, 2.0 ** 30])
    assert list(hist_of("raw", v, 1, 0.5)) == [6] and list(bin_index("raw", v, 1, 0.5)) == [-1, 0, 0, 0, 0, 0, 0]


def test_square_against_a_double_loop():
    rng = np.random.default_rng(11)
    n = 23
    vals = rng.integers(0, 9, n * (n - 1) // 2).astype(np.float64) / 8
    vals[rng.integers(0, len(vals), 20)] = NAN
    vals[rng.integers(0, len(vals), 5)] = INF
    T = 0.5
    w = summary("k80", vals, n, n, True, T, bins=4, width=0.25)
    within, summable, sums, hist, k = [0] * n, [0] * n, [0.0] * n, [0] * 4, 0
    for i in range(n):
        for j in range(i + 1, n):
            v = vals[k]
            k += 1
            if v <= T:
                within[i] += 1
                within[j] += 1
            if v == v and abs(v) < 2.0 ** 25:
                summable[i] += 1
                summable[j] += 1
                sums[i] += v   # (eighths: exact in f64)
                sums[j] += v
            if v == v:
                hist[3 if v == INF else min(int(v // 0.25), 3)] += 1
    assert list(w["within"]) == within and list(w["summable"]) == summable and list(w["sum"]) == sums
    assert list(w["hist"]) == hist and w["links"] * 2 == sum(within) and w["summable_pairs"] * 2 == sum(summable)
    assert w["total_sum"] * 2 == sum(sums) and w["pairs"] == len(vals) and w["nan_pairs"] == int(np.isnan(vals).sum())
