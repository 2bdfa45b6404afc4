"""GPU (-m gpu): the device's f64 finalisation of jc69 / k80 / tn93 against the exact value (finalise_reference.py) and
against the host's bits, on tallies chosen to sit at every branch of dst_device.hpp's fin_*_fast / fin_*_close.

(a) the pair kernels' epilogue (DST_OUT_DISTANCE, dst_finalize_device without DST_FIN_CLOSE): nine-term series of
    -ln(1 - e) for every e_i below 2^-5, reciprocals from the f32 unit and one Newton step; everything else through
    the close arithmetic.  Bar |got - x| <= B_m S with S = sum_i |k_i ln(1 - e_i)| the scale of the terms.
(b) the text path's arithmetic (DST_FIN_CLOSE: the reference's operation order, the table logarithm dst_log) against
    the oracle's glibc finalisation, in ulp.
(c) the 16-bit tally format against the 32-bit one.
(d) the real pair kernels (dense, consensus, auto) on an alignment whose pairs straddle each measure's series switch.

Each test prints its measured maxima as one JSON line (pytest -s shows them).
"""
import json
import os

import numpy as np
import pytest

import distance_amd as da
import finalise_reference as fr
import oracle
from helpers import KNOWN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
THREADS = min(16, len(os.sched_getaffinity(0)))
LD = np.longdouble

# (a): 4x the largest |got - x| / S measured on an MI355X over these cases' series path, rounded up to a power of two:
# jc69 1.41e-14 (1.05e-14 with d below 2^24: above it the f32 seed also carries the rounding of d), k80 1.11e-14,
# tn93 3.39e-14.  The series leaves e^10 / 10 of e (3e-15 of a term at e = 2^-5); v_rcp_f32 is specified to 1 ulp, which
# the Newton step squares to 2^-46; tn93 forms each e_i from a few more products.  (Caps, not to be raised: 2^-44 for
# jc69 / k80, 2^-42 for tn93.)
BAR = {"jc69": 2.0 ** -44, "k80": 2.0 ** -44, "tn93": 2.0 ** -42}
# (b): the text path sends every value within 2^-47 |v| of a rounding boundary of the 12th decimal to the host's libm
# (dst_text.hip, kGuardShift): 2^-47 |v| is at least 32 ulp of v.  8 ulp (2^-49 |v|) leaves a factor of four to the
# guard; jc69 computes the same f64 argument as the host and differs only in the logarithm (dst_log: <= 1 ulp of glibc)
# and the rounding of -0.75 times it: 2 ulp.
CLOSE_ULP = {"jc69": 2, "k80": 8, "tn93": 8}
SWITCH_SLACK = LD(1e-9)   # e_i this close to 2^-5 (relative): the device's rounded e_i may fall on either side


def report(key, rec):
    print(json.dumps({key: rec}, sort_keys=True))


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


def _finalize(eng, measure, tl, n, close=False, kind=da.OUT_TALLY):
    dev = torch.device("cuda", 0)
    d_t = torch.from_numpy(np.ascontiguousarray(tl, np.uint16 if kind == da.OUT_TALLY16 else np.uint32)).to(dev)
    d_o = torch.empty(len(tl), dtype=torch.float64, device=dev)
    eng.finalize_device(measure, 0, n, d_t.data_ptr(), d_o.data_ptr(), d_o.numel() * 8, tally_kind=kind, close=close)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


_CACHE = {}


def adversarial(eng, measure):
    """the adversarial cases of `measure` on the canonical pairs of an uploaded set: tallies, base counts (tn93), the
    exact values, the host's, and the device's in both arithmetics"""
    if measure in _CACHE:
        return _CACHE[measure]
    tl, counts = fr.cases(measure)
    if counts is None:
        n = fr.records_for(len(tl))
        tl = np.resize(tl, (n * (n - 1) // 2, tl.shape[1]))       # the last pairs repeat the first cases
        q = t = None
    else:
        n = len(counts)
        q, t = fr.pair_counts(counts)
    c = dict(tl=tl, n=n, counts=counts, q=q, t=t, ex=fr.exact(measure, tl, q, t),
             host=oracle.finalize_square(measure, tl, n, counts, threads=THREADS))
    upload(eng, c)
    c["fast"], c["close"] = _finalize(eng, measure, tl, n), _finalize(eng, measure, tl, n, close=True)
    _CACHE[measure] = c
    return c


def upload(eng, c):
    """n records of 16 sites; for tn93 with the cases' base counts"""
    codes = np.random.default_rng(3).choice(np.array(KNOWN, np.uint8), size=(c["n"], 16))
    if c["counts"] is None:
        eng.upload(0, codes)
    else:
        eng.upload(0, codes, base_counts=c["counts"].astype(np.uint32))
        assert np.array_equal(eng.base_counts(0), c["counts"].astype(np.uint32))


def takes_the_series(measure, c):
    """the branch fin_*_fast takes, from the exact tallies: True (the series), False (fin_*_close), None (an e_i within
    SWITCH_SLACK of 2^-5: either)"""
    ex, tl = c["ex"], c["tl"].astype(np.int64)
    sm = LD(fr.SERIES_MAX)
    with np.errstate(invalid="ignore"):
        past = (ex.e >= sm).any(axis=1) | np.isnan(ex.e).any(axis=1)
        unsure = (np.abs(ex.e / sm - 1) < SWITCH_SLACK).any(axis=1)
    if measure == "jc69":
        long_way = tl[:, 1] == 0
    elif measure == "k80":
        long_way = tl[:, 0] == 0
    else:   # counts of 2^24 and more, a zero frequency sum or count_L = 0
        s = c["q"].astype(np.int64) + c["t"].astype(np.int64)
        big = (np.maximum(c["q"], c["t"]) >= fr.B24).any(axis=1) | (tl[:, 0] >= fr.B24)
        long_way = big | (s.min(axis=1) == 0) | (tl[:, 0] == 0)
    series = ~(long_way | past)
    return np.where(unsure & ~long_way, None, series)


def check_special(got, host, x, what):
    """where the exact value is NaN, +-inf or zero: the host's value exactly (NaN, inf, the sign of zero)"""
    special = ~np.isfinite(x) | (x == 0)
    assert np.array_equal(np.isnan(got[special]), np.isnan(host[special])), what
    h, g = host[special & ~np.isnan(host)], got[special & ~np.isnan(host)]
    assert np.array_equal(g.view(np.uint64), h.view(np.uint64)), what
    return special


def series_error(got, ex):
    """|got - x| / S"""
    with np.errstate(all="ignore"):
        return (np.abs(got.astype(LD) - ex.value) / ex.scale).astype(np.float64)


@pytest.mark.parametrize("measure", fr.MEASURES)
def test_series_epilogue_against_the_exact_value(eng, measure):
    c = adversarial(eng, measure)
    ex, got, x = c["ex"], c["fast"], c["ex"].value.astype(np.float64)
    special = check_special(got, c["host"], x, measure)
    branch = takes_the_series(measure, c)
    series = ~special & (branch == True)                                      # noqa: E712
    long_way = ~special & (branch == False)                                   # noqa: E712
    # the pairs past the series (or with tallies it does not take) are the close arithmetic's, bit for bit: (b) holds
    # that to the host's libm.  Its error against x is the reference formula's own — 1 - e rounds away the low bits of
    # a small e, 2^-53 / e of the value — and is only reported.
    assert np.array_equal(got[long_way].view(np.uint64), c["close"][long_way].view(np.uint64)), measure
    r = series_error(got[series], _take(ex, series))
    small = (c["tl"][series] < fr.B24).all(axis=1)
    worst = int(np.argmax(r))
    with np.errstate(invalid="ignore"):
        well = long_way & (ex.min_log_arg >= LD(1) / 16)
    rec = {"cases": int(len(x)), "series_cases": int(series.sum()), "close_cases": int(long_way.sum()),
           "max_err_over_S": float(r.max()), "worst_tallies": c["tl"][series][worst].tolist(),
           "max_err_over_S_tallies_below_2^24": float(r[small].max()),
           "close_cases_max_err_over_S_log_args_from_1/16": float(series_error(got[well], _take(ex, well)).max()),
           "bar": BAR[measure]}
    report("a_" + measure, rec)
    assert series.sum() > 10000 and long_way.sum() > 5000, rec
    assert r.max() <= BAR[measure], (measure, rec)


def _take(ex, mask):
    return fr.Exact(ex.value[mask], ex.scale[mask], ex.e[mask], ex.k[mask])


@pytest.mark.parametrize("measure", fr.MEASURES)
def test_close_arithmetic_against_the_host_bits(eng, measure):
    """every finite value within CLOSE_ULP of glibc's; NaN / inf / zero exactly.  (tn93: k1, k2 >= 0 and
    k3 >= g_R g_Y > 0 with every e_i >= 0, so no two terms of a finite value cancel and the ulp bar needs no scale.)"""
    c = adversarial(eng, measure)
    got, host = c["close"], c["host"]
    assert np.array_equal(np.isnan(got), np.isnan(host)), measure
    inf = np.isinf(host)
    assert np.array_equal(got[inf], host[inf]), measure
    zero = host == 0
    assert np.array_equal(got[zero].view(np.uint64), host[zero].view(np.uint64)), measure
    fin = np.isfinite(host) & ~zero
    assert np.array_equal(np.signbit(got[fin]), np.signbit(host[fin])), measure
    ulp = np.abs(got[fin].view(np.int64) - host[fin].view(np.int64))
    rec = {"finite": int(fin.sum()), "max_ulp": int(ulp.max()), "bits_differ": int((ulp > 0).sum()),
           "bar_ulp": CLOSE_ULP[measure]}
    if measure == "jc69":
        with np.errstate(all="ignore"):
            w = 1.0 - (4.0 / 3.0) * (c["tl"][:, 0].astype(np.float64) / c["tl"][:, 1].astype(np.float64))
        cells = ((w[fin].view(np.uint64) - np.uint64(0x3FE6000000000000)) >> np.uint64(45)) & np.uint64(127)
        binades = np.frexp(w[fin])[1]
        assert len(np.unique(cells)) == 128 and set(range(-32, 1)) <= set(binades.tolist())
        rec["cells"], rec["binades"] = int(len(np.unique(cells))), int(len(np.unique(binades)))
    report("b_" + measure, rec)
    assert ulp.max() <= CLOSE_ULP[measure], (measure, rec, c["tl"][fin][np.argmax(ulp)].tolist())


@pytest.mark.parametrize("measure", fr.MEASURES)
def test_tally16_gives_the_tally32_bits(eng, measure):
    c = adversarial(eng, measure)
    upload(eng, c)
    small = np.where((c["tl"] < 65536).all(axis=1)[:, None], c["tl"], 0)
    assert (small.any(axis=1)).sum() > 1000
    for close in (False, True):
        a = _finalize(eng, measure, small, c["n"], close=close)
        b = _finalize(eng, measure, small, c["n"], close=close, kind=da.OUT_TALLY16)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (measure, close)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the real kernels at the switch
L_SITES = 4096
GROUP = [14, 15, 16, 16, 17, 18, 30, 31, 32, 32, 33, 34, 46, 47, 48, 48, 49, 50, 62, 63, 64, 64, 65, 66]
A, G, C, T = 136, 72, 40, 24
TRANSVERSION = {A: C, C: A, G: T, T: G}


def switch_alignment():
    """a root of balanced composition and three groups of records, each record with private differences at sites of
    its own (so a pair's tallies are sums of two records' counts): A<->G transitions, C<->T transitions, and
    transversions (every site one fixed alternative: pairs of that group have ts = 0).  The per-record counts GROUP
    put pair sums around every switch at L = 4096: jc69 n = 96, k80 2 ts or 2 tv = 128 (and tv = 128, where ea
    reaches 2^-5), tn93 P1 or P2 = 32 (e1, e2) and Q = 64 (e3)."""
    rng = np.random.default_rng(5)
    root = rng.permutation(np.repeat(np.array([A, G, C, T], np.uint8), L_SITES // 4))
    codes = np.tile(root, (3 * len(GROUP), 1))
    free = {b: list(np.nonzero(root == b)[0]) for b in (A, G, C, T)}
    r = 0
    for kind in ("AG", "CT", "tv"):
        for cnt in GROUP:
            for _ in range(cnt):
                b = {"AG": (A, G), "CT": (C, T), "tv": (A, G, C, T)}[kind][rng.integers(0, 2 if kind != "tv" else 4)]
                s = free[b].pop()
                codes[r, s] = {A: G, G: A, C: T, T: C}[b] if kind != "tv" else TRANSVERSION[b]
            r += 1
    return np.ascontiguousarray(codes)


@pytest.mark.parametrize("path", ["dense", "consensus", "auto"])
def test_real_kernels_at_the_series_switch(eng, path):
    """DST_OUT_DISTANCE of the pair kernels is finalize_device of the same run's tallies bit for bit, and within (a)'s
    bars of the exact value, on pairs straddling each measure's switch"""
    codes = switch_alignment()
    n = len(codes)
    counts = oracle.count_bases_matrix(codes)
    q, t = fr.pair_counts(counts)
    eng.set_path(path)
    try:
        eng.upload(0, codes)
        rec = {}
        for m in fr.MEASURES:
            got = eng.run_square(m)
            if path != "auto":
                assert eng.last_path() == path
            tl = eng.run_square(m, tallies=True)
            fin = _finalize(eng, m, tl, n)
            assert np.array_equal(got.view(np.uint64), fin.view(np.uint64)), (path, m)
            ex = fr.exact(m, tl, q, t)
            sm = LD(fr.SERIES_MAX)
            emax = ex.e.max(axis=1)
            near = np.abs(emax / sm - 1) < 0.04
            assert (near & (emax < sm)).sum() >= 20 and (near & (emax >= sm)).sum() >= 20, (path, m)
            if m == "k80":
                eb_only = (tl[:, 1] == 0) & (ex.e[:, 1] >= sm) & (ex.e[:, 0] < sm)
                assert eb_only.sum() >= 50, path
            if m == "tn93":
                binding = np.argmax(ex.e, axis=1)
                for b in range(3):
                    assert (near & (binding == b) & (emax < sm)).any() and (near & (binding == b) & (emax >= sm)).any()
            assert np.isfinite(ex.value.astype(np.float64)).all()
            r = series_error(got, ex)
            rec[m] = float(r.max())
            assert r.max() <= BAR[m], (path, m, float(r.max()), tl[np.argmax(r)].tolist())
        rec["path"] = eng.last_path()
        report("d_" + path, rec)
    finally:
        eng.set_path("auto")
