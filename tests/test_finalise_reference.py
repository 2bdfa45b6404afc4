"""CPU: the high-precision finalisation reference (finalise_reference.py) the GPU accuracy tests measure against,
pinned three ways: against mpmath at 50 digits on the adversarial tallies, against the oracle's glibc finalisation
where the f64 formula is well conditioned, and against the reference's own f64 golden vectors."""
import fractions

import numpy as np
import pytest

import finalise_reference as fr
import oracle

LD = np.longdouble


def _adversarial(measure, size, seed):
    """a sample of the adversarial cases: every kind of case is in it (they come in runs; the sample takes a stride
    and random picks), as (tallies, q, t)"""
    tl, counts = fr.cases(measure)
    q, t = (None, None) if counts is None else fr.pair_counts(counts)
    rng = np.random.default_rng(seed)
    idx = np.unique(np.concatenate([np.arange(0, len(tl), max(len(tl) // (size // 2), 1)),
                                    rng.choice(len(tl), size // 2, replace=False)]))
    return tl[idx], None if q is None else q[idx], None if t is None else t[idx]


def _mp_exact(measure, tl, q, t):
    """the same terms with mpmath at 50 digits: (value, S) as mpf, or None where the value is not finite"""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 50
    z = [mp.mpf(int(x)) for x in tl]
    if measure == "jc69":
        n, d = z
        if d == 0:
            return None
        terms = [(mp.mpf(3) / 4, 4 * n / (3 * d))]
    elif measure == "k80":
        L, ts, tv = z
        if L == 0:
            return None
        terms = [(mp.mpf(1) / 2, (2 * ts + tv) / L), (mp.mpf(1) / 4, 2 * tv / L)]
    else:
        L, d, P1, P2 = z
        sA, sT, sG, sC = (mp.mpf(int(q[x]) + int(t[x])) for x in range(4))
        sL, sR, sY = sA + sT + sG + sC, sA + sG, sT + sC
        if L == 0 or 0 in (sA, sT, sG, sC):
            return None
        gA, gT, gG, gC, gR, gY = (x / sL for x in (sA, sT, sG, sC, sR, sY))
        P1, P2, Q = P1 / L, P2 / L, (d - z[2] - z[3]) / L
        k1, k2 = 2 * gA * gG / gR, 2 * gT * gC / gY
        k3 = 2 * (gR * gY - gA * gG * gY / gR - gT * gC * gR / gY)
        terms = [(k1, P1 / k1 + Q / (2 * gR)), (k2, P2 / k2 + Q / (2 * gY)), (k3, Q / (2 * gR * gY))]
    if any(e >= 1 for _, e in terms):
        return None
    vals = [-k * mp.log(1 - e) for k, e in terms]
    return sum(vals), sum(abs(v) for v in vals)


@pytest.mark.parametrize("measure", fr.MEASURES)
def test_reference_against_mpmath(measure):
    """<= 1e-17 S on ~3,000 adversarial cases per measure: the series switches, counts around 2^24, degenerate counts,
    1-50 differences, the high-diversity end and (jc69) the cells of the table logarithm"""
    mpmath = pytest.importorskip("mpmath")
    tl, q, t = _adversarial(measure, 3000, 1)
    ex = fr.exact(measure, tl, q, t)
    checked = 0
    for k in range(len(tl)):
        want = _mp_exact(measure, tl[k], None if q is None else q[k], None if t is None else t[k])
        got = ex.value[k]
        if want is None:
            assert not np.isfinite(got) or got == np.inf, (measure, tl[k])
            continue
        v, s = (LD(mpmath.nstr(x, 30, min_fixed=-np.inf, max_fixed=np.inf)) for x in want)
        assert np.isfinite(got), (measure, tl[k])
        assert abs(got - v) <= LD(1e-17) * s, (measure, tl[k], got, v, s)
        assert abs(ex.scale[k] - s) <= LD(1e-17) * s, (measure, tl[k])
        checked += 1
    assert checked > 1500, checked


@pytest.mark.parametrize("measure", fr.MEASURES)
def test_reference_against_the_oracle(measure):
    """Where every log argument is at least 2^-10, the oracle's f64 formula (glibc log, the reference's operation
    order) lies within a few roundings of its inputs from the exact value: each log argument 1 - e_i is formed in f64
    with an absolute error of a few 2^-53 (it lies in [2^-10, 1]), which moves the value by that over 1 - e_i times
    k_i, and the value itself takes a few relative roundings:  |oracle - x| <= 2^-50 S + 2^-51 sum_i k_i / (1 - e_i).
    (Near e_i = 0 that is far more than an ulp of the value: 1 - e loses the low bits of a small e.)  Where every
    e_i lies in [1/8, 1/2] it is a few ulp.  Not finite / zero values: the same NaN / inf pattern, and the sign of
    zero the measure's formula gives."""
    tl, counts = fr.cases(measure)
    q, t = (None, None) if counts is None else fr.pair_counts(counts)
    ex = fr.exact(measure, tl, q, t)
    host = np.array([oracle.finalize(measure, tl[k], None if q is None else q[k], None if t is None else t[k])
                     for k in range(len(tl))])
    x = ex.value.astype(np.float64)
    with np.errstate(all="ignore"):
        good = np.isfinite(x) & (ex.min_log_arg >= LD(2.0 ** -10))
        cond = np.sum(ex.k / (1 - ex.e), axis=1)
    assert good.sum() > len(tl) // 3
    err = np.abs(host[good].astype(LD) - ex.value[good])
    bar = LD(2.0 ** -50) * ex.scale[good] + LD(2.0 ** -51) * cond[good]
    assert np.all(err <= bar), (measure, tl[good][np.argmax(err / bar)], float(np.max(err / bar)))
    mid = good & (ex.e.min(axis=1) >= LD(0.125)) & (ex.e.max(axis=1) <= LD(0.5))
    assert mid.sum() > 100, measure
    assert np.all(np.abs(host[mid] - x[mid]) <= 8 * np.spacing(x[mid])), measure
    assert np.array_equal(np.isnan(host), np.isnan(x)), measure
    inf = np.isinf(x)
    assert np.array_equal(host[inf], x[inf]), measure
    zero = x == 0
    assert zero.any() and np.array_equal(host[zero], x[zero]) and \
        np.array_equal(np.signbit(host[zero]), np.signbit(ex.value[zero])), measure


def test_reference_against_the_golden_vectors(golden):
    """the reference's own 15-bp pair (src/measures.rs:240-308): raw exactly, jc69 / k80 / tn93 within 2 ulp of the
    f64 values the reference computes"""
    seen = set()
    for v in golden["measures"]:
        m = v["measure"]
        if m in ("n", "n_high"):
            continue
        q, t = oracle.encode(v["query"].encode()), oracle.encode(v["target"].encode())
        want = float.fromhex(v["hex"])
        tl = oracle.tallies(m, q, t)
        if m == "raw":
            assert float(fractions.Fraction(int(tl[0]), int(tl[1]))) == want
        else:
            qc, tc = oracle.count_bases(q)[None, :], oracle.count_bases(t)[None, :]
            x = fr.exact(m, tl[None, :], qc, tc).value[0]
            assert abs(x - LD(want)) <= 2 * np.spacing(want), (m, float(x), want)
        seen.add(m)
    assert seen == {"raw", "jc69", "k80", "tn93"}


def test_adversarial_tallies_reach_every_branch():
    """the generator's cases sit on both sides of every switch of fin_*_fast: the series bound of each term, the
    k80 term eb alone past it (ts = 0, L/64 <= tv < L/32), tallies and base counts around 2^24, least == 0, and the
    jc69 slice covers all 128 cells of dst_log's table in every binade from 2^-33 to 1"""
    sm = LD(fr.SERIES_MAX)
    tl, _ = fr.cases("jc69")
    e = fr.exact("jc69", tl).e[:, 0]
    gap = np.abs(e - sm) * 3 * tl[:, 1].astype(LD) / 4           # in counts of n
    assert ((e < sm) & (gap <= 1)).sum() > 1000 and ((e >= sm) & (gap <= 1)).sum() > 1000
    assert (tl[:, 1] >= fr.B24).sum() > 200 and (tl[:, 1] == fr.U32).any()
    with np.errstate(all="ignore"):
        w = 1.0 - (4.0 / 3.0) * (tl[:, 0].astype(np.float64) / tl[:, 1].astype(np.float64))   # the f64 argument
    ok = (w > 0) & (w <= 1)
    mant, expo = np.frexp(w[ok])                                     # w = mant 2^expo, mant in [0.5, 1)
    bits = w[ok].view(np.uint64) - np.uint64(0x3FE6000000000000)
    cell = (bits >> np.uint64(45)) & np.uint64(127)
    assert len(np.unique(cell)) == 128
    assert set(range(-32, 1)) <= set(np.unique(expo).tolist())
    for b in range(-20, 1):                                          # (below, d < 2^32 spaces the arguments wider)
        assert len(np.unique(cell[expo == b])) >= 48, b

    tl, _ = fr.cases("k80")
    e = fr.exact("k80", tl).e
    L, ts, tv = (tl[:, x].astype(np.int64) for x in range(3))
    only_eb = (ts == 0) & (e[:, 1] >= sm) & (e[:, 0] < sm)           # what the guard on ea alone sent to the series
    assert only_eb.sum() > 1000 and (only_eb & (L < fr.B24)).sum() > 500
    assert ((e[:, 0] < sm) & (e[:, 1] < sm) & (np.abs(e[:, 1] - sm) * L <= 2)).sum() > 500
    assert ((e[:, 0] >= sm) & ((e[:, 0] - sm) * L <= 2)).sum() > 500
    assert np.isin([fr.B24 - 1, fr.B24, fr.B24 + 1], L).all()

    tl, counts = fr.cases("tn93")
    q, t = fr.pair_counts(counts)
    ex = fr.exact("tn93", tl, q, t)
    with np.errstate(all="ignore"):
        binding = np.nanargmax(np.where(np.isnan(ex.e), -1, ex.e), axis=1)
        near = np.abs(ex.e.max(axis=1) / sm - 1) < 0.05
    for b in range(3):
        assert ((binding == b) & near & (ex.e.max(axis=1) < sm)).sum() > 50, b
        assert ((binding == b) & near & (ex.e.max(axis=1) >= sm)).sum() > 50, b
    s = q.astype(np.int64) + t.astype(np.int64)
    assert (s.min(axis=1) == 0).sum() > 50                            # least == 0
    assert ((s >= fr.B24) & (np.maximum(q, t) < fr.B24)).any()         # sums past 2^24 of halves below it
    assert ((q == fr.B24 - 1).all(axis=1) & (t == fr.B24 - 1).all(axis=1)).any()
    assert np.isin([fr.B24 - 1, fr.B24, fr.B24 + 1], q).all()
    assert (tl[:, 0] == 0).any() and ((tl[:, 1] == 0) & (tl[:, 0] > 0)).any()
