"""Host-only high-precision reference for the f64 finalisation of jc69 / k80 / tn93 (src/measures.rs:72-190), and
adversarial tallies for the device's two arithmetics (dst_device.hpp: fin_*_fast, the pair kernels' epilogue, and
fin_*_close, the text path's).

Every measure is a sum of terms k_i * -ln(1 - e_i) whose e_i are ratios of the exact integer tallies (and, for tn93,
of the two records' {A,T,G,C} counts).  They are evaluated in numpy longdouble (the 80-bit format on x86-64: 64-bit
significand): each e_i from the integers with a few roundings of 2^-64, then -log1p(-e_i).  `exact()` returns the
value, the scale S = sum |term| the device's error is measured against, and the e_i and k_i themselves.

The tallies are (count_L is the number of sites where both records are known):
  jc69  (n, d)                      n differences over d sites
  k80   (count_L, ts, tv)           transitions, transversions
  tn93  (count_L, count_d, P1, P2)  differences, A<->G and C<->T transitions among them;  q, t = the two records' counts
"""
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, (
    "finalise_reference needs numpy.longdouble with a 64-bit significand (the x87 80-bit format of x86-64 hosts); "
    f"this platform's has {np.finfo(LD).nmant + 1} bits")

SERIES_MAX = 2.0 ** -5          # kSeriesMax: the epilogue's series covers every e_i below it
U32 = (1 << 32) - 1
B24 = 1 << 24
MEASURES = ("jc69", "k80", "tn93")


@dataclass
class Exact:
    value: np.ndarray     # longdouble (N,)
    scale: np.ndarray     # S = sum_i |k_i * -ln(1 - e_i)|
    e: np.ndarray         # (N, terms): the log arguments are 1 - e
    k: np.ndarray         # (N, terms): the terms' factors

    @property
    def min_log_arg(self):
        return np.min(1 - self.e, axis=1)


def _int(x):
    """as Python integers (numpy object arrays): the numerators and denominators below are exact"""
    return np.asarray(x, np.uint64).astype(object)


def _to_ld(v):
    """a non-negative Python integer to longdouble, its top 64 bits kept (relative error below 2^-63)"""
    sh = max(v.bit_length() - 64, 0)
    return np.ldexp(LD(v >> sh), sh)


def _ratio(num, den):
    """num / den for arrays of non-negative Python integers, with the f64 semantics of a zero denominator"""
    out = np.empty(len(num), LD)
    # non-negative integers below 2^64 convert exactly (what _to_ld gives them): whole arrays at once; the others one by one
    small = np.asarray((num >= 0) & (num < (1 << 64)) & (den >= 0) & (den < (1 << 64)), bool)
    if small.any():
        a, b = num[small].astype(np.uint64), den[small].astype(np.uint64)
        with np.errstate(all="ignore"):
            out[small] = np.where(b == 0, np.where(a == 0, LD(np.nan), LD(np.inf)), a.astype(LD) / b.astype(LD))
    for k in np.nonzero(~small)[0]:
        a, b = num[k], den[k]
        out[k] = (np.nan if a == 0 else np.inf) if b == 0 else _to_ld(a) / _to_ld(b)
    return out


def _measure(k_num, k_den, e_num, e_den):
    """terms k_i * -ln(1 - e_i), each k_i and e_i a ratio of integers.  -ln(1 - e) is -log1p(-e) for e < 1/2, and
    -ln(w) with w = (e_den - e_num) / e_den formed from the exact integers above: no cancellation anywhere."""
    k = np.stack([_ratio(a, b) for a, b in zip(k_num, k_den)], axis=1)
    e = np.stack([_ratio(a, b) for a, b in zip(e_num, e_den)], axis=1)
    w = np.stack([_ratio(np.maximum(b - a, 0), b) for a, b in zip(e_num, e_den)], axis=1)
    neg = np.stack([b < a for a, b in zip(e_num, e_den)], axis=1).astype(bool)
    with np.errstate(all="ignore"):
        s = np.where(e < 0.5, -np.log1p(-e), -np.log(w))
        s = np.where(neg, np.nan, s)
        s = np.where(np.isnan(e), np.nan, s)
        s = np.where(e == 0, LD(-0.0), s)          # -k ln(1) = -0.0: the measures' sign of a zero distance
        t = k * s
        v = t[:, 0]
        for i in range(1, t.shape[1]):             # (not sum(): its +0.0 start would turn -0.0 into +0.0)
            v = v + t[:, i]
        scale = np.abs(t).sum(axis=1)
    return Exact(v, scale, e, k)


def jc69(n, d) -> Exact:
    """-0.75 ln(1 - 4/3 n/d) = 0.75 * -ln(1 - e), e = 4n / (3d)"""
    n, d = _int(n), _int(d)
    one = np.ones(len(n), object)
    return _measure([3 * one], [4 * one], [4 * n], [3 * d])


def k80(count_L, ts, tv) -> Exact:
    """-0.5 ln((1 - 2P - Q) sqrt(1 - 2Q)) = 0.5 * -ln(1 - ea) + 0.25 * -ln(1 - eb), ea = (2 ts + tv) / L, eb = 2 tv / L"""
    L, ts, tv = _int(count_L), _int(ts), _int(tv)
    one = np.ones(len(L), object)
    ex = _measure([one, one], [2 * one, 4 * one], [2 * ts + tv, 2 * tv], [L, L])
    # 2 tv = L: the product (1 - ea) sqrt(0) is 0 whatever the sign of 1 - ea, so ln of it is -inf (the sum of the two
    # logarithms would be NaN for ea > 1)
    ex.value = np.where(((2 * tv == L) & (L > 0)).astype(bool), LD(np.inf), ex.value)
    return ex


def tn93(count_L, count_d, p1, p2, q, t) -> Exact:
    """-k1 ln(1 - e1) - k2 ln(1 - e2) - k3 ln(1 - e3) (src/measures.rs:118-190) with g_X = s_X / s_L the pair's base
    frequencies (s_X = q_X + t_X, s_L their sum, s_R = s_A + s_G, s_Y = s_T + s_C), P1, P2, Q = (d - P1 - P2) over L:
      k1 = 2 g_A g_G / g_R,  k2 = 2 g_T g_C / g_Y,  k3 = 2 (g_R g_Y - g_A g_G g_Y / g_R - g_T g_C g_R / g_Y)
      e1 = P1 / k1 + Q / (2 g_R),  e2 = P2 / k2 + Q / (2 g_Y),  e3 = Q / (2 g_R g_Y)
    as ratios of integers.  Zero sums give the reference's NaN (0 / 0, or x / 0 into the log).  A zero value is +0.0
    (:188-190)."""
    L, d, P1, P2 = _int(count_L), _int(count_d), _int(p1), _int(p2)
    q, t = np.asarray(q, np.uint64).astype(object), np.asarray(t, np.uint64).astype(object)
    sA, sT, sG, sC = (q[:, x] + t[:, x] for x in range(4))
    sL, sR, sY = sA + sT + sG + sC, sA + sG, sT + sC
    Q = d - P1 - P2
    AG, TC = sA * sG, sT * sC
    ex = _measure([2 * AG, 2 * TC, 2 * (sR * sR * sY * sY - AG * sY * sY - TC * sR * sR)],
                  [sL * sR, sL * sY, sL * sL * sR * sY],
                  # P1 / k1 + Q / (2 g_R) = s_L (P1 s_R^2 + Q s_A s_G) / (2 L s_A s_G s_R), and so on
                  [sL * (P1 * sR * sR + Q * AG), sL * (P2 * sY * sY + Q * TC), Q * sL * sL],
                  [2 * L * AG * sR, 2 * L * TC * sY, 2 * L * sR * sY])
    # a zero frequency makes its k_i 0 and P_i / k_i 0 / 0 or x / 0 in the reference: NaN, whatever the rest says
    zero = (sA * sT * sG * sC == 0) | (L == 0)
    ex.value = np.where(zero.astype(bool), LD(np.nan), np.where(ex.value == 0, LD(0), ex.value))
    return ex


def exact(measure, tallies, q=None, t=None) -> Exact:
    tl = np.asarray(tallies, np.uint64)
    if measure == "jc69":
        return jc69(tl[:, 0], tl[:, 1])
    if measure == "k80":
        return k80(tl[:, 0], tl[:, 1], tl[:, 2])
    if measure == "tn93":
        return tn93(tl[:, 0], tl[:, 1], tl[:, 2], tl[:, 3], q, t)
    raise ValueError(measure)


# ---------------------------------------------------------------------------------------------------------------------
# adversarial tallies: at, and one count either side of, every branch of fin_*_fast / fin_*_close
def _around(x):
    """the integers next to the real threshold x: the last two below it, the first two at or above it"""
    c = int(np.ceil(float(x)))
    return [c - 2, c - 1, c, c + 1]


def _denominators(rng, n_random):
    """d / count_L: 1,000 .. 2^24 - 1 log-spaced and random, 2^24 - 1 / 2^24 / 2^24 + 1, and a few above"""
    lo = np.unique(np.geomspace(1000, B24 - 1, 60).astype(np.int64))
    rnd = np.exp(rng.uniform(np.log(1000), np.log(B24 - 1), n_random)).astype(np.int64)
    return np.concatenate([lo, rnd, [1000, 1024, 29903, 30000, B24 - 1, B24, B24 + 1]])


def _big(rng, n):
    return np.concatenate([rng.integers(B24 + 2, U32, n), [1 << 28, U32 - 1, U32]])


def jc69_cases(rng):
    """(n, d) pairs, n <= d"""
    out = []
    d = np.concatenate([_denominators(rng, 3000), _big(rng, 200)])
    # series switch: 4n / (3d) around 2^-5
    for dd in d:
        out += [(int(x), int(dd)) for x in _around(3 * dd * SERIES_MAX / 4)]
    # 1-50 differences over L from 1,000 to 2^24 - 1, and over the large denominators
    for dd in np.concatenate([np.unique(np.geomspace(1000, B24 - 1, 60).astype(np.int64)), [B24 - 1, B24, B24 + 1],
                              _big(rng, 20)]):
        out += [(x, int(dd)) for x in range(1, 51)]
    # e from 2^-9 to 1 (series, past the switch, the close path) on random denominators
    dd = np.concatenate([rng.choice(d, 6000), rng.integers(1, 1000, 500)])
    e = np.exp(rng.uniform(np.log(2.0 ** -9), 0, len(dd)))
    nn = np.minimum(np.round(3 * dd * e / 4), dd).astype(np.int64)
    out += list(zip(nn.tolist(), dd.tolist()))
    # the high-diversity end: p through 0.75 (+inf at p = 3/4 exactly, NaN past it), log arguments 1 / (3d) .. 0.01
    for dd in [4, 400, 4000, 29904, B24 - 4, B24, 1 << 28, U32 - 3, U32]:
        base = 3 * dd // 4
        out += [(int(x), dd) for x in range(max(base - 40, 0), min(base + 40, dd) + 1)]
        out += [(int(dd * p), dd) for p in np.linspace(0.74, 1.0, 27)]
    for m in range(1, 200, 3):               # 3d - 4n = m: w = m / (3d), from 2^-33.6 up (d = 2^32 - 1 = 3 mod 4)
        dd = U32
        if (3 * dd - m) % 4 == 0:
            out.append(((3 * dd - m) // 4, dd))
    # degenerate: nothing comparable (0 / 0), nothing different (-0.0)
    out += [(0, 0), (0, 1), (0, 1000), (0, B24), (0, U32), (1, 1), (U32, U32)]
    out += jc69_log_slice(rng)
    t = np.array(out, np.int64)
    assert (t[:, 0] >= 0).all() and (t[:, 0] <= t[:, 1]).all() and (t[:, 1] <= U32).all()
    return t.astype(np.uint32)


def log_cells():
    """the 128 cells of dst_log's table (dst_logtab.h): z in [0.6875, 1.375), the bit pattern of z minus that of 0.6875
    cut into 128 equal pieces; returns (lo, hi) of each"""
    off = 0x3FE6000000000000
    b = np.array([off + (i << 45) for i in range(129)], np.uint64).view(np.float64)
    return b[:-1], b[1:]


def jc69_log_slice(rng):
    """(n, d) whose f64 log argument 1 - 4/3 (n/d) lands at both edges and the middle of every cell of dst_log's table
    (2^k z, k = 0 .. -33): all 128 cells, every binade from 2^-33 to 1"""
    lo, hi = log_cells()
    out = []
    for k in range(0, -34, -1):
        for i in range(128):
            for z in (lo[i], hi[i], 0.5 * (lo[i] + hi[i])):
                w = np.ldexp(z, k)
                if not (0 < w < 1):
                    continue
                d = int(rng.integers(1 << 31, U32)) if k > -31 else U32
                for dz in (-1, 0, 1):
                    n = int(round(3 * d * (1 - w) / 4)) + dz
                    if 0 <= n <= d:
                        out.append((n, d))
    return out


def k80_cases(rng):
    """(count_L, ts, tv), ts + tv <= count_L"""
    out = []
    Ls = np.concatenate([_denominators(rng, 1500), _big(rng, 100)])
    for L in Ls:
        L = int(L)
        # ea binding: (2 ts + tv) / L around 2^-5, tv = 0 and small
        for tv in (0, 1, 3):
            out += [(L, int(ts), tv) for ts in _around((L * SERIES_MAX - tv) / 2)]
        # eb binding: ts = 0, tv around L / 64 (the switch of eb) and just below L / 32 (where ea switches)
        for ts in (0, 1, 2):
            out += [(L, ts, int(tv)) for tv in _around(L * SERIES_MAX / 2)]
            out += [(L, ts, int(tv)) for tv in _around(L * SERIES_MAX - 2 * ts)]
        out += [(L, 0, int(tv)) for tv in np.linspace(L * SERIES_MAX / 2, L * SERIES_MAX, 8).astype(np.int64)]
    # 1-50 differences of either kind
    for L in np.concatenate([np.unique(np.geomspace(1000, B24 - 1, 30).astype(np.int64)), [B24 - 1, B24, B24 + 1]]):
        for x in range(1, 51, 7):
            for y in range(0, 51, 5):
                out += [(int(L), x, y), (int(L), y, x)]
    # (ts + tv) / L from 2^-9 to 1 and past it (NaN), every mix
    L = rng.choice(Ls, 8000)
    frac = np.exp(rng.uniform(np.log(2.0 ** -9), 0, len(L)))
    frac[:800] = rng.uniform(0.3, 1.0, 800)
    diff = np.minimum(np.round(L * frac), L).astype(np.int64)
    ts = np.round(diff * rng.random(len(L))).astype(np.int64)
    ts[:1000] = 0
    out += list(zip(L.tolist(), ts.tolist(), (diff - ts).tolist()))
    # the high-diversity end: 1 - ea or 1 - eb through 0 (+inf, NaN), log arguments down to ~1e-10
    for L in (1000, 4096, 30000, B24 - 2, 1 << 28, U32 - 1):
        h = L // 2
        out += [(L, int(x), 0) for x in range(h - 5, h + 1)]                   # 1 - 2P down to 0
        out += [(L, 0, int(x)) for x in range(h - 5, h + 6)]                   # 1 - 2Q through 0
        out += [(L, int(x), L - 2 * int(x)) for x in range(0, 5)]              # 2P + Q = 1 with Q = 1 - 2P
    # degenerate
    out += [(0, 0, 0), (1, 0, 0), (1000, 0, 0), (B24, 0, 0), (U32, 0, 0), (1, 1, 0), (1, 0, 1), (2, 1, 1)]
    t = np.array(out, np.int64)
    assert (t >= 0).all() and (t[:, 1] + t[:, 2] <= t[:, 0]).all() and (t[:, 0] <= U32).all()
    return t.astype(np.uint32)


def tn93_records():
    """{A,T,G,C} base counts of the records whose pairs carry the tn93 cases (Engine.upload(base_counts=...)):
    balanced and skewed (one base at 0.1 %) frequencies, base counts of 1, one base 0 in both records of a pair (a zero
    frequency sum: least == 0), single counts 2^24 - 1 / 2^24 / 2^24 + 1, halves below 2^24 whose sums are not, and all
    eight counts 2^24 - 1 (the 2^124 product of the reciprocal's seed)"""
    r = []
    for L in (1000, 4096, 29903, 1 << 20, B24 - 1):
        q = L // 4
        r.append((q, q, q, L - 3 * q))                                          # balanced
        r.append((int(0.30 * L), int(0.32 * L), int(0.20 * L), L - int(0.30 * L) - int(0.32 * L) - int(0.20 * L)))
        for x in range(4):                                                       # one base at 0.1 %
            c = [(L - max(L // 1000, 1)) // 3] * 4
            c[x] = max(L // 1000, 1)
            r.append(tuple(c))
    for x in range(4):
        c = [7000] * 4
        c[x] = 1
        r.append(tuple(c))                                                       # a base count of 1
        c = [7000] * 4
        c[x] = 0
        r.append(tuple(c))                                                       # one base 0
        r.append(tuple(c))                                                       # ... twice: its pairs sum to 0
        for v in (B24 - 1, B24, B24 + 1):
            c = [1 << 20] * 4
            c[x] = v
            r.append(tuple(c))
        c = [1 << 22] * 4
        c[x] = (1 << 23) + 3 + x                                                 # halves < 2^24, sums >= 2^24
        r.append(tuple(c))
    r.append((B24 - 1,) * 4)
    r.append((B24 - 1,) * 4)
    r.append((1, 1, 1, 1))
    r.append((0, 0, 0, 0))
    return np.array(r, np.uint64)


def tn93_cases(rng, counts):
    """(count_L, count_d, P1, P2) for every pair (i < j) of records with base counts `counts`, in canonical order;
    each pair carries one case, the kinds taken in turn: e1, e2 or e3 the binding term at the series switch (exactly
    at, one count below, one above), with some transversions beside a binding transition, few differences over a
    large count_L, e from 2^-9 to 1 and past it, and zero counts"""
    n = len(counts)
    i, j = np.triu_indices(n, 1)
    q, t = counts[i], counts[j]
    m = len(i)
    Ls = _denominators(rng, m)
    cL = rng.choice(Ls, m).astype(np.int64)
    cL[::7] = B24 - 1
    cL[3::97] = B24
    cL[5::97] = B24 + 1
    unit = tn93(cL, np.zeros(m, np.int64), np.ones(m, np.int64), np.zeros(m, np.int64), q, t).e[:, 0]   # e1 per P1
    unit2 = tn93(cL, np.ones(m, np.int64), np.zeros(m, np.int64), np.ones(m, np.int64), q, t).e[:, 1]   # e2 per P2
    unitq = tn93(cL, np.ones(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64), q, t).e      # e1..3 per Q
    kind = np.arange(m) % 14
    delta = (np.arange(m) // 14) % 4 - 2
    P1 = np.zeros(m, np.int64)
    P2 = np.zeros(m, np.int64)
    Q = np.zeros(m, np.int64)
    with np.errstate(all="ignore"):
        at1 = np.ceil(SERIES_MAX / unit.astype(np.float64))
        at2 = np.ceil(SERIES_MAX / unit2.astype(np.float64))
        at3 = np.ceil(SERIES_MAX / unitq[:, 2].astype(np.float64))
    fin = lambda x: np.where(np.isfinite(x), x, 0).astype(np.int64)   # noqa: E731
    at1, at2, at3 = fin(at1), fin(at2), fin(at3)
    small_q = rng.integers(0, 4, m)
    s = kind == 0
    P1[s] = at1[s] + delta[s]                                        # e1 binding, nothing else
    s = kind == 1
    P2[s] = at2[s] + delta[s]                                        # e2 binding
    s = kind == 2
    Q[s] = at3[s] + delta[s]                                         # e3 binding (it always is for Q alone)
    s = kind == 3                                                    # e1 binding beside a few transversions
    Q[s] = small_q[s]
    with np.errstate(all="ignore"):
        P1[s] = fin(np.ceil((SERIES_MAX - Q[s] * unitq[s, 0].astype(np.float64)) / unit[s].astype(np.float64)))
    P1[s] += delta[s]
    s = kind == 4
    Q[s] = small_q[s]
    with np.errstate(all="ignore"):
        P2[s] = fin(np.ceil((SERIES_MAX - Q[s] * unitq[s, 1].astype(np.float64)) / unit2[s].astype(np.float64)))
    P2[s] += delta[s]
    s = kind == 5                                                    # 1-50 differences of every kind
    P1[s], P2[s], Q[s] = rng.integers(0, 17, s.sum()), rng.integers(0, 17, s.sum()), rng.integers(0, 17, s.sum())
    for kk, share in ((6, 2.0 ** -9), (7, 2.0 ** -6), (8, 2.0 ** -4), (9, 2.0 ** -2), (10, 0.7), (11, 1.0)):
        s = kind == kk                                               # e of the order of `share` and past it
        diff = np.minimum(np.round(cL[s] * share * rng.uniform(0.5, 1.5, s.sum())), cL[s]).astype(np.int64)
        a = np.round(diff * rng.random(s.sum()) * 0.6).astype(np.int64)
        b = np.round((diff - a) * rng.random(s.sum()) * 0.6).astype(np.int64)
        P1[s], P2[s], Q[s] = a, b, diff - a - b
    # kind 12: P1 = P2 = Q = 0 (+0.0); kind 13: count_L = 0 too (NaN)
    cL[kind == 13] = 0
    P1, P2, Q = np.maximum(P1, 0), np.maximum(P2, 0), np.maximum(Q, 0)
    over = P1 + P2 + Q > cL                                          # keep the tallies consistent
    scale = np.where(over, cL / np.maximum(P1 + P2 + Q, 1), 1.0)
    P1, P2, Q = (np.floor(x * scale).astype(np.int64) for x in (P1, P2, Q))
    tl = np.stack([cL, P1 + P2 + Q, P1, P2], axis=1)
    assert (tl >= 0).all() and (tl[:, 2] + tl[:, 3] <= tl[:, 1]).all() and (tl[:, 1] <= tl[:, 0]).all()
    assert (tl <= U32).all()
    return tl.astype(np.uint32)


def records_for(n_cases):
    """the number of records whose canonical pairs hold n_cases"""
    n = 2
    while n * (n - 1) // 2 < n_cases:
        n += 1
    return n


def cases(measure, seed=20261016):
    """adversarial tallies of `measure`: (tallies (N, w) uint32, base counts (R, 4) or None).  For tn93 the tallies
    belong to the canonical pairs of R records with those counts; jc69 / k80 need no records."""
    rng = np.random.default_rng(seed)
    if measure == "jc69":
        return jc69_cases(rng), None
    if measure == "k80":
        return k80_cases(rng), None
    counts = tn93_records()
    reps = 6                                                           # every profile six times: 6 x 6 pairs per kind
    counts = np.repeat(counts, reps, axis=0)
    return tn93_cases(rng, counts), counts


def pair_counts(counts):
    """(q, t) base counts of the canonical pairs (i < j) of the records with `counts`"""
    i, j = np.triu_indices(len(counts), 1)
    return counts[i], counts[j]
