"""Designed alignments for the two situations of the `{:.12}` text that random data never produces: plain numpy and
decimal, no GPU.

1. An EXACT tie of the 12th decimal.  A double v has v x 10^12 ending in exactly .5 only if v = a / 8192 with a odd
   (10^12 = 2^12 x 5^12: one more binary place than decimal places).  With `-m raw` that is a pair with 8,192 k
   comparable sites and a suitable difference count; only there does the `tie && (R & 1)` branch of a formatter decide
   the last digit: 1/8192 = 0.0001220703125 stays at ...312 (even), 3/8192 = 0.0003662109375 goes up to ...938.
2. A value >= 10: its text has 15 characters, not 14.  jc69 reaches 10.18 at 196,607 differences over 262,143 sites.

`tie_alignment()` and `long_jc69_alignment()` build sets whose pairs (0, k) have exactly the raw tallies (n_k, d_k) of
a designed list: record 0 is a root of certain bases, record k differs from it at its first n_k sites and is N from
site d_k on.  `expected_field(n, d)` is the expectation of the tie set, from the exact quotient in decimal arithmetic:
it calls neither %-formatting, nor the oracle, nor the code under test.  test_text_rounding_host.py asserts on the oracle
alone that the sets hold these tallies, ties `expected_field` to Python's exact `%.12f` and runs the host formatters
on every exact tie; test_gpu_text_rounding.py runs the sets through every text writer of the device and the CLI.
"""
import decimal
from fractions import Fraction

import numpy as np

A, G, N = 136, 72, 240
KNOWN = (136, 72, 40, 24)
TIE_L = 24_576
TIE_D = 8_192
FIXED_A = (1, 3, 5, 7, 4095, 4097, 8189, 8191)    # 2^-13 a: sh = 65, 64, 63, 63 in put_fixed12, then the middle and the top
N_DRAWN = 220
N_OTHER = 24                                      # how many a go through the denominators 16,384 and 24,576 as well
N_CONTROL = 12                                    # ... and have their two neighbours (a - 1, a + 1) in the set
LONG_L = 262_143
LONG_ND = ((196_607, LONG_L), (196_606, LONG_L), (196_608, LONG_L), (1, LONG_L))   # 10.18..., 8.97..., NaN, 3.8e-6
_CTX = decimal.Context(prec=60, rounding=decimal.ROUND_HALF_EVEN)
_Q12 = decimal.Decimal(1).scaleb(-12)


def expected_field(n, d):
    """`{:.12}` of n / d for a quotient whose decimal expansion terminates (every d here is 2^k or 3 x 2^k with n a
    multiple of 3): the exact quotient, quantised to 12 places half to even.  d = 0: the 0 / 0 of raw"""
    if d == 0:
        return "NaN"
    q = _CTX.divide(decimal.Decimal(n), decimal.Decimal(d))
    assert _CTX.multiply(q, decimal.Decimal(d)) == n, (n, d)   # exact: nothing was rounded before the quantisation
    return format(q.quantize(_Q12, context=_CTX), "f")


def is_tie(n, d):
    """n / d x 10^12 ends in exactly .5"""
    return d != 0 and (Fraction(n, d) * 10 ** 12 * 2) % 2 == 1


def rounds_up(n, d):
    """a tie whose even neighbour is the upper one"""
    return is_tie(n, d) and (Fraction(n, d) * 10 ** 12 - Fraction(1, 2)) % 2 == 1


def tie_cases():
    """the (n_k, d_k) of records 1 ..: the d = 8,192 cases first (what the CLI test cuts the set to), then the others"""
    rng = np.random.default_rng(20261018)
    odd = np.arange(9, TIE_D - 4, 2)
    odd = odd[~np.isin(odd, FIXED_A)]
    drawn = [int(a) for a in rng.choice(odd, size=N_DRAWN, replace=False)]
    ties = list(FIXED_A) + drawn
    cases = [(a, TIE_D) for a in ties]
    control_a = (1, 3, 4095, 8191) + tuple(drawn[:N_CONTROL - 4])
    for a in control_a:                           # one count either side of a tie: an even a / 8192 has 12 digits
        cases += [(a - 1, TIE_D), (a + 1, TIE_D)]
    cases += [(0, TIE_D), (TIE_D, TIE_D)]          # n = 0 and n = d (the controls of 1 and 8191 are these again)
    other_a = (1, 3) + tuple(drawn[N_CONTROL:N_CONTROL + N_OTHER - 2])
    cases += [(2 * a, 2 * TIE_D) for a in other_a]   # the same values through other denominators
    cases += [(3 * a, 3 * TIE_D) for a in other_a]
    cases += [(1, 2 * TIE_D),                     # 0.00006103515625: 14 digits, below the tie
              (0, 3 * TIE_D), (2 * TIE_D, 2 * TIE_D), (3 * TIE_D, 3 * TIE_D)]
    return cases


def ids_of(n, prefix=""):
    """ids of every length from 0 to 22 (record 5's is empty), so that the numbers of the text start at every offset
    modulo 16; a digit prefix keeps them distinct"""
    out = []
    for k in range(n):
        tag = "%s%d" % (prefix, k)
        want = (7 * k + 1) % 23
        out.append("" if k == 5 else (tag + "x" * 22)[:max(want, len(tag))])
    return out


def designed_alignment(L, cases, seed):
    """codes uint8 (1 + len(cases), L): record 0 the root; record k differs from it at its first n_k sites and is N
    from site d_k on, so that the raw / jc69 tallies of pair (0, k) are exactly (n_k, d_k)"""
    rng = np.random.default_rng(seed)
    root = rng.choice(np.array(KNOWN, np.uint8), size=L)
    codes = np.tile(root, (len(cases) + 1, 1))
    for k, (n, d) in enumerate(cases, start=1):
        assert 0 <= n <= d <= L
        codes[k, :n] = np.where(root[:n] == A, G, A)
        codes[k, d:] = N
    return np.ascontiguousarray(codes)


def tie_alignment():
    """(codes (307, 24,576), cases, ids)"""
    cases = tie_cases()
    codes = designed_alignment(TIE_L, cases, 1)
    return codes, cases, ids_of(len(codes))


def cli_subset(cases, most=260):
    """indices of the root and the d = 8,192 records, at most `most` of them: a FASTA file of a few MB"""
    return [0] + [k for k, (_, d) in enumerate(cases, start=1) if d == TIE_D][:most - 1]


def long_jc69_alignment():
    """(codes (5, 262,143), cases, ids): the 32-bit tally form, a jc69 of 10.18 (15 characters), 8.97, NaN, 3.8e-6"""
    cases = list(LONG_ND)
    codes = designed_alignment(LONG_L, cases, 2)
    return codes, cases, ["root", "ten", "nine_", "nan", "one___"]


def format_values():
    """what the host formatters are run on: every odd a / 8192 below 1, k + a / 8192 for a few integer parts of every
    length up to the last below 1.8e7 (where fmt_fixed12 leaves 64 bits), and the negatives; each is a tie and exact in
    a double.  -> list of (sign, k, a)"""
    out = []
    for sign in (1, -1):
        for k in (0, 1, 9, 10, 99, 12_345, 17_999_999):
            out += [(sign, k, a) for a in range(1, TIE_D, 2)]
    return out


def format_value(sign, k, a):
    return sign * (k + a / TIE_D)                 # exact: at most 25 + 13 bits


def expected_format(sign, k, a):
    return ("-" if sign < 0 else "") + expected_field(k * TIE_D + a, TIE_D)
