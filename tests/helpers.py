"""Shared test inputs: seeded synthetic alignments over the full 17-code Paradis alphabet; and the bar the census modules
hold device-finalised jc69 / k80 / tn93 to (check_f64)."""
import numpy as np

# the 17 valid codes (src/encoding.rs:7-38)
CODES = np.array([136, 72, 40, 24, 192, 160, 144, 96, 80, 48, 224, 176, 208, 112, 240, 244, 242],
                 np.uint8)
LETTERS = b"AGCTRMWSKYVHDBN-?"
KNOWN = (136, 72, 40, 24)


def alignment_root(L, seed):
    """the root sequence random_alignment(n, L, seed) starts from"""
    return np.random.default_rng(seed).choice(np.array(KNOWN, np.uint8), size=L, p=[0.30, 0.20, 0.18, 0.32])


def random_alignment(n, L, seed, p_ambig=0.02, p_gap=0.02, divergence=0.05, root=None):
    """Root sequence + per-row substitutions + N/gap/IUPAC noise; returns uint8 codes (n, L).
    root: another set's root (alignment_root) in place of this seed's own: two files of one alignment."""
    rng = np.random.default_rng(seed)
    own = rng.choice(np.array(KNOWN, np.uint8), size=L, p=[0.30, 0.20, 0.18, 0.32])
    root = own if root is None else root
    codes = np.tile(root, (n, 1))
    if n and L:
        mut = rng.random((n, L)) < divergence
        codes[mut] = rng.choice(np.array(KNOWN, np.uint8), size=int(mut.sum()))
        amb = rng.random((n, L)) < p_ambig
        codes[amb] = rng.choice(CODES[4:14], size=int(amb.sum()))
        gap = rng.random((n, L)) < p_gap
        codes[gap] = rng.choice(CODES[14:], size=int(gap.sum()))
    return np.ascontiguousarray(codes)


def uniform_codes(n, L, seed):
    """Every one of the 17 codes equally likely at every site (adversarial for the predicates)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.choice(CODES, size=(n, L)))


def to_fasta_bytes(codes_row):
    lut = {int(c): LETTERS[k] for k, c in enumerate(CODES)}
    return bytes(lut[int(c)] for c in codes_row)


def exact_of(fr, measure, tl, q, t):
    """finalise_reference's exact value of every pair; jc69 / k80 on the distinct tallies only (low-diversity rows repeat)"""
    if measure == "tn93":
        return fr.exact(measure, tl, q, t)
    uniq, inv = np.unique(tl, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ex = fr.exact(measure, uniq)
    return fr.Exact(ex.value[inv], ex.scale[inv], ex.e[inv], ex.k[inv])


def check_f64(measure, got, want, tl, q, t, ex=None):
    """jc69 / k80 / tn93 distances of whole rows (concatenated) within test_gpu_finalise_accuracy's bars.  The exact value x
    comes from the launch's own tally rows, which are first tied to the ORACLE's distances of the same pairs: a tally off
    by one moves some e_i, and the value, by 2^-17 of itself or more (tallies stay below 2^17 at 70,001 sites), while the
    host's formula is within 2^-53 / e_i <= 2^-36 of x — so |want - x| <= 2^-27 |x| holds for the right integers only.
    Then: NaN, inf and zeros as the host gives them; where every series argument lies below the switch |got - x| <= BAR S;
    past it the close arithmetic, within CLOSE_ULP of the host's bits.  ex: exact_of() of the same tallies and counts, where
    the caller has computed it already."""
    import finalise_reference as fr
    from test_gpu_finalise_accuracy import BAR, CLOSE_ULP
    ex = exact_of(fr, measure, tl, q, t) if ex is None else ex
    x = ex.value.astype(np.float64)
    special = ~np.isfinite(x) | (x == 0)
    assert np.array_equal(np.isnan(x), np.isnan(want)) and np.array_equal(np.isinf(x), np.isinf(want)), measure
    assert np.array_equal(x == 0, want == 0), measure
    with np.errstate(all="ignore"):
        tied = np.abs(want.astype(fr.LD) - ex.value) <= np.abs(ex.value) * fr.LD(2.0 ** -27)
    assert tied[~special].all(), (measure, int((~tied[~special]).sum()))
    assert np.array_equal(np.isnan(got[special]), np.isnan(want[special])), measure
    keep = special & ~np.isnan(want)
    assert np.array_equal(got[keep].view(np.uint64), want[keep].view(np.uint64)), measure
    sm = fr.LD(fr.SERIES_MAX)
    with np.errstate(all="ignore"):
        unsure = (np.abs(ex.e / sm - 1) < fr.LD(1e-9)).any(axis=1)       # the device's rounded e_i may fall on either side
        series = ~special & ~unsure & (ex.e < sm).all(axis=1)
        err = (np.abs(got.astype(fr.LD) - ex.value) / ex.scale).astype(np.float64)
    assert (err[series] <= BAR[measure]).all(), (measure, float(err[series].max()))
    rest = ~special & ~unsure & ~series
    ulp = np.abs(got[rest].view(np.int64) - want[rest].view(np.int64))
    assert (ulp <= CLOSE_ULP[measure]).all(), (measure, int(ulp.max()))
