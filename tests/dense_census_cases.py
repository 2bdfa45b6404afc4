"""The dense census: designed inputs, job shapes and the table of pair_kernel<M, BM, TN, MINW, OUT> instantiations
(dst_kernels.hip) for tests/test_gpu_dense_census.py; tests/test_dense_census_host.py checks without a GPU that the inputs
and shapes have what the GPU module relies on.  Nothing here needs a GPU.

An instantiation is (family, rows per tile, output).  The table is built from the library (dst_variant_count,
dst_plan_tiles), not from a copy of its variant arrays: a variant added to the library shows as a count other than
EXPECTED_INSTANTIATIONS, and has to be given cases here.

Outputs: the measure's native one (int, raw, jc69, k80, tn93), tally, tally16, tally_add (a split-L launch with tally
output, and a split f64 launch, which meets in the scratch buffer and goes through finalize_kernel), int_add (a split
n / n_high distance launch).
"""
import functools

import numpy as np

import distance_amd as da
import oracle
from helpers import alignment_root, random_alignment
from test_gpu_launch_variants import low_diversity, with_clade

ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
F64 = ("jc69", "k80", "tn93")
FAMILY = {"n": 0, "n_high": 0, "raw": 1, "jc69": 1, "k80": 2, "tn93": 3}
NATIVE = {"n": "int", "n_high": "int", "raw": "raw", "jc69": "jc69", "k80": "k80", "tn93": "tn93"}
TALLY_OF = {"n": "n_high", "n_high": "n_high", "raw": "raw", "jc69": "raw", "k80": "k80", "tn93": "tn93"}   # the oracle's name
ORACLE_OF = {"n": "n_high"}           # (n needs the difference lists on the host: the dense path computes n_high's tally)
EXPECTED_INSTANTIATIONS = 50          # n / n_high 3 x 5, raw / jc69 3 x 5, k80 2 x 4, tn93 3 x 4
FILLER = 0xFFFFFFFF                   # i0 of an idle tile of the schedule
CHUNK = 128                           # sites per chunk
FORCED = (2, 4, 7)                    # split factors forced on set A's 6 chunks: 4 gives parts of 1, 2, 1, 2 chunks; 7 is capped to 6
NEIGHBOUR_TIE_CAP = 0.05              # the most pairs of A whose tallies may equal one neighbour's


def variant_count(measure):
    return da.load().dst_variant_count(da.MEASURES[measure])


def variants():
    """(measure, variant) of every tile variant of every measure"""
    return [(m, v) for m in ALL for v in range(variant_count(m))]


def tile_of(measure, variant):
    """(rows per tile, columns per tile) as the library plans them; a variant out of range is variant 0"""
    _, bm, bn = da.plan_tiles(True, 0, 1, 2, measure, variant)
    return bm, bn


def tallest_variant(measure):
    return max(range(variant_count(measure)), key=lambda v: tile_of(measure, v)[0])


def outputs_of(measure):
    """every output a launch of `measure` can end in"""
    return (NATIVE[measure], "tally", "tally16", "tally_add") + (("int_add",) if FAMILY[measure] == 0 else ())


def build_table():
    """(family, rows per tile, out) of every pair_kernel launch_outputs instantiates"""
    return {(FAMILY[m], tile_of(m, v)[0], out) for m, v in variants() for out in outputs_of(m)}


# ---- the sets ----------------------------------------------------------------------------------------------------------
NAN_PAIR = (b"ACGTACGTACGTACGTAAAA", b"CATGCATGCATGCATGAAAA", b"CATGCATGCATGCATTAAAA")   # a-b: p = 0.8, jc69 NaN; a-c: p = 0.75, +inf
A_ALL_N, A_COPY, A_TRIO = 512, 770, (600, 601, 602)
B_ALL_N, B_COPY, B_TRIO = 7, 99, (20, 21, 22)


def designed(n, L, seed, all_n, copy, trio, root=None):
    """random_alignment at 30 % divergence (all 17 codes) with: record all_n all N (raw and tn93 NaN with everybody),
    record copy a copy of the one before it (distance 0, jc69 -0.0), records trio built as those of test_nan_inf_cases_match
    on the first 20 sites, N elsewhere (16 and 15 differences over 20 sites: jc69 NaN and +inf)"""
    codes = random_alignment(n, L, seed, divergence=0.3, root=root)
    codes[all_n] = 240
    codes[copy] = codes[copy - 1]
    for r, text in zip(trio, NAN_PAIR):
        codes[r] = 240
        codes[r, :len(text)] = oracle.encode(text)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def codes_of(name):
    """A: 771 x 677 — two column panels of 512, the second partial with 3 records in its tn = 1 half, 6 chunks (the last of
    37 sites), row tiles of every height straddling the diagonal, npad 1536.  B: 100 x 677 from A's root (one alignment in two
    files: unrelated records would be NaN in most f64 pairs), npad 512: the rectangles' row and column plane strides differ.  C: 70 x 2,049, 17 chunks: the library splits it 2 ways by itself.  H: 300 x 2,048 and
    HW: 40 x 65,600 (32-bit hot tallies): a third of the records share substitutions at 2 % of the sites, hot columns for
    the hybrid path; H40: the first 40 records of H."""
    if name == "A":
        return designed(771, 677, 31, A_ALL_N, A_COPY, A_TRIO)
    if name == "B":
        return designed(100, 677, 32, B_ALL_N, B_COPY, B_TRIO, root=alignment_root(677, 31))
    if name == "C":
        codes = random_alignment(70, 2049, 33, divergence=0.3)
    elif name == "H":
        codes = with_clade(low_diversity(300, 2048, 34), 84)
    elif name == "HW":
        codes = with_clade(low_diversity(40, 65600, 35), 85)
    elif name == "H40":
        codes = codes_of("H")[:40].copy()
    else:
        raise KeyError(name)
    codes.setflags(write=False)
    return codes


# ---- job shapes: rows [rb, re) of set `rows` against (square: the later records of) set `cols` ---------------------------
SHAPES = {
    "square_whole": dict(rows="A", cols="A", square=True, rb=0, re=771),
    "square_37_150": dict(rows="A", cols="A", square=True, rb=37, re=150),     # 113 rows: a partial last tile at every height
    "square_500_530": dict(rows="A", cols="A", square=True, rb=500, re=530),   # across the panel edge on the diagonal
    "square_768_771": dict(rows="A", cols="A", square=True, rb=768, re=771),   # the last rows; row 770 has no pair
    "rect_ab_whole": dict(rows="A", cols="B", square=False, rb=0, re=771),
    "rect_ab_37_150": dict(rows="A", cols="B", square=False, rb=37, re=150),
    "rect_ba_whole": dict(rows="B", cols="A", square=False, rb=0, re=100),
    "rect_ba_5_96": dict(rows="B", cols="A", square=False, rb=5, re=96),
}
SPLIT_SHAPES = ("square_37_150", "rect_ba_whole")
AUTO_SPLIT = dict(rows="C", cols="C", square=True, rb=0, re=70)
HYBRID_SHAPES = {
    "hybrid_square_whole": dict(rows="H", cols="H", square=True, rb=0, re=300),
    "hybrid_square_41_130": dict(rows="H", cols="H", square=True, rb=41, re=130),
    "hybrid_rect": dict(rows="H", cols="H40", square=False, rb=0, re=300),
    "hybrid_wide_whole": dict(rows="HW", cols="HW", square=True, rb=0, re=40),
    "hybrid_wide_3_29": dict(rows="HW", cols="HW", square=True, rb=3, re=29),
}
SLOT = {"A": 0, "B": 1, "C": 0, "H": 0, "H40": 1, "HW": 0}


def chunks_of(name):
    return -(-codes_of(name).shape[1] // CHUNK)


def forced_ksplit(k, shape):
    """the factor a launch forced to k reports: capped at the alignment's chunks"""
    return min(k, chunks_of(shape["rows"]))


def automatic_ksplit(tiles, chunks):
    """run_sets' own rule for launches of fewer than 1,024 tiles on 16 chunks and more: enough parts for 2,048
    workgroups, eight chunks each at least, 64 at the most"""
    if not 0 < tiles < 1024 or chunks < 16:
        return 1
    return max(1, min(-(-2048 // tiles), chunks // 8, 64))


def plan(shape, measure, variant):
    """(tiles with the idle fillers, rows per tile, columns per tile) of one launch"""
    return da.plan_tiles(shape["square"], shape["rb"], shape["re"], len(codes_of(shape["cols"])), measure, variant)


def pairs_of(shape):
    """(i, j) of every pair of the job in the order of its output"""
    n_cols = len(codes_of(shape["cols"]))
    if shape["square"]:
        i, j = np.triu_indices(n_cols, 1)
        keep = (i >= shape["rb"]) & (i < shape["re"])
        return i[keep], j[keep]
    i, j = np.divmod(np.arange((shape["re"] - shape["rb"]) * n_cols), n_cols)
    return i + shape["rb"], j


def hot_is_wide(name):
    """the hybrid path's hot launch writes 16-bit tallies below 65,536 sites and 32-bit ones from there"""
    return codes_of(HYBRID_SHAPES[name]["rows"]).shape[1] >= 65536


# ---- which case names which instantiation ----------------------------------------------------------------------------------
def cases_naming(measure, variant):
    """{(family, rows per tile, out): [the cases of tests/test_gpu_dense_census.py that launch it]} for one (measure, variant)"""
    fam, bm = FAMILY[measure], tile_of(measure, variant)[0]
    named = {}
    for name in SHAPES:
        for out in (NATIVE[measure], "tally", "tally16"):
            named.setdefault((fam, bm, out), []).append(f"{measure} v{variant} {name} {out}")
    for name in HYBRID_SHAPES:
        out = "tally" if hot_is_wide(name) else "tally16"
        named.setdefault((fam, bm, out), []).append(f"{measure} v{variant} {name} hot {out}")
    for name in SPLIT_SHAPES:
        for k in FORCED:
            named.setdefault((fam, bm, "tally_add"), []).append(f"{measure} v{variant} {name} k={k} tally")
            if fam == 0:
                named.setdefault((fam, bm, "int_add"), []).append(f"{measure} v{variant} {name} k={k} distance")
            else:
                named[(fam, bm, "tally_add")].append(f"{measure} v{variant} {name} k={k} distance through the scratch buffer")
    return named


# ---- the oracle's results, once per set pair ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts_of(name):
    return oracle.count_bases_matrix(codes_of(name))


@functools.lru_cache(maxsize=None)
def oracle_tallies(measure, rows, cols):
    """the oracle's tallies of every record of set `rows` against every record of set `cols`: uint64 (n_rows, n_cols, width)"""
    out = oracle.tallies_rect(TALLY_OF[measure], codes_of(rows), codes_of(cols), threads=16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_distances(measure, rows, cols):
    """the oracle's distance of every record of `rows` against every record of `cols`: f64 (n_rows, n_cols)"""
    out = oracle.all_pairs_rect(ORACLE_OF.get(measure, measure), codes_of(rows), codes_of(cols), counts_of(rows), counts_of(cols),
                                threads=16)
    out.setflags(write=False)
    return out


def want_tallies(measure, shape):
    """(pairs, width) uint64 in the job's output order"""
    i, j = pairs_of(shape)
    return oracle_tallies(TALLY_OF[measure], shape["rows"], shape["cols"])[i, j]


def want_distances(measure, shape):
    i, j = pairs_of(shape)
    return oracle_distances(measure, shape["rows"], shape["cols"])[i, j]


@functools.lru_cache(maxsize=None)
def exact_values(measure, rows, cols):
    """finalise_reference's exact value of every pair of (rows x cols), from the oracle's tallies and base counts: an
    Exact whose arrays run over the flattened (n_rows * n_cols) pairs"""
    import finalise_reference as fr
    from helpers import exact_of
    tl = oracle_tallies(TALLY_OF[measure], rows, cols)
    n_rows, n_cols, width = tl.shape
    q = np.repeat(counts_of(rows), n_cols, axis=0)
    t = np.tile(counts_of(cols), (n_rows, 1))
    return exact_of(fr, measure, tl.reshape(-1, width), q, t)


def want_exact(measure, shape):
    """the Exact of the job's pairs, its output order"""
    import finalise_reference as fr
    ex = exact_values(measure, shape["rows"], shape["cols"])
    i, j = pairs_of(shape)
    at = i * len(codes_of(shape["cols"])) + j
    return fr.Exact(ex.value[at], ex.scale[at], ex.e[at], ex.k[at])


def singular(measure, shape):
    """the job's pairs where a logarithm's argument is exactly 0 (some e_i = 1: k80 at 2 ts + tv = count_L, jc69 at
    4 n = 3 d).  The exact value is +inf there, and the reference's own f64 arithmetic may leave a rounding residue in its
    place (k80: 1 - 2P - Q = 5.5e-17, a distance of 18.9, or a NaN): the reference agrees with the exact value on
    NaN, inf and 0 everywhere else (test_dense_census_host.py), so these pairs are held to the reference's bits alone."""
    return np.asarray((want_exact(measure, shape).e == 1).any(axis=1), bool)
