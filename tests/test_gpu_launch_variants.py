"""GPU (-m gpu): a census of consensus_pair_kernel<FAM, WIDE, OUT, EW> (dst_consensus.hip).

The host picks the instantiation and the tile height of every consensus-path launch from its size and the sampled
statistics of the column set (plan_consensus_launch in dst_api.cpp, exported as dst_plan_consensus_launch).  TABLE lists
every instantiation launch_consensus_pairs can reach, CASES gives for each an input and a call that reaches it.  Every
launch here
  1. asserts with Engine.last_launch() that the intended instantiation and tile height ran (a case that lands elsewhere
     fails);
  2. is compared whole, on the device, bit for bit with the dense kernels of a second engine;
  3. is compared with the oracle directly on whole rows at tile and panel edges (census_rows, every case): n / n_high /
     raw exactly; jc69 / k80 / tn93 whole rows within test_gpu_finalise_accuracy's bars against the exact value
     (check_f64); tallies exactly on one column of every 64 of each row, and on whole rows wherever the oracle's
     distances pin the integers (check_tally_row).
The closing test holds the instantiations seen against TABLE.  tests/test_launch_plan_host.py checks without a GPU that
TABLE is what the plan function can return and that every case's shape reaches the variant it names.
"""
import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import CODES, check_f64

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
KNOWN4 = np.array([136, 72, 40, 24], np.uint8)
FAMILY = {"n": 0, "n_high": 0, "raw": 1, "jc69": 1, "k80": 2, "tn93": 3}
NATIVE = {"n": "int", "n_high": "int", "raw": "raw", "jc69": "jc69", "k80": "k80", "tn93": "tn93"}
KIND_NAME = {da.OUT_TALLY: "tally", da.OUT_TALLY16: "tally16"}
PANEL = 2048
SAMPLE = 192       # columns per row held to the exact value


def out_name(measure, kind):
    return KIND_NAME.get(kind, NATIVE[measure])


def default_ew(out, wide):
    """event_waves<FAM, WIDE, OUT>(): tn93's distance output runs without roles (wide: one event wave), all else 2 + 6"""
    return (1 if wide else 8) if out == "tn93" else 2


def ew_of(heavy, out, wide):
    """launch_cpair: heavy_events 2 -> 8 (no roles), 1 -> 4, else the output's default"""
    return 8 if heavy == 2 else 4 if heavy == 1 else default_ew(out, wide)


def build_table():
    """(family, wide, out, EW) of every consensus_pair_kernel launch_cpair_outputs / launch_cpair instantiate"""
    outs = {0: ("int",), 1: ("raw", "jc69"), 2: ("k80",), 3: ("tn93",)}
    table = set()
    for fam in range(4):
        for wide in (False, True):
            for out in outs[fam] + ("tally",) + (() if wide else ("tally16",)):
                for heavy in (0, 1, 2):
                    table.add((fam, wide, out, ew_of(heavy, out, wide)))
    return table


TABLE = build_table()          # 65: 13 narrow and 9 wide outputs x three wave splits, tn93's default being the no-roles one


def low_diversity(n, L, seed, subs=3e-3, p_n=2e-3, p_amb=3e-4, gap_rows=0.05):
    """SARS-CoV-2-like, as low_diversity of test_gpu_consensus.py (one root, sparse substitutions, sparse N / - / ? and
    IUPAC codes, terminal gap runs: all 17 codes), drawn sparsely so that a 16,000 x 70,001 set takes seconds."""
    rng = np.random.default_rng(seed)
    root = rng.choice(KNOWN4, size=L)
    codes = np.tile(root, (n, 1))
    flat = codes.reshape(-1)
    for p, alphabet in ((subs, KNOWN4), (p_n, CODES[14:]), (p_amb, CODES[4:14])):
        at = rng.integers(0, n * L, size=rng.binomial(n * L, p))
        flat[at] = rng.choice(alphabet, size=len(at))
    for r in np.nonzero(rng.random(n) < gap_rows)[0]:
        codes[r, : rng.integers(0, min(L, 60) + 1)] = 244
        codes[r, L - rng.integers(0, min(L, 60) + 1):] = 244
    return codes


def with_clade(codes, seed, frac=0.33, sites=0.02):
    """a third of the records share substitutions at 2 % of the sites: hot columns for the hybrid path"""
    rng = np.random.default_rng(seed)
    n, L = codes.shape
    clade = np.nonzero(rng.random(n) < frac)[0]
    alt = {136: 72, 72: 136, 40: 24, 24: 40}
    for s in np.nonzero(rng.random(L) < sites)[0]:
        codes[clade, s] = alt.get(int(codes[0, s]), 24)
    return codes


def with_runs(codes, seed, share=0.01):
    """1 % of the records lose half their sites to a run of N: run records (four whole 128-site chunks of N and more)"""
    rng = np.random.default_rng(seed)
    n, L = codes.shape
    for r in rng.choice(n, size=max(1, int(n * share)), replace=False):
        a = int(rng.integers(0, L // 2))
        codes[r, a:a + L // 2] = 240
    return codes


# Every case: rows x L of low_diversity data (cols: a rectangle against a second set of that many records), the path, the
# (heavy_events, rows_per_tile) it must reach for every measure, the sample statistics the shape is expected to give
# (events per pair, list length: what test_launch_plan_host.py feeds the plan function), and which launches run.
# Rates: p = 0.75 subs + p_n + p_amb of the sites deviate; list = p L (+ ~3 from the gap runs), events = p^2 L + list / 512
# (the 512-record sample over-states the sum of squares by that much).
EVERY = tuple((m, k) for m in ALL for k in (da.OUT_DISTANCE, da.OUT_TALLY, da.OUT_TALLY16))
EVERY_WIDE = tuple((m, k) for m in ALL for k in (da.OUT_DISTANCE, da.OUT_TALLY))
BIG = tuple((m, da.OUT_DISTANCE) for m in ALL) + tuple((m, k) for m in ("n_high", "raw", "k80", "tn93")
                                                       for k in (da.OUT_TALLY, da.OUT_TALLY16))
BIG_WIDE = tuple((m, da.OUT_DISTANCE) for m in ALL) + tuple((m, da.OUT_TALLY) for m in ("n_high", "raw", "k80", "tn93"))
FEW = (("n_high", da.OUT_DISTANCE), ("raw", da.OUT_DISTANCE), ("k80", da.OUT_DISTANCE), ("k80", da.OUT_TALLY),
       ("raw", da.OUT_TALLY), ("raw", da.OUT_TALLY16))
CASES = {
    # the default split (2 + 6 waves; tn93: no roles) at each tile height: whole squares of 1.2e8 pairs and more
    "square_16000": dict(n=16000, L=600, gen={}, path="consensus", heavy=0, rows=8, events=0.03, list=6, runs=BIG),
    "square_22000": dict(n=22000, L=600, gen={}, path="consensus", heavy=0, rows=16, events=0.03, list=6, runs=BIG),
    "square_30000": dict(n=30000, L=600, gen={}, path="consensus", heavy=0, rows=32, events=0.03, list=6, runs=BIG),
    "rect_16384_x_24576": dict(n=16384, cols=24576, L=600, gen={}, path="consensus", heavy=0, rows=32, events=0.03, list=6,
                               runs=BIG),
    # 32-bit accumulators: 2 + 6 waves, tn93 1 + 7
    "wide_16000": dict(n=16000, L=70001, gen=dict(subs=8e-4, p_n=1.5e-4, p_amb=5e-5), path="consensus", heavy=0, rows=8,
                       events=0.17, list=59, runs=BIG_WIDE),
    # 4 + 4 waves: events between 0.3 and 1 per pair (narrow), lists beyond 100 entries (wide), run records and hot columns
    # (which keep n / n_high / raw / k80 at 4 + 4 whatever the size: split_helps)
    "ew4_events": dict(n=2500, L=3000, gen=dict(subs=1.2e-2, p_n=3e-3, p_amb=5e-4), path="consensus", heavy=1, rows=8,
                       events=0.55, list=40, runs=EVERY),
    "ew4_wide_lists": dict(n=600, L=70001, gen=dict(subs=1.6e-3, p_n=4e-4, p_amb=1e-4), path="consensus", heavy=1, rows=8,
                           events=0.44, list=122, runs=EVERY_WIDE),
    "ew4_run_records_16000": dict(n=16000, L=1500, gen={}, extra="runs", path="consensus", heavy=1, rows=8, events=0.06,
                                  list=10, run_adds=0.02, runs=FEW),
    "ew4_hybrid_16000": dict(n=16000, L=600, gen={}, extra="clade", path="hybrid", heavy=1, rows=8, events=0.03, list=6,
                             runs=FEW),
    # no roles: more than one event per pair (clade structure on 3 % substitutions), also under the hybrid path
    "ew8_events": dict(n=1500, L=3000, gen=dict(subs=4e-2), extra="clade", path="consensus", heavy=2, rows=8, events=5.0,
                       list=160, runs=EVERY),
    "ew8_hybrid": dict(n=1500, L=3000, gen=dict(subs=4e-2), extra="clade", path="hybrid", heavy=2, rows=8, events=3.0,
                       list=100, runs=FEW),
    "ew8_wide": dict(n=400, L=70001, gen=dict(subs=2e-2, p_n=1e-2), path="consensus", heavy=2, rows=8, events=40.0,
                     list=1700, runs=EVERY_WIDE),
}


def case_shape(c):
    """(square, rows in the launch, column records, pairs)"""
    if "cols" in c:
        return False, c["n"], c["cols"], c["n"] * c["cols"]
    return True, c["n"], c["n"], c["n"] * (c["n"] - 1) // 2


def expected_of(c, measure, kind):
    """the (family, wide, out, EW) a launch of the case must report"""
    wide = c["L"] >= 65536
    out = out_name(measure, kind)
    return (FAMILY[measure], wide, out, ew_of(c["heavy"], out, wide))


def census_rows(n_rows, n_cols, square, seed):
    """rows 0, 1, the last two, the edges of 32-, 16- and 8-row tiles, either side of the column panels' boundaries, the
    diagonal tile of the last (partial) panel, and a seeded random dozen"""
    last = n_rows - 2 if square else n_rows - 1          # (the last row of a square has no pair)
    rows = {0, 1, last - 1, last}
    for r in (32, 16, 8):
        for t in (1, 3, 100, 200, 401):
            rows |= {r * t - 1, r * t, r * t + 1}
    for p in range(1, 4):
        rows |= {PANEL * p - 1, PANEL * p, PANEL * p + 1}
    p0 = (n_cols - 1) // PANEL * PANEL                     # first column of the last panel
    rows |= {p0 - 1, p0, p0 + 1, p0 + 31, p0 + 32, p0 + 33, (p0 + n_cols) // 2}
    rng = np.random.default_rng(seed)
    rows |= {int(x) for x in rng.integers(0, last + 1, 12)}
    return sorted(r for r in rows if 0 <= r <= last)


SEEN = {}      # (family, wide, out, EW) -> rows per tile it was seen with


@pytest.fixture(scope="module")
def engines():
    cons, dense = da.Engine(0), da.Engine(0)
    dense.set_path("dense")
    yield cons, dense
    cons.close()
    dense.close()


def make_case(name):
    c = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    a = low_diversity(c["n"], c["L"], seed, **c["gen"])
    if c.get("extra") == "clade":
        a = with_clade(a, seed + 50)
    if c.get("extra") == "runs":
        a = with_runs(a, seed + 60)
    b = low_diversity(c["cols"], c["L"], seed, **c["gen"]) if "cols" in c else None      # the same root: one alignment, two files
    if b is not None:
        b[1] = a[1]                                                                       # an identical pair across the files
    return a, b


def check_tally_row(measure, kind, got, i, j0, a, cols, tal32, rng):
    """one row of a tally launch against the oracle.  DST_OUT_TALLY: exactly, on one column of every 64 (any run of 128
    columns, however aligned, holds one: a lost group of a wave's line-groups shows in every row) and on the panel edges;
    whole rows where the oracle's distances pin the integers: {d} of n / n_high is its distance, {n, d} of raw / jc69 has
    n = n_high's distance and n / d = raw's bits.  (k80's and tn93's whole rows are tied to the oracle's distances where
    the f64 bars take the exact value from them: check_f64.)  DST_OUT_TALLY16: the 32-bit rows, whole."""
    om = "n_high" if measure == "n" else measure
    n_cols = len(cols)
    if kind == da.OUT_TALLY16:
        assert np.array_equal(got.astype(np.uint32), tal32), (measure, kind, i)
        return
    blocks = np.arange(j0, n_cols, 64)
    js = np.minimum(blocks + rng.integers(0, 64, len(blocks)), n_cols - 1)
    js = sorted(set(js.tolist()) | {j0, n_cols - 1} | {j for j in (PANEL - 1, PANEL, 2 * PANEL - 1, 2 * PANEL) if j0 <= j < n_cols})
    for j in js:
        assert list(got[j - j0]) == [int(x) for x in oracle.tallies(om, a[i], cols[j])], (measure, kind, i, j)
    if FAMILY[measure] <= 1:
        d = oracle.all_pairs_rect("n_high", a[i:i + 1], cols[j0:], threads=16)[0].astype(np.int64)
        assert np.array_equal(got[:, 0].astype(np.int64), d), (measure, kind, i)
    if FAMILY[measure] == 1:
        raw = oracle.all_pairs_rect("raw", a[i:i + 1], cols[j0:], threads=16)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            mine = got[:, 0].astype(np.float64) / got[:, 1].astype(np.float64)
        assert np.array_equal(mine, raw, equal_nan=True), (measure, kind, i)


def check_rows_against_the_oracle(measure, kind, buf, width, rows, a, b, counts_a, counts_b, tal_rows):
    """rows of a launch's device buffer against the oracle; tal_rows: {row: the DST_OUT_TALLY row of this measure's
    family}, fetched from the tally launch that ran before"""
    square = b is None
    cols = a if square else b
    n_cols = len(cols)
    om = "n_high" if measure == "n" else measure
    rng = np.random.default_rng(7)
    f64 = ([], [], [], [], [])
    for i in rows:
        first = da.square_row_start(n_cols, i) if square else i * n_cols
        j0 = i + 1 if square else 0
        count = n_cols - j0
        got = buf[first * width:(first + count) * width].cpu().numpy()
        if kind != da.OUT_DISTANCE:
            got = got.view(np.uint16 if kind == da.OUT_TALLY16 else np.uint32).reshape(count, width)
            check_tally_row(measure, kind, got, i, j0, a, cols, tal_rows[i], rng)
            continue
        want = oracle.all_pairs_rect(om, a[i:i + 1], cols[j0:], counts_a[i:i + 1], counts_b[j0:], threads=16)[0]
        if measure in da.INT_MEASURES:
            assert np.array_equal(got.view(np.int64), want.astype(np.int64)), (measure, i)
        elif measure == "raw":       # one correctly rounded division: the reference's bits
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (measure, i)
        else:
            for lst, v in zip(f64, (got.view(np.float64), want, tal_rows[i], np.broadcast_to(counts_a[i], (count, 4)),
                                    counts_b[j0:])):
                lst.append(v)
    if f64[0]:
        g, w, tl, q, t = (np.concatenate(v) for v in f64)
        check_f64(measure, g, w, tl, q, t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_instantiation_against_the_dense_kernels_and_the_oracle(engines, name):
    torch = pytest.importorskip("torch")
    cons, dense = engines
    c = CASES[name]
    a, b = make_case(name)
    square, n_rows, n_cols, pairs = case_shape(c)
    dev = torch.device("cuda", 0)
    for e in (cons, dense):
        if e is cons:
            e.set_path("auto")         # (the fused preparation of an open path: run records are found by it)
        e.upload(0, a)
        if b is not None:
            e.upload(1, b)
    cons.set_path(c["path"])
    counts_a = cons.base_counts(0).astype(np.uint64)
    counts_b = counts_a if b is None else cons.base_counts(1).astype(np.uint64)
    rows = census_rows(n_rows, n_cols, square, 11)
    assert len(rows) >= 64 or pairs < 10_000_000, len(rows)
    bufs = [torch.empty(pairs * 4, dtype=torch.int32, device=dev) for _ in range(2)]       # room for tn93's tallies
    item = {da.OUT_DISTANCE: 8, da.OUT_TALLY: 4, da.OUT_TALLY16: 2}
    view = {da.OUT_DISTANCE: torch.int64, da.OUT_TALLY: torch.int32, da.OUT_TALLY16: torch.int16}
    tal_rows = {}
    # tallies first: the 16-bit rows are held to the 32-bit ones, the f64 bars take the exact value from them
    for measure, kind in sorted(c["runs"], key=lambda mk: mk[1] != da.OUT_TALLY):
        width = 1 if kind == da.OUT_DISTANCE else da.tally_width(measure)
        nbytes = pairs * width * item[kind]
        out = []
        for e, raw in zip((cons, dense), bufs):
            v = raw.view(torch.uint8)[:nbytes].view(view[kind])
            if square:
                e.run_square_device(measure, 0, n_rows, v.data_ptr(), nbytes, out_kind=kind)
            else:
                e._check(e._lib.dst_run_rect(e._h, da.MEASURES[measure], 0, 1, 0, n_rows, kind, v.data_ptr(), nbytes, None))
            out.append(v)
        torch.cuda.synchronize()
        info = cons.last_launch()
        seen = (info["family"], info["wide"], out_name(info["measure"], info["out_kind"]), info["event_waves"])
        assert info["path"] == c["path"] and info["square"] == square and info["pairs"] == pairs, (name, measure, kind, info)
        assert seen == expected_of(c, measure, kind) and info["rows_per_tile"] == c["rows"], (name, measure, kind, info)
        assert info["hot"] == (c["path"] == "hybrid") and info["run_records"] == (c.get("extra") == "runs"), (name, info)
        assert dense.last_launch()["path"] == "dense" and dense.last_launch()["event_waves"] == 0
        SEEN.setdefault(seen, set()).add(info["rows_per_tile"])
        assert torch.equal(out[0], out[1]), (name, measure, kind)            # every bit of the whole launch
        if kind == da.OUT_TALLY:
            for i in rows:
                first = da.square_row_start(n_cols, i) if square else i * n_cols
                count = n_cols - i - 1 if square else n_cols
                tal_rows.setdefault(measure, {})[i] = (out[0][first * width:(first + count) * width].cpu().numpy()
                                                       .view(np.uint32).reshape(count, width))
        tl = tal_rows.get({"jc69": "raw", "n": "n_high"}.get(measure, measure) if kind != da.OUT_TALLY else measure)
        assert tl is not None or measure in ("n", "n_high", "raw"), (name, measure, kind)     # tallies ran first
        check_rows_against_the_oracle(measure, kind, out[0], width, rows, a, b, counts_a, counts_b, tl)
    cons.set_path("auto")


def test_the_census_is_complete():
    """every instantiation of TABLE ran in this module, and each tile height with the default split for every family's
    native output (run after the cases: pytest keeps the file's order)"""
    missing = sorted(TABLE - set(SEEN))
    extra = sorted(set(SEEN) - TABLE)
    print("instantiations seen:", len(SEEN), "of", len(TABLE))
    for key in sorted(SEEN):
        print("  family %d wide %d %-7s EW %d  rows per tile %s" % (key[0], key[1], key[2], key[3], sorted(SEEN[key])))
    assert not missing and not extra, (missing, extra)
    for fam, outs in ((0, ("int",)), (1, ("raw", "jc69")), (2, ("k80",)), (3, ("tn93",))):
        for out in outs:
            assert SEEN[(fam, False, out, default_ew(out, False))] >= {8, 16, 32}, (fam, out)
