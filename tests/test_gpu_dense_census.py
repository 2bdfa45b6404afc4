"""GPU (-m gpu): a census of pair_kernel<M, BM, TN, MINW, OUT> (dst_kernels.hip), the dense bit-plane kernel the rest of
the suite compares everything else with.

dense_census_cases.py holds the designed sets, the job shapes and the table of (family, rows per tile, output) built
from the library's own variant tables; test_dense_census_host.py checks without a GPU that the shapes have the partial
tiles, diagonal tiles and partial panels they are there for and that neighbouring slots hold different values.  Here, for
every (measure, tile variant):
  a. every output form (the measure's distance, 32-bit and 16-bit tallies) on every job shape — whole square, three row
     ranges, both rectangles whole and in part — against the oracle: tallies, n / n_high exactly, raw bit for bit,
     jc69 / k80 / tn93 within test_gpu_finalise_accuracy's bars of the exact value (helpers.check_f64; the few pairs
     with a logarithm's argument of exactly 0 within CLOSE_ULP of the reference's bits) AND bitwise
     equal to dst_finalize_device of the oracle's tallies (another kernel; the header's contract);
  b. launches split 2, 4 and 7 ways over L (the tally_add and int_add outputs, the scratch buffer and finalize_kernel):
     bitwise the unsplit results, and held to the oracle as in (a);
  c. the launch report after every launch: dense, this variant, plan_tiles' tile shape and tile count, the split factor;
  d. the automatic split on 70 x 2,049;  e. variants out of range;
  f. the hybrid path's hot launch per variant (16-bit hot tallies, and 32-bit ones on 65,600 sites);
  g. every output form into a device buffer of exactly the job's size between two guard bands, which keep their fill.
The closing test holds the instantiations seen against the table of 50.
"""
import numpy as np
import pytest

import dense_census_cases as dc
import distance_amd as da
from helpers import check_f64

pytestmark = pytest.mark.gpu
KIND = {"distance": da.OUT_DISTANCE, "tally": da.OUT_TALLY, "tally16": da.OUT_TALLY16}
SEEN = {}      # (family, rows per tile, out) -> the cases it was seen in
FIN = {}       # (measure, shape name) -> dst_finalize_device of the oracle's tallies


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    e.set_path("dense")
    e.upload(0, dc.codes_of("A"))
    e.upload(1, dc.codes_of("B"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_c():
    e = da.Engine(0)
    e.set_path("dense")
    e.upload(0, dc.codes_of("C"))
    yield e
    e.close()


@pytest.fixture(scope="module")
def hyb():
    e = da.Engine(0)
    e.set_prep_threshold(0)
    e.set_path("hybrid")
    yield e
    e.close()


def launch(e, measure, shape, kind):
    """one launch into host memory: (pairs[, width]) in the job's output order, and its report"""
    kw = dict(tallies=kind == "tally", tallies16=kind == "tally16")
    if shape["square"]:
        out = e.run_square(measure, shape["rb"], shape["re"], **kw)
    else:
        out = e.run_rect(measure, dc.SLOT[shape["rows"]], dc.SLOT[shape["cols"]], shape["rb"], shape["re"], **kw)
        out = out.reshape((-1,) + out.shape[2:])
    return out, e.last_launch()


def instantiation(measure, kind, ksplit):
    """the output launch_outputs instantiates for this launch"""
    if ksplit > 1:
        return "int_add" if kind == "distance" and dc.FAMILY[measure] == 0 else "tally_add"
    return dc.NATIVE[measure] if kind == "distance" else kind


def check_report(li, measure, variant, shape, kind, ksplit):
    """(c): a dense launch of this variant, with plan_tiles' tile shape and count and the expected split factor"""
    tiles, bm, bn = dc.plan(shape, measure, variant)
    want = dict(path="dense", measure=measure, family=dc.FAMILY[measure], variant=variant, rows_per_tile=bm, tile_cols=bn,
                tiles=len(tiles), square=shape["square"], out_kind=KIND[kind], ksplit=ksplit, pairs=len(dc.pairs_of(shape)[0]),
                event_waves=0, hot=False)
    assert {k: li[k] for k in want} == want, (measure, variant, kind, li)
    return (dc.FAMILY[measure], bm, instantiation(measure, kind, ksplit))


def finalized(e, measure, name, shape):
    """dst_finalize_device of the oracle's tallies of the job (finalize_kernel: not the epilogue under test)"""
    import torch
    if (measure, name) not in FIN:
        dev = torch.device("cuda", e.device)
        tl = np.ascontiguousarray(dc.want_tallies(measure, shape).astype(np.uint32))
        d_t = torch.from_numpy(tl).to(dev)
        d_o = torch.empty(len(tl), dtype=torch.float64, device=dev)
        e.finalize_device(measure, shape["rb"], shape["re"], d_t.data_ptr(), d_o.data_ptr(), d_o.numel() * 8, tally_kind=da.OUT_TALLY,
                          square=shape["square"], row_slot=dc.SLOT[shape["rows"]], col_slot=dc.SLOT[shape["cols"]])
        torch.cuda.synchronize()
        FIN[(measure, name)] = d_o.cpu().numpy()
    return FIN[(measure, name)]


def check_values(e, measure, name, shape, kind, got):
    """(a): one launch's output against the oracle"""
    want_t = dc.want_tallies(measure, shape)
    where = (measure, name, kind)
    assert len(got) == len(want_t) and len(got) > 0, where
    if kind != "distance":
        assert got.dtype == (np.uint16 if kind == "tally16" else np.uint32) and got.shape == want_t.shape, where
        assert np.array_equal(got.astype(np.uint64), want_t), where
        return
    want = dc.want_distances(measure, shape)
    if measure in da.INT_MEASURES:
        assert got.dtype == np.int64 and np.array_equal(got, want.astype(np.int64)), where
        return
    assert got.dtype == np.float64
    fin = finalized(e, measure, name, shape)
    if measure == "raw":         # one correctly rounded division: the reference's bits (a NaN is a NaN)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), where
        assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), where
    else:
        import finalise_reference as fr
        from test_gpu_finalise_accuracy import CLOSE_ULP
        ex, sing = dc.want_exact(measure, shape), dc.singular(measure, shape)
        keep = ~sing
        check_f64(measure, got[keep], want[keep], want_t[keep], None, None,
                  ex=fr.Exact(ex.value[keep], ex.scale[keep], ex.e[keep], ex.k[keep]))
        # a logarithm's argument of exactly 0 (dense_census_cases.singular): the reference's bits, as past the series
        nan = np.isnan(want[sing])
        assert np.array_equal(np.isnan(got[sing]), nan), where
        ulp = np.abs(got[sing][~nan].view(np.int64) - want[sing][~nan].view(np.int64))
        assert (ulp <= CLOSE_ULP[measure]).all(), (where, int(ulp.max()))
    # NaN, +-inf and -0.0 included: the bits of the other kernel
    assert np.array_equal(got.view(np.uint64), fin.view(np.uint64)), where


def saw(key, case):
    SEEN.setdefault(key, []).append(case)


@pytest.mark.parametrize("measure,variant", dc.variants())
def test_every_output_on_every_job_shape(eng, measure, variant):
    eng.set_ksplit(0)
    eng.set_variant(variant)
    try:
        for name, shape in dc.SHAPES.items():
            for kind in ("tally", "tally16", "distance"):
                got, li = launch(eng, measure, shape, kind)
                key = check_report(li, measure, variant, shape, kind, 1)
                check_values(eng, measure, name, shape, kind, got)
                saw(key, f"{measure} v{variant} {name} {kind}")
    finally:
        eng.set_variant(0)


@pytest.mark.parametrize("measure,variant", dc.variants())
def test_split_launches_are_the_single_sweep(eng, measure, variant):
    eng.set_variant(variant)
    try:
        for name in dc.SPLIT_SHAPES:
            shape = dc.SHAPES[name]
            eng.set_ksplit(1)
            one = {kind: launch(eng, measure, shape, kind)[0] for kind in ("distance", "tally", "tally16")}
            for k in dc.FORCED:
                eng.set_ksplit(k)
                for kind in ("distance", "tally"):
                    got, li = launch(eng, measure, shape, kind)
                    key = check_report(li, measure, variant, shape, kind, dc.forced_ksplit(k, shape))
                    assert got.dtype == one[kind].dtype, (measure, variant, name, k, kind)
                    assert np.array_equal(got.view(np.uint64 if kind == "distance" else np.uint32),
                                          one[kind].view(np.uint64 if kind == "distance" else np.uint32)), (measure, variant, name, k, kind)
                    check_values(eng, measure, name, shape, kind, got)
                    saw(key, f"{measure} v{variant} {name} k={k} {kind}")
                got, li = launch(eng, measure, shape, "tally16")       # no 16-bit atomics: one sweep, whatever is forced
                key = check_report(li, measure, variant, shape, "tally16", 1)
                assert np.array_equal(got, one["tally16"]), (measure, variant, name, k)
                saw(key, f"{measure} v{variant} {name} k={k} tally16")
    finally:
        eng.set_ksplit(0)
        eng.set_variant(0)


@pytest.mark.parametrize("measure", dc.ALL)
def test_automatic_split(eng_c, measure):
    """70 x 2,049: 17 chunks and a handful of tiles, which the library splits 2 ways by itself"""
    shape = dc.AUTO_SPLIT
    eng_c.set_ksplit(0)
    try:
        for variant in sorted({0, dc.tallest_variant(measure)}):
            eng_c.set_variant(variant)
            for kind in ("tally", "distance", "tally16"):
                got, li = launch(eng_c, measure, shape, kind)
                key = check_report(li, measure, variant, shape, kind, 1 if kind == "tally16" else 2)
                check_values(eng_c, measure, "auto_split", shape, kind, got)
                saw(key, f"{measure} v{variant} auto_split {kind}")
    finally:
        eng_c.set_variant(0)


@pytest.mark.parametrize("measure", dc.ALL)
def test_variants_out_of_range_run_as_variant_0(eng, measure):
    """dst_set_variant takes any variant >= 0, and one the measure does not have runs as variant 0; a negative one is
    refused (DST_ERR_ARG) and leaves the context at the variant it had"""
    shape = dc.SHAPES["square_37_150"]
    eng.set_ksplit(0)
    count = dc.variant_count(measure)
    try:
        eng.set_variant(count)
        for kind in ("tally", "distance"):
            got, li = launch(eng, measure, shape, kind)
            check_report(li, measure, 0, shape, kind, 1)
            check_values(eng, measure, "square_37_150", shape, kind, got)
        eng.set_variant(0)
        with pytest.raises(da.DistanceError) as err:
            eng.set_variant(-1)
        assert err.value.status == 1
        got, li = launch(eng, measure, shape, "distance")
        check_report(li, measure, 0, shape, "distance", 1)
        check_values(eng, measure, "square_37_150", shape, "distance", got)
    finally:
        eng.set_variant(0)


@pytest.mark.parametrize("measure,variant", dc.variants())
def test_hybrid_hot_launches(hyb, measure, variant):
    """the dense kernel on the hot planes: DST_OUT_TALLY16 below 65,536 sites, DST_OUT_TALLY from there, with the
    context's variant"""
    bm = dc.tile_of(measure, variant)[0]
    hyb.set_variant(variant)
    try:
        loaded = None
        for name, shape in dc.HYBRID_SHAPES.items():
            if loaded != shape["rows"]:
                loaded = shape["rows"]
                hyb.upload(0, dc.codes_of(loaded))
                if loaded == "H":
                    hyb.upload(1, dc.codes_of("H40"))
            for kind in ("tally", "distance"):
                got, li = launch(hyb, measure, shape, kind)
                assert li["path"] == "hybrid" and li["hot"] == 1 and li["measure"] == measure, (measure, variant, name, kind, li)
                assert li["square"] == shape["square"] and li["wide"] == dc.hot_is_wide(name) and li["tiles"] > 0, (name, li)
                check_values(hyb, measure, name, shape, kind, got)
            saw((dc.FAMILY[measure], bm, "tally" if dc.hot_is_wide(name) else "tally16"), f"{measure} v{variant} {name} hot launch")
    finally:
        hyb.set_variant(0)


GUARD = 1 << 16       # bytes either side of a device buffer: more than a row of any job's output (771 x 16 bytes)


@pytest.mark.parametrize("measure,variant", dc.variants())
def test_nothing_is_written_outside_the_output(eng, measure, variant):
    """every output form, whole and split 4 ways, into a device buffer of exactly the job's size between two guard bands:
    the bands keep their fill (a row past row_end, or a column past the last, would land there), and the buffer holds
    what the host-buffer form returned"""
    import torch
    dev = torch.device("cuda", eng.device)
    item = {"distance": 8, "tally": 4 * da.tally_width(measure), "tally16": 2 * da.tally_width(measure)}
    eng.set_variant(variant)
    try:
        for name, shape in dc.SHAPES.items():
            pairs = len(dc.pairs_of(shape)[0])
            for k in (1, 4):
                eng.set_ksplit(k)
                for kind in ("distance", "tally", "tally16"):
                    want, _ = launch(eng, measure, shape, kind)
                    need = pairs * item[kind]
                    room = -(-need // 16) * 16                   # (the guard behind starts on a 16-byte boundary at the latest)
                    buf = torch.full((GUARD + room + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()         # (the fill runs on torch's stream, the launch on the context's own)
                    ptr = buf.data_ptr() + GUARD
                    if shape["square"]:
                        eng.run_square_device(measure, shape["rb"], shape["re"], ptr, need, out_kind=KIND[kind])
                    else:
                        eng.run_rect_device(measure, dc.SLOT[shape["rows"]], dc.SLOT[shape["cols"]], shape["rb"], shape["re"], ptr, need,
                                            out_kind=KIND[kind])
                    torch.cuda.synchronize()
                    li = eng.last_launch()
                    key = check_report(li, measure, variant, shape, kind, 1 if kind == "tally16" else dc.forced_ksplit(k, shape))
                    host = buf.cpu().numpy()
                    where = (measure, variant, name, k, kind)
                    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), where
                    assert host[GUARD:GUARD + need].tobytes() == want.tobytes(), where
                    saw(key, f"{measure} v{variant} {name} k={k} {kind} between guard bands")
    finally:
        eng.set_ksplit(0)
        eng.set_variant(0)


def test_the_dense_census_is_complete():
    """every instantiation of the table ran in this module (run after the cases: pytest keeps the file's order)"""
    table = dc.build_table()
    assert len(table) == dc.EXPECTED_INSTANTIATIONS, sorted(table)
    print("dense instantiations seen:", len(set(SEEN) & table), "of", len(table))
    for key in sorted(SEEN):
        print("  family %d  %2d rows  %-9s %4d launches, e.g. %s" % (key + (len(SEEN[key]), SEEN[key][0])))
    assert set(SEEN) == table, (sorted(table - set(SEEN)), sorted(set(SEEN) - table))
