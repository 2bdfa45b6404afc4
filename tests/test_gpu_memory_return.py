"""GPU (-m gpu): every owner of device and page-locked memory gives it back.

test_gpu_parity.py's create / use / close cycle covers the planes, dense runs and dst_run_slabs.  Here the same cycle for
every other owner: the buffers of a set (DeviceSet and its reference, lists, site buckets, run-record tables and hot
columns), of a stream's slots, and of the calls that allocate for themselves.  One warm cycle, a reading of the device's
free memory, 20 more cycles, a second reading: the two differ by less than 64 MiB (that test's bound and its way of
reading).  Every family's shapes are chosen from the sizes in dst_api.cpp / dst_stream.cpp / dst_analysis.cpp so that the
buffers it is about total 4 MiB or more per cycle (the figures are in each docstring): lost once per cycle they pass the
bound within 20 cycles.  Buffers far below that (the 16 bytes of runs.state, a reference's statistics, the run masks, the
few KB of a stream's bad-code words) cannot be seen this way: for them the guarantee is that the library's sources name
hipMalloc / hipFree / hipHostMalloc / hipHostFree in one owner type only (Grown, dst_owner.h), which frees what it holds.
"""
import numpy as np
import pytest

import distance_amd as da
from helpers import random_alignment

pytestmark = pytest.mark.gpu

BOUND = 64 << 20
CYCLES = 20


def quiet_alignment(n, L, seed):
    """about 2.5 % of the sites differ from the plurality sequence: lists are worth it (below kListsMaxDeviation)"""
    return random_alignment(n, L, seed, p_ambig=0.005, p_gap=0.005, divergence=0.02)


def fused_engine():
    """the consensus path with its preparation riding on the upload (reference, list lengths and slots from the pack)"""
    e = da.Engine(0)
    e.set_prep_threshold(0.0)
    e.set_path("consensus")
    return e


def assert_memory_returns(cycle):
    import torch
    torch.cuda.init()
    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(CYCLES):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f"free before {free0}, after {free1}, difference {free0 - free1}")
    assert abs(free0 - free1) < BOUND, (free0, free1)


def test_lists_from_the_pack():
    """2,000 x 8,192, square, lists from the pack's slots: slots 2.6 MB, about 0.5 M entries = 2 MB of lists and 2 MB of
    overflow room, the lookup table 0.26 MB, the pack's counters, range marks and A-constants 0.2 MB: 7 MB a cycle
    beside the 21 MB of planes"""
    codes = quiet_alignment(2000, 8192, 61)

    def cycle():
        e = fused_engine()
        e.upload(0, codes)
        e.run_square("raw", 0, 64)
        assert e.last_path() == "consensus" and not e.planes_stored(0)
        e.run_square("tn93", 0, 64)      # (another family: the A-constants again)
        e.close()

    assert_memory_returns(cycle)


def test_run_records_then_a_rectangle():
    """1,500 x 8,192 with 100 records half N (32 run chunks each): the entries' a-words 16 bytes per entry = 4.5 MB, the
    correction tables and their transposes 0.6 MB per word and the 7-bit sums 0.5 MB per word, beside masks, known sites
    and panel starts; then a second file against slot 0, which drops the stripping and rebuilds the lists from the
    planes (2 x 2.5 MB: the runs' sites are entries again)"""
    codes = quiet_alignment(1500, 8192, 62)
    codes[::15, 2048:6144] = 240
    other = quiet_alignment(200, 8192, 63)

    def cycle():
        e = fused_engine()
        e.upload(0, codes)
        e.run_square("raw", 0, 64)
        assert e.run_records()[0] == 100
        e.run_square("tn93", 0, 64)
        e.upload(1, other)
        e.run_rect("k80", 1, 0)
        assert e.last_path() == "consensus" and e.run_records()[0] == 0
        e.close()

    assert_memory_returns(cycle)


def test_hybrid_path_forced():
    """4,000 x 8,192 with every sixth column clade-like (a tenth of the records share G there: about 1,100 hot sites = 9
    chunks): the hot columns as a set of their own 8 x 9 x 4,608 x 16 B = 5.3 MB of planes, beside the hot tallies of 128
    rows x 4,000 columns"""
    n = 4000
    codes = quiet_alignment(n, 8192, 64)
    codes[: n // 10, ::6] = 72

    def cycle():
        e = fused_engine()
        e.upload(0, codes)
        e.set_path("hybrid")
        e.run_square("raw", 0, 128)
        assert e.last_path() == "hybrid"
        e.close()

    assert_memory_returns(cycle)


def test_reupload_larger_then_smaller():
    """one context: 600 x 4,000 (4 MB of planes), then 1,200 x 8,000 (12 MB: the set is freed whole, lists and all, and
    starts over), then 600 x 4,000 again (the larger buffers stay); lists built every time"""
    small, big = quiet_alignment(600, 4000, 65), quiet_alignment(1200, 8000, 66)

    def cycle():
        e = fused_engine()
        for codes in (small, big, small):
            e.upload(0, codes)
            e.run_square("k80", 0, 32)
            assert e.last_path() == "consensus"
        e.close()

    assert_memory_returns(cycle)


def test_failed_upload_then_close():
    """1,000 x 8,192 with one invalid code byte: 10.5 MB of planes, 1.5 MB of slots and the reference are there when the
    upload fails; close frees them"""
    codes = quiet_alignment(1000, 8192, 67)
    codes[700, 5000] = 1

    def cycle():
        e = fused_engine()
        with pytest.raises(da.DistanceError) as err:
            e.upload(0, codes)
        assert "record 700 at site 5000" in str(err.value)
        e.close()

    assert_memory_returns(cycle)


def test_streams_open_feed_close():
    """600 x 4,096 loaded; four streams of 3 slots x 256 records, each fed one batch: a slot holds 1 MB of page-locked and
    1 MB of device input, its results (1.2 MB of distances on the device, and page-locked for the plain stream; 2.5 MB of
    tallies on the device otherwise), 2 MB of planes, and the lists or the links window of its kind: over 15 MB a
    stream"""
    loaded = quiet_alignment(600, 4096, 68)
    batch = quiet_alignment(256, 4096, 69)

    def cycle():
        e = da.Engine(0)
        e.upload(0, loaded)
        with e.stream("tn93", 256) as s:
            s.push(batch)
            assert s.pop().shape == (256, 600)
        for side in ("loaded", "streamed"):
            with e.closest_stream("raw", 8, 256, side=side) as s:
                s.push(batch)
                s.pop()
                if side == "loaded":
                    assert s.result()[0].shape == (600, 8)
        with e.links_stream("raw", 0.05, 256, tallies=True) as s:
            s.push(batch)
            assert s.pop()[0] == 256
        e.close()

    assert_memory_returns(cycle)


def test_calls_that_allocate_for_themselves():
    """800 x 4,096: the square of nj, of each bootstrap tree and of the dendrogram 5.1 MB (nj: and 2.9 MB for its
    compaction), the bootstrap's two code matrices 3.3 MB each and its replicate's set 6.3 MB of planes.  Then 48 x 360,000:
    consensus() counts into 12 bytes per site = 4.3 MB, differences() lists about 0.9 M sites = 3.5 MB"""
    codes = quiet_alignment(800, 4096, 70)
    wide = quiet_alignment(48, 360_000, 71)
    other = wide[0].copy()

    def cycle():
        e = da.Engine(0)
        e.upload(0, codes)
        parent, _ = e.nj("raw")
        e.nj_bootstrap("raw", codes, parent, 3)
        e.dendrogram("raw")
        e.upload(0, wide)
        assert e.consensus().shape == (360_000,)
        assert len(e.differences(0, other)) == 48
        e.close()

    assert_memory_returns(cycle)
