"""GPU (-m gpu): a result depends on the bytes inside the rows, on all of them, and on nothing else — the three kernels
that turn bytes into bit planes (pack_kernel / pack_chunk, pack_stream_kernel, pack_nibbles_kernel) on the designed cases
of ingest_edge_cases.py: the row's end at every position of a last word on both sides of a chunk's edge, every offset and
stride residue of a device upload, 255 / 256 / 257 records, and every byte that is no row hostile: 0x00 (a read past a
row must raise) or seeded known bases (a read past a row moves tallies and base counts).  Everything is held to the oracle
on the row bytes alone: tallies of every measure and n / n_high / raw bit for bit, tn93 (device-counted base counts: the
counts kernel reads the planes the pack wrote) within test_gpu_stream.py's 1e-12, base counts exactly; every planted
invalid byte is named exactly, the hostile bytes around it never."""
import contextlib
import functools

import numpy as np
import pytest

import distance_amd as da
import ingest_edge_cases as ic
import oracle

pytestmark = pytest.mark.gpu
SETTINGS = (("dense", None), ("auto", 0.0))      # pack_kernel with nothing asked of it; lists wanted and planes deferred
PREP_DEFAULT = 2.0e10


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def setting(eng, path, prep):
    eng.set_path(path)
    if prep is not None:
        eng.set_prep_threshold(prep)
    try:
        yield
    finally:
        eng.set_path("auto")
        eng.set_prep_threshold(PREP_DEFAULT)


# ---- the oracle, once per case ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def stream_reference(L, n):
    """[streamed][loaded]: tallies of every measure, distances, as the oracle has them from the rows alone"""
    rows, loaded = ic.case_rows(L, n), ic.loaded_set(L)
    tl = {m: oracle.tallies_rect(m, rows, loaded, threads=8) for m in ic.ALL}
    d = {m: oracle.all_pairs_rect(m, loaded, rows, threads=8).T for m in ic.DISTANCES}
    return tl, d


@functools.lru_cache(maxsize=8)
def square_reference(L, n):
    codes = ic.case_rows(L, n)
    iu = np.triu_indices(n, 1)
    tl = {m: oracle.tallies_rect(m, codes, codes, threads=8)[iu] for m in ic.ALL}
    d = {m: oracle.all_pairs_square(m, codes, threads=8) for m in ic.DISTANCES}
    return tl, d, oracle.count_bases_matrix(codes)


def same_distance(m, got, want):
    if m in da.INT_MEASURES:
        return got.dtype == np.int64 and np.array_equal(got, want.astype(np.int64))
    if m == "raw":      # one correctly rounded division: the oracle's bits (NaN for NaN)
        num = ~np.isnan(want)
        return np.array_equal(np.isnan(got), ~num) and np.array_equal(got[num].view(np.uint64), want[num].view(np.uint64))
    return bool(np.isclose(got, want, rtol=0, atol=1e-12, equal_nan=True).all())


def check_square(eng, L, n, what):
    """slot 0 against the oracle: base counts, and every pair's tallies and distances"""
    tl, d, counts = square_reference(L, n)
    assert eng.set_info(0) == (n, L), what
    if n >= 2:
        for m in ic.ALL:
            got = eng.run_square(m, tallies=True)
            assert got.shape == tl[m].shape and np.array_equal(got.astype(np.uint64), tl[m]), ("tallies", m) + what
        for m in ic.DISTANCES:
            assert same_distance(m, eng.run_square(m), d[m]), ("distance", m) + what
    assert np.array_equal(eng.base_counts(0).astype(np.uint64), counts), ("base counts",) + what


def prime(eng, fill, n, pitch, seed):
    """leave hostile bytes in the staging buffer's row tails: an upload of n rows, pitch wide, of known bases — or of 0x00,
    which is refused and stays in the buffer all the same"""
    if fill == "valid":
        eng.upload(0, ic.primer(n, pitch, seed))
    else:
        with pytest.raises(da.DistanceError):
            eng.upload(0, np.zeros((n, pitch), np.uint8))


def expect_named(call, plant, L, what):
    r, s = ic.named(plant, L)
    with pytest.raises(da.DistanceError) as e:
        call()
    assert e.value.status == 3 and f"record {r} at site {s} " in e.value.message, (e.value.message, plant) + what


# ---- the stream: code bytes and nibbles through the slot's full-pitch view -------------------------------------------
STREAM_CASES = [(wire, L) for wire in ic.WIRES for L in ic.widths(wire)]


def load(eng, L):
    """the loaded set in slot 0, behind a primer: its row tails in the staging buffer are known bases too"""
    loaded = ic.loaded_set(L)
    prime(eng, "valid", ic.N_LOADED, ic.pitch_of(L), L)
    eng.upload(0, loaded)
    assert np.array_equal(eng.base_counts(0).astype(np.uint64), oracle.count_bases_matrix(loaded)), L


def slot_images(L, wire, counts, cap, rows_of):
    """the whole (cap, pitch) slot for every (fill, batch size): hostile tails, hostile records behind the batch"""
    out = {}
    for fill in ic.FILLS:
        for n in counts:
            img = np.empty((cap, ic.pitch_of(L, wire)), np.uint8)
            ic.hostile_slot(img, rows_of(fill, n), fill, L, wire)
            out[fill, n] = img
    return out


@pytest.mark.parametrize("wire,L", STREAM_CASES)
def test_streamed_batches_depend_on_their_rows_alone(eng, wire, L):
    load(eng, L)
    counts = ic.batch_counts(L)
    cap = max(counts) + 1
    images = slot_images(L, wire, counts, cap, lambda fill, n: ic.to_wire(ic.case_rows(L, n), wire, ic.pad_nibble(fill, L)))
    for m, tallies in [(m, True) for m in ic.ALL] + [(m, False) for m in ic.DISTANCES]:
        with eng.stream(m, max_records=cap, depth=2, tallies=tallies, nibbles=wire == "nibbles") as st:
            for (fill, n), img in images.items():
                buf, _ = st.buffer(padded=True)
                assert buf.shape == img.shape, (buf.shape, img.shape)
                buf[...] = img
                st.submit(n)
                got = st.pop()                    # (the invalid fill raises nothing)
                tl, d = stream_reference(L, n)
                if tallies:
                    assert got.shape == tl[m].shape and np.array_equal(got.astype(np.uint64), tl[m]), (m, fill, n)
                else:
                    assert got.shape == d[m].shape and same_distance(m, got, d[m]), (m, fill, n)


@pytest.mark.parametrize("wire,L", STREAM_CASES)
def test_streamed_invalid_sites_are_named_exactly(eng, wire, L):
    load(eng, L)
    counts = (3,) + ((ic.BLOCK + 1,) if L in ic.BLOCK_EDGE_WIDTHS else ())
    cap = max(counts) + 1
    with eng.stream("raw", max_records=cap, depth=2, nibbles=wire == "nibbles") as st:
        for fill in ic.FILLS:
            for n in counts:
                for plant in ic.plants(L, n, wire):
                    buf, _ = st.buffer(padded=True)
                    ic.hostile_slot(buf, ic.planted(ic.case_rows(L, n), plant, wire, ic.pad_nibble(fill, L)), fill, L, wire)
                    st.submit(n)
                    expect_named(st.pop, plant, L, (wire, fill, n))
        # and the stream is fine afterwards
        st.push(ic.case_rows(L, 3))
        assert same_distance("raw", st.pop(), stream_reference(L, 3)[1]["raw"])


# ---- Engine.upload from a strided numpy view: the staging buffer's row tails hold the upload before -------------------
@pytest.mark.parametrize("L", ic.CODE_WIDTHS)
def test_host_uploads_depend_on_their_rows_alone(eng, L):
    pitch = ic.pitch_of(L)
    for n in ic.batch_counts(L):
        codes = ic.case_rows(L, n)
        for path, prep in SETTINGS:
            with setting(eng, path, prep):
                for k, fill in enumerate(ic.FILLS):
                    offset, stride = ic.layouts(L)[(5 * k + L) % 16]
                    _, view = ic.hostile_buffer(codes, offset, stride, fill, L)
                    prime(eng, fill, n, pitch, L)
                    eng.upload(0, view)
                    check_square(eng, L, n, (path, fill, n))


@pytest.mark.parametrize("L", ic.CODE_WIDTHS)
def test_host_upload_invalid_sites_are_named_exactly(eng, L):
    for n in (3,) + ((ic.BLOCK + 1,) if L in ic.BLOCK_EDGE_WIDTHS else ()):
        codes = ic.case_rows(L, n)
        for path, prep in SETTINGS:
            with setting(eng, path, prep):
                for fill in ic.FILLS:
                    prime(eng, fill, n, ic.pitch_of(L), L)
                    for plant in ic.plants(L, n):
                        bad = ic.planted(codes, plant, "codes")
                        expect_named(lambda: eng.upload(0, bad), plant, L, (path, fill, n))
                eng.upload(0, codes)
                check_square(eng, L, n, (path, "after", n))


# ---- Engine.upload_device from a torch byte buffer: every (offset, stride) -------------------------------------------
def to_device(torch, buf):
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    return d


@pytest.mark.parametrize("n", ic.DEVICE_COUNTS)
@pytest.mark.parametrize("L", ic.DEVICE_WIDTHS)
def test_device_uploads_depend_on_their_rows_alone(eng, L, n):
    torch = pytest.importorskip("torch")
    codes = ic.case_rows(L, n)
    for k, (offset, stride) in enumerate(ic.layouts(L)):
        for fill in ic.FILLS:
            buf, _ = ic.hostile_buffer(codes, offset, stride, fill, k)
            d = to_device(torch, buf)
            for path, prep in SETTINGS:
                with setting(eng, path, prep):
                    eng.upload_device(0, d.data_ptr() + offset, n, L, stride)
                    check_square(eng, L, n, (path, fill, offset, stride))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", (3, ic.BLOCK + 1))
@pytest.mark.parametrize("L", ic.DEVICE_WIDTHS)
def test_device_upload_invalid_sites_are_named_exactly(eng, L, n):
    torch = pytest.importorskip("torch")
    codes = ic.case_rows(L, n)
    lay = ic.layouts(L)
    for k, plant in enumerate(ic.plants(L, n)):
        bad = ic.planted(codes, plant, "codes")
        for j, fill in enumerate(ic.FILLS):
            offset, stride = lay[(2 * k + j) % len(lay)]
            buf, _ = ic.hostile_buffer(bad, offset, stride, fill, k)
            d = to_device(torch, buf)
            for path, prep in SETTINGS:
                with setting(eng, path, prep):
                    expect_named(lambda: eng.upload_device(0, d.data_ptr() + offset, n, L, stride), plant, L,
                                 (path, fill, offset, stride))
    torch.cuda.synchronize()
