"""No GPU: the ingest edge cases (ingest_edge_cases.py) held to themselves and to the oracle — the rows come back out of
every hostile buffer, the case list reaches every position of the kernels' last words on every load path, and the cases can
fail: what a wrong mask would read changes the oracle's answer for the case."""
import itertools

import numpy as np
import pytest

import distance_amd as da
import ingest_edge_cases as ic
import oracle
from helpers import CODES


def test_the_rows_come_back_out_of_every_hostile_buffer_and_the_rest_is_fill():
    for L, n, fill in itertools.product(ic.DEVICE_WIDTHS, (1, 3), ic.FILLS):
        codes = ic.case_rows(L, n)
        for k, (offset, stride) in enumerate(ic.layouts(L)):
            buf, view = ic.hostile_buffer(codes, offset, stride, fill, k)
            assert np.array_equal(view, codes)
            cut = np.stack([buf[offset + r * stride:offset + r * stride + L] for r in range(n)])
            assert np.array_equal(cut, codes), (L, n, offset, stride)
            mask = ic.row_mask(n, L, offset, stride, buf.size)
            assert mask.sum() == n * L
            rest = buf[~mask]
            assert np.array_equal(rest, ic.fill_bytes(fill, buf.size, k)[~mask])
            assert (rest == 0).all() if fill == "invalid" else np.isin(rest, ic.KNOWN).all()
            assert buf.size - (offset + (n - 1) * stride + L) == ic.SLACK


def test_valid_fill_differs_from_row_to_row():
    for wire in ic.WIRES:
        tails = ic.fill_bytes("valid", (257, 128), 5, wire)
        assert len({t.tobytes() for t in tails}) == 257
        assert not np.array_equal(ic.fill_bytes("valid", (4, 128), 5, wire), ic.fill_bytes("valid", (4, 128), 6, wire))
    assert np.isin(ic.fill_bytes("valid", 4096, 1, "nibbles") & 15, ic.BASE_NIBBLES).all()
    assert np.isin(ic.fill_bytes("valid", 4096, 1, "nibbles") >> 4, ic.BASE_NIBBLES).all()


def test_a_stream_slot_is_hostile_around_the_batch():
    for wire, fill, L in itertools.product(ic.WIRES, ic.FILLS, (1, 7, 129, 257)):
        codes = ic.case_rows(L, 3)
        rows = ic.to_wire(codes, wire, ic.pad_nibble(fill, L))
        slot = np.full((5, ic.pitch_of(L, wire)), 0xAA, np.uint8)
        ic.hostile_slot(slot, rows, fill, L, wire)
        assert np.array_equal(slot[:3, :rows.shape[1]], rows)
        want = ic.fill_bytes(fill, slot.shape, L, wire)
        assert np.array_equal(slot[:3, rows.shape[1]:], want[:3, rows.shape[1]:]) and np.array_equal(slot[3:], want[3:])
        assert slot.shape[1] > rows.shape[1], "no tail to fill"


def test_the_widths_have_the_residues_the_design_claims():
    below = lambda L: L % ic.CHUNK >= ic.CHUNK - 8          # noqa: E731   the 8 sites before a multiple of 128
    above = lambda L: 1 <= L % ic.CHUNK <= 8                # noqa: E731   the 8 behind it (and the multiple itself: 0)
    for side in (below, above):
        assert {L % 8 for L in ic.WIDTHS if side(L) and L > 8} == set(range(8)), side
        assert {L % 4 for L in ic.WIDTHS if side(L) and L > 8} == set(range(4)), side
        assert {L % 4 for L in ic.DEVICE_WIDTHS if side(L) and L > 8} == set(range(4)), side
    assert set(range(1, 18)) <= set(ic.WIDTHS) and {127, 128, 129, 255, 256, 257, 384} <= set(ic.WIDTHS)
    assert set(ic.BLOCK_EDGE_WIDTHS) <= set(ic.WIDTHS) and ic.BLOCK_EDGE_COUNTS == (ic.BLOCK - 1, ic.BLOCK, ic.BLOCK + 1)
    assert {1023, 1024, 1025, 1026, 1027, 1039} <= set(ic.CODE_WIDTHS) and set(ic.WIDTHS) <= set(ic.CODE_WIDTHS)
    assert {L % 4 for L in ic.CODE_WIDTHS if L >= 1023} == set(range(4))
    assert max(ic.DEVICE_COUNTS) == ic.BLOCK + 1 and set(ic.FILLS) == {"invalid", "valid"}


def test_every_offset_and_stride_residue_pair_occurs():
    for L in ic.DEVICE_WIDTHS:
        lay = ic.layouts(L)
        assert {(o % 4, s % 4) for o, s in lay} == set(itertools.product(range(4), range(4))), L
        assert {4, 8, 16} <= {o for o, _ in lay}
        assert all(s >= L for _, s in lay) and (0, L) in lay
        assert any(o % 16 == 0 and s % 16 == 0 and s > L for o, s in lay), L            # every row on a 16-byte boundary
        assert any(o % 16 == 0 and s % 16 == 1 for o, s in lay), L                      # ... missed by one


def test_the_nibble_wire_decodes_to_the_codes_high_nibbles():
    for L in ic.WIDTHS:
        codes = ic.case_rows(L, 3)
        for pad in (0, 15) + ic.BASE_NIBBLES:
            w = ic.to_wire(codes, "nibbles", pad)
            assert w.shape == (3, (L + 1) // 2)
            assert np.array_equal(ic.from_nibbles(w, L), codes >> 4), (L, pad)
            assert np.array_equal(w, da.engine.Stream.to_nibbles(codes, pad)), (L, pad)     # the engine's encoder: the same bytes
            if L % 2:
                assert (w[:, -1] >> 4 == pad).all()
        assert np.array_equal(da.engine.Stream.to_nibbles(codes), ic.to_wire(codes, "nibbles", 15))


def test_the_case_list_reaches_every_keep_on_every_path():
    # the nibble wire: keep = 0..7 sites of the row's last word, with both pad nibbles (both fills run at every width)
    keeps = set()
    for L in ic.WIDTHS:
        keeps |= ic.last_word_keeps(L, 8)
    assert keeps == set(range(8))
    assert {L % 8 for L in ic.WIDTHS if L % 2} == {1, 3, 5, 7}                              # the lone low nibble at each
    assert {ic.pad_nibble(f, L) == 0 for f in ic.FILLS for L in ic.WIDTHS} == {True, False}
    # the stream's code wire and the staging buffer of a host upload: rows on 128-byte boundaries
    seen = {}
    for L in ic.CODE_WIDTHS:
        for n in ic.batch_counts(L):
            for path, k in ic.code_keeps_by_path(0, ic.pitch_of(L), n, L).items():
                seen.setdefault(path, set()).update(k)
    assert seen["words"] == set(range(4)) and seen["bytes"] == set(range(4)), seen
    # device uploads: every layout
    seen, paths = {}, set()
    for L in ic.DEVICE_WIDTHS:
        for n in ic.DEVICE_COUNTS:
            for offset, stride in ic.layouts(L):
                for path, k in ic.code_keeps_by_path(offset, stride, n, L).items():
                    seen.setdefault(path, set()).update(k)
                paths |= {ic.code_load_path(offset, stride, n, L, s, c) for s in (0, 1, n - 1) if s < n
                          for c in range((L + ic.CHUNK - 1) // ic.CHUNK)}
    assert seen["words"] == set(range(4)) and seen["bytes"] == set(range(4)), seen
    assert paths == {"fast", "words", "bytes"}
    # the first chunk of a matrix off a 4-byte boundary is read by bytes, whatever follows
    assert ic.code_load_path(2, 1031, 3, 1000, 0, 0) == "bytes" and ic.code_load_path(2, 1031, 3, 1000, 0, 1) == "words"
    # the three block-edge record counts, on every wire
    assert all(set(ic.BLOCK_EDGE_COUNTS) <= set(ic.batch_counts(L)) for L in ic.BLOCK_EDGE_WIDTHS)
    assert ic.BLOCK + 1 in ic.DEVICE_COUNTS


def test_plants_name_the_smallest_record_and_site():
    for wire in ic.WIRES:
        for L, n in ((1, 1), (1, 257), (7, 3), (129, 3), (257, 257)):
            ps = ic.plants(L, n, wire)
            flat = {p for plant in ps for p in plant}
            assert {(0, 0), (n - 1, L - 1)} <= flat
            if L > ic.CHUNK:
                assert {s for _, s in flat} >= {ic.CHUNK - 1, ic.CHUNK}
            if n > ic.BLOCK:
                assert {r for r, _ in flat} >= {ic.BLOCK - 1, ic.BLOCK}
            if n * L > 1:
                assert any(len(p) == 2 for p in ps)
            codes = ic.case_rows(L, n)
            for plant in ps:
                r, s = ic.named(plant, L)
                assert all(r * L + s <= a * L + b for a, b in plant)
                w = ic.planted(codes, plant, wire, pad=8)
                if wire == "codes":
                    bad = ~np.isin(w, CODES)
                else:
                    bad = ic.from_nibbles(w, L) == 0
                assert sorted(zip(*np.nonzero(bad))) == sorted(set(plant)), (wire, L, n, plant)


# ---- the tests can fail -------------------------------------------------------------------------------------------
def pair_tallies(a, b):
    return oracle.tallies_rect("raw", a, b), oracle.tallies_rect("tn93", a, b)


def differs(true, wrong):
    return any(not np.array_equal(t, w) for t, w in zip(true, wrong))


def picked(n):
    """the records the condition is shown on: the first two and the last (whose tail is fill in every layout)"""
    return sorted({0, min(1, n - 1), n - 1})


def square_failures(codes, tails, uptos):
    """extensions of the rows that leave the base counts, or (n >= 2) every picked pair's tallies, as they were"""
    n, L = codes.shape
    rows = picked(n)
    true = pair_tallies(codes[rows], codes[rows])
    out = []
    for upto in sorted(set(uptos) - {L}):
        wrong = ic.extend(codes, tails, upto)[rows]
        if np.array_equal(oracle.count_bases_matrix(wrong), oracle.count_bases_matrix(codes[rows])):
            out.append(("counts", upto))
        if n >= 2 and not differs(true, pair_tallies(wrong, wrong)):
            out.append(("tallies", upto))
    return out


def device_failures(L, n):
    """valid fill: the rows extended by what a missing word mask (4 bytes) or a missing length check (the chunk) would read
    give other tallies (n >= 2) and other base counts (every n), in every layout"""
    codes = ic.case_rows(L, n)
    out = []
    for k, (offset, stride) in enumerate(ic.layouts(L)):
        buf, _ = ic.hostile_buffer(codes, offset, stride, "valid", k)
        tails = ic.buffer_tails(buf, n, L, offset, stride)
        out += [(offset, stride) + f for f in square_failures(codes, tails, (ic.round_up(L, 4), ic.round_up(L, ic.CHUNK)))]
    return out


def host_failures(L, n):
    """the staging buffer's row tails hold the primer's known bases"""
    pitch = ic.pitch_of(L)
    return square_failures(ic.case_rows(L, n), ic.primer(n, pitch, L)[:, L:], (ic.round_up(L, 4), pitch))


def stream_failures(wire, L, n):
    """A streamed row read past its end meets the loaded set there.  Where the loaded set is read past its end too (its
    staging tails hold a primer's bases: a missing word mask reads up to a multiple of 4 sites, a missing length check
    the chunk), the pair tallies move.  Where only the batch is (the nibble mask alone at L = 4 mod 8: N in the loaded set
    takes the site out of every tally), its device-counted base counts move, and with them a finite tn93 distance by more
    than the comparison's 1e-12."""
    word = 4 if wire == "codes" else 8
    loaded = ic.loaded_set(L)
    ltails = ic.primer(ic.N_LOADED, ic.pitch_of(L), L)[:, L:]
    codes = ic.case_rows(L, n)
    rows = picked(n)
    slot = np.zeros((n + 1, ic.pitch_of(L, wire)), np.uint8)
    ic.hostile_slot(slot, ic.to_wire(codes, wire, ic.pad_nibble("valid", L)), "valid", L, wire)
    tails = slot[:n, L:] if wire == "codes" else ic.nibble_tail_codes(slot[:n], L)
    assert np.isin(tails, ic.KNOWN).all()
    true = pair_tallies(codes[rows], loaded)
    true_counts = oracle.count_bases_matrix(codes[rows])
    out = []
    for upto, lupto in {(ic.round_up(L, word), ic.round_up(L, 4)), (ic.round_up(L, ic.CHUNK), ic.round_up(L, ic.CHUNK))}:
        if upto == L:
            continue
        wrong = ic.extend(codes, tails, upto)[rows]
        counts = oracle.count_bases_matrix(wrong)
        if np.array_equal(counts, true_counts):
            out.append(("counts", upto))
        if lupto > L:       # both sides read past the end, the loaded set up to lupto
            wl = ic.extend(loaded, ltails, lupto)
            if not differs(true, pair_tallies(wrong[:, :lupto], wl)):
                out.append(("tallies", upto))
        else:               # the batch alone
            lcounts = oracle.count_bases_matrix(loaded)
            d_true = oracle.all_pairs_rect("tn93", loaded, codes[rows], lcounts, true_counts)
            d_wrong = oracle.all_pairs_rect("tn93", loaded, codes[rows], lcounts, counts)
            if np.isclose(d_true, d_wrong, rtol=0, atol=1e-12, equal_nan=True).all():
                out.append(("tn93", upto))
    return out


HINT = "choose another seed for these rows in ingest_edge_cases.SEEDS"


@pytest.mark.parametrize("L", ic.DEVICE_WIDTHS)
def test_a_wrong_mask_changes_the_answer_of_every_device_upload_case(L):
    for n in ic.DEVICE_COUNTS:
        assert device_failures(L, n) == [], (L, n, HINT)


@pytest.mark.parametrize("L", ic.CODE_WIDTHS)
def test_a_wrong_mask_changes_the_answer_of_every_host_upload_case(L):
    for n in ic.batch_counts(L):
        assert host_failures(L, n) == [], (L, n, HINT)


@pytest.mark.parametrize("wire", ic.WIRES)
def test_a_wrong_mask_changes_the_answer_of_every_stream_case(wire):
    for L in ic.widths(wire):
        for n in ic.batch_counts(L):
            assert stream_failures(wire, L, n) == [], (wire, L, n, HINT)
