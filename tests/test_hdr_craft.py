"""The crafted Radiance .hdr corpus (tests/hdr_craft.py) proves itself on the CPU: every file
decodes, through the oracle, to the pixels its packet plan means; the restated locate rule sends it
down the path it was built for; and the restated window and scan rules put each packet and each
scanline start on the edge its row of the table names. tests/test_gpu_hdr_craft.py then holds the
kernels to the same table."""
import numpy as np
import pytest

import hdr_craft as K
import hdrutil as H
from oracle import pyoracle as O

CASES = K.cases()
BY_GROUP = {g: [c for c in CASES if c.group == g] for g in K.GROUPS}


def test_writer_codes():
    data, row = K.scanline(8, [[("lit", b""), ("run", 1, 9), ("run", 2, 8), ("run", 3, 7), ("lit", b"\x05\x06")],
                               [("lit", bytes(range(8)))], K.runs(8, 4), K.runs(8, 130)])
    assert data == bytes((2, 2, 0, 8, 0, 129, 9, 130, 8, 131, 7, 2, 5, 6, 8)) + bytes(range(8)) + bytes((136, 4, 136, 130))
    assert row[:, 0].tolist() == [9, 8, 8, 7, 7, 7, 5, 6] and row[:, 3].tolist() == [130] * 8
    data, row = K.scanline(128, [[("lit", bytes(range(128)))]] + [[("run", 127, 3), ("run", 1, 4)]] * 3)
    assert data[4] == 128 and data[5:133] == bytes(range(128)) and data[133:137] == bytes((255, 3, 129, 4))
    with pytest.raises(AssertionError):
        K.scanline(8, [[("run", 0, 1)] + K.runs(8, 1)] + [K.runs(8, 1)] * 3)
    with pytest.raises(AssertionError):
        K.scanline(8, [K.runs(7, 1)] + [K.runs(8, 1)] * 3)


def test_case_names_unique_and_groups_known():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.group for c in CASES} == set(K.GROUPS)
    assert all(0 <= c.blob_offset < 16 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_decodes_to_its_plan_on_its_path(case):
    ref, (mode, ncand) = K.expectations()[case.name]
    if case.status is not None:
        assert ref[0] == case.status
    if case.pixels is not None:
        assert ref[0] == O.HDR_OK and (ref[1], ref[2], ref[3]) == (*case.dims, case.dims[1])
        np.testing.assert_array_equal(ref[4].view(np.uint32), H.expected_floats(case.pixels).view(np.uint32))
    assert mode == case.mode, (mode, ncand)


@pytest.mark.parametrize("case", BY_GROUP["window"], ids=lambda c: c.name)
def test_window_packets_land_where_stated(case):
    f, a = case.file, case.blob_offset
    w = case.dims[0]
    seen = set()
    for m in case.aux["marks"]:
        at, which, delta = m["at"], m["which"], m["delta"]
        heads = {pos: code for pos, code, _ in K.walk_row(f, m["row_start"], w)}
        code = heads[at]  # the packet under test is a packet header of this row
        assert code == {"lit128": 128, "lit1": 1, "code0": 0, "run127": 255, "run1": 129}[m["packet"]]
        size = 2 if code > 128 else 1 + code
        ref = K.window_refills(f, m["row_start"], a)
        base, lim = ref[which - 1]
        assert (a + base) % 16 == 0 and lim == base + 4096 - 129
        assert at - lim == delta
        if delta <= 0:  # decoded out of this window, which holds the whole packet
            assert len(ref) == which or ref[which][0] > at
            assert at + size <= base + 4096
            if delta == 0 and code == 128:
                assert at + size == base + 4096  # its last byte is the window's last byte
            # (delta == 0 and a run: its value byte, at + 1, is the first byte past lim)
        else:  # this header reloads the window
            assert ref[which][0] == at - ((a + at) & 15)
            assert not any(lim < p < at for p in heads)
        seen.add((which, delta, m["packet"]))
    assert len(seen) == 40
    if case.mode == 2:
        cap = 16 * w + 64
        assert all(K.scanline_end(f, m["row_start"], w, cap) is not None for m in case.aux["marks"])
    else:  # empty-literal filler only, and every scanline longer than the link step walks
        assert all(K.scanline_end(f, m["row_start"], w, 16 * w + 64) is None for m in case.aux["marks"])
        assert all(K.scanline_end(f, m["row_start"], w) is not None for m in case.aux["marks"])


def test_window_cases_cover_every_address_residue():
    assert {c.blob_offset for c in BY_GROUP["window"] if c.mode == 2} == set(range(16))
    assert {c.blob_offset for c in BY_GROUP["window"] if c.mode == 3} == {0, 5, 10, 15}


def test_eof_cases_cross_the_file_end_at_every_residue():
    assert {len(c.file) % 16 for c in BY_GROUP["eof"]} == set(range(16))
    for c in BY_GROUP["eof"]:
        w, h, ds = K.parse_header(c.file)
        last = K.scanline_end(c.file, ds, w)
        assert K.scanline_end(c.file, last, w) == len(c.file)  # the last row ends the file
        (base, lim), = K.window_refills(c.file, last, c.blob_offset)
        assert base < len(c.file) < base + 4096


def _row_starts(f):
    w, h, ds = K.parse_header(f)
    out, p = [], ds
    for _ in range(h):
        out.append(p)
        p = K.scanline_end(f, p, w)
    return out, p, ds


def test_scan_cases_reach_every_chunk_position_and_the_tail():
    assert {(c.aux["trailing"], c.blob_offset) for c in BY_GROUP["scan"]} == {(t, o) for t in range(24) for o in range(4)}
    for c in BY_GROUP["scan"]:
        if c.blob_offset:
            continue  # the same file at another offset
        starts, end, ds = _row_starts(c.file)
        assert len(c.file) - end == c.aux["trailing"]
        assert all(12 <= b - a <= 40 for a, b in zip(starts, starts[1:] + [end]))
        assert {(s - ds) % 16 for s in starts} == set(range(16))
        tail = K.scan_tail_start(c.file)
        assert 0 < len(c.file) - tail < 24 and (tail - ds) % 16 == 0 and tail - 16 + 24 <= len(c.file)
        assert K.scan_tail_hits(c.file) >= 3
        # the false starts all sort behind the true ones: the file still links
        pats = K.pattern_positions(c.file, 8, ds)
        assert pats[:len(starts)] == starts and len(pats) >= len(starts) + 3


def test_cap_lengths_fall_on_both_sides():
    modes = {}
    for c in BY_GROUP["link"]:
        if c.name.startswith("link_cap"):
            starts, end, _ = _row_starts(c.file)
            modes[end - starts[-1] - (16 * 8 + 64)] = K.predict(c.file)[0]
    assert sorted(modes) == [-1, 0, 1, 2, 3]
    assert set(modes.values()) == {2, 3}


def test_link_counts():
    want = {"link_h1": (1, 1), "link_h2": (2, 2), "link_h3": (3, 3), "link_h1025": (1025, 1025), "link_trailing_false": (3, 4),
            "link_false_mid": (3, 4), "link_false_row0": (3, 4), "link_false_last": (3, 4), "link_h8192": (8192, 8192),
            "link_h8191_trailing": (8191, 8192), "link_h8193": (8193, 8193), "link_width_mismatch": (4, 3)}
    for c in BY_GROUP["link"]:
        if c.name in want:
            assert (c.dims[1], K.predict(c.file)[1]) == want[c.name], c.name


def test_marker_cases():
    by = {c.name: c for c in BY_GROUP["plain"]}
    for name in ("mixed_row_marker", "mixed_misaligned_flat"):
        f = by[name].file
        w, h, ds = K.parse_header(f)
        assert not K.aligned_marker(f, ds)
        row1 = K.scanline_end(f, ds, w)
        assert (row1 - ds) % 4 != 0
        groups = [f[row1 + 4 * k: row1 + 4 * k + 3] for k in range(w)]
        assert (b"\x01\x01\x01" in groups) == (name == "mixed_row_marker")
    f = by["new_with_marker"].file
    assert K.aligned_marker(f, K.parse_header(f)[2])
    f = by["plain_111_straddle"].file
    assert b"\x01\x01\x01" in f and not K.aligned_marker(f, K.parse_header(f)[2])


def test_w514_adjacent_false_start():
    by = {c.name: c for c in BY_GROUP["width"]}
    f = by["w514_lit2"].file
    pats = K.pattern_positions(f, 514, K.parse_header(f)[2])
    assert len(pats) == 4 and any(b - a == 1 for a, b in zip(pats, pats[1:]))
    f = by["w514"].file
    assert len(K.pattern_positions(f, 514, K.parse_header(f)[2])) == 3


def test_place_puts_each_file_at_its_residue():
    blob, offs, sizes = K.place(BY_GROUP["plain"])
    for c, o, s in zip(BY_GROUP["plain"], offs, sizes):
        assert o % 16 == c.blob_offset and blob[o:o + s] == c.file


# predict's (mode, ncand) for the seeded corpus of tests/hdrutil.py, recorded so that a change to
# that corpus (or to the rule) shows here. The old-style encoder only emits a run marker where
# pixels repeat, so most old_* files are in fact plain rows. rle_false_candidates is walked
# serially: its false starts sit between the true ones.
CORPUS_VALID = {
    'rle_1x3': (1, 0), 'rle_5x4': (1, 0), 'rle_7x9': (1, 0), 'rle_8x8': (2, 8), 'rle_9x5': (2, 5), 'rle_64x33': (2, 33),
    'rle_258x20': (2, 20), 'rle_1000x7': (2, 7), 'flat_1x3': (1, 0), 'flat_5x4': (1, 0), 'flat_7x9': (1, 0),
    'flat_8x8': (1, 0), 'flat_9x5': (1, 0), 'flat_64x33': (1, 0), 'flat_258x20': (1, 0), 'flat_1000x7': (1, 0),
    'old_1x3': (1, 0), 'old_5x4': (1, 0), 'old_7x9': (1, 0), 'old_8x8': (1, 0), 'old_9x5': (1, 0), 'old_64x33': (3, 0),
    'old_258x20': (3, 0), 'old_1000x7': (1, 0), 'mixed_8x12': (3, 3), 'mixed_33x17': (3, 5), 'mixed_300x9': (3, 3),
    'rle_false_candidates': (3, 18), 'old_chained_runs': (3, 0),
}
CORPUS_EDGE = {
    'empty': (0, 0), 'not_radiance': (0, 0), 'short_magic': (0, 0), 'no_blank_line': (0, 0), 'no_reso_newline': (0, 0),
    'reso_x_first': (0, 0), 'reso_only_y': (0, 0), 'reso_zero': (0, 0), 'reso_negative': (0, 0), 'reso_spaces': (1, 0),
    'reso_huge': (0, 0), 'header_only': (3, 0), 'trunc_rle_0.1': (3, 1), 'trunc_flat_0.1': (3, 0), 'trunc_old_0.1': (3, 0),
    'trunc_rle_0.5': (3, 3), 'trunc_flat_0.5': (3, 0), 'trunc_old_0.5': (3, 0), 'trunc_rle_0.97': (3, 6),
    'trunc_flat_0.97': (3, 0), 'trunc_old_0.97': (3, 0), 'trunc_flat_minus1': (3, 0), 'trunc_rle_minus1': (3, 6),
    'trunc_in_row_header': (3, 0), 'rle_run_overflow': (3, 1), 'rle_literal_overflow': (3, 1), 'old_run_first_px': (3, 0),
    'old_run_zero_first_px': (3, 0), 'old_rshift_24_zero': (3, 0), 'old_rshift_32': (3, 0), 'old_run_past_end': (3, 0),
    'rle_width_mismatch': (3, 5), 'narrow_2_2': (1, 0), 'rle_trailing': (2, 6), 'flat_trailing': (3, 0),
    'fuzz_rle_0': (2, 6), 'fuzz_rle_1': (2, 6), 'fuzz_rle_2': (2, 6), 'fuzz_rle_3': (2, 6), 'fuzz_rle_4': (2, 6),
    'fuzz_rle_5': (2, 6), 'fuzz_rle_6': (3, 5), 'fuzz_rle_7': (3, 5), 'fuzz_rle_8': (2, 6), 'fuzz_rle_9': (2, 6),
    'fuzz_rle_10': (2, 6), 'fuzz_rle_11': (3, 6),
    **{f'fuzz_flat_{k}': (1, 0) for k in range(12)}, **{f'fuzz_old_{k}': (1, 0) for k in range(12)},
}


def test_predict_on_the_seeded_corpus():
    assert {n: K.predict(f) for n, f, _ in H.valid_cases()} == CORPUS_VALID
    assert {n: K.predict(f) for n, f in H.edge_cases()} == CORPUS_EDGE


def test_parse_header_agrees_with_the_oracle():
    """predict's header walk accepts exactly the files the oracle finds a size for."""
    for n, f in H.edge_cases():
        ref = O.hdr_decode(f)
        hd = K.parse_header(f)
        assert (hd is not None) == (ref[0] in (O.HDR_OK, O.HDR_MALFORMED, O.HDR_TRUNCATED)), n
        if hd:
            assert hd[:2] == (ref[1], ref[2]), n
