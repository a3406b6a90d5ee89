"""The crafted JPEG decoder inputs (tests/jpegdec_craft.py) reach the gates they are named after.

CPU only. The reach conditions below are conditions on the INPUTS, read from the oracle's trace of
each file (quantized cells and absolute DC per block) and the file's own tables; they never read
the code under test. tests/test_gpu_decode_craft.py then compares the GPU decoder with the oracle
on exactly these files, so a state listed here is a state that comparison exercises. The oracle is
pinned to the reference decoder on every file where the reference build is present, and the
host-compiled lane emulator (tests/test_gw2_emu.py) must agree with the oracle's trace on every
entropy-family stream: what is left for the GPU test to guard is the device code.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
import jpegdec_craft as J
import test_gw2_emu as E

_A = {}


def files():
    """{name: (bytes, analyse())} for streams() and the IDCT families at the other samplings."""
    if not _A:
        every = J.streams()
        for sampling in ("444", "422", "gray"):
            every.update(J.idct_streams(sampling))
        for n, d in every.items():
            _A[n] = (d, J.analyse(d, O.decode_trace))
    return _A


def _q0(a, ci=0):
    return int(a["hd"]["qt"][a["hd"]["comps"][ci][2]][0])


def _uniform_q(a):
    return {int(v) for c in a["hd"]["comps"] for v in a["hd"]["qt"][c[2]]}


def _block_extremes(a):
    """Per block the dequantized value of largest magnitude, signed, and its natural position."""
    d = a["deq"]
    pos = np.abs(d).argmax(1)
    return [(int(d[i, p]), int(p)) for i, p in enumerate(pos)]


def reach_failures(drop_family=None):
    """Names of the reach conditions that the crafted set (without drop_family) misses."""
    fs = {n: a for n, (d, a) in files().items() if J.family(n) != drop_family}
    main = {n: a for n, a in fs.items() if n in J.streams()}  # the batch of the mode runs
    fails = []

    def need(name, ok):
        if not ok:
            fails.append(name)

    # ---- entropy side ----
    ac_vals = set()
    for a in main.values():
        ac_vals |= {int(v) for v in np.unique(a["coef"])}
    need("both ends of AC categories 11 .. 15, both signs", set(J.cat_values()) <= ac_vals)
    for sub in (1, 3):
        tot = {t for a in main.values() if len(a["hd"]["comps"]) == sub for row in a["tots"] for _s, t in row}
        need(f"code + magnitude totals 29, 30 and 31, {sub} components", {29, 30, 31} <= tot)
    shifts = set()
    for a in main.values():  # after a 3-bit symbol: second totals 15 (paired), 16 and 18 (refused)
        seen = {row[k + 1][1] for row in a["tots"] for k in range(len(row) - 1) if row[k][1] == 3}
        if {15, 16, 18} <= seen:
            shifts.add(J.CJ._category(int(a["diffs"][0])))
    need("pair totals 15 / 16 / 18 behind every shift of 1 .. 8 bits", set(range(1, 9)) <= shifts)
    wide, nibble = set(), set()
    for a in main.values():
        d = {int(v) for v in a["diffs"]}
        wide |= d
        if any(s > 15 for s in a["hd"]["huff"][("dc", 0)]):
            nibble |= {J.CJ._category(v) for v in d}
    need("DC differences +-32767, +-16384, +-8191, +-2048",
         {sg * v for v in (32767, 16384, 8191, 2048) for sg in (1, -1)} <= wide)
    need("DC symbols with a high nibble, sizes 12, 13 and 15", {12, 13, 15} <= nibble)
    for q in (1, 255):
        dcs, first, last, mid = set(), False, False, False
        for a in main.values():
            if len(a["hd"]["comps"]) != 3 or _q0(a) != q:
                continue
            hit = np.isin(a["dc"], J.DC_ESCAPE_VALUES)
            dcs |= {int(v) for v in a["dc"][hit]}
            if len({int(v) for v in a["dc"][hit]}) == 10:
                per_row = a["n"] // ((a["hd"]["h"] + 15) // 16)
                idx = np.nonzero(hit)[0]
                first |= bool((idx < 24).any())
                last |= bool((idx >= a["n"] - per_row).any())
                mid |= bool(((idx >= per_row) & (idx < a["n"] - per_row)).any())
        need(f"absolute DC -32770 .. -32766 and 32766 .. 32770, q[0] = {q}", set(J.DC_ESCAPE_VALUES) <= dcs)
        need(f"the DC walk at the start, in the middle and in the last MCU row, q[0] = {q}", first and last and mid)
    need("a DC product past 2^31", any(int(np.abs(a["deq"][:, 0]).max()) >= 1 << 31 for a in main.values()))
    for sub in (1, 3):
        dense = [a for a in main.values() if len(a["hd"]["comps"]) == sub and a["ff00"] >= 0.95]
        need(f"FF 00 share of 0.95 or more, valid, {sub} components", any(a["code"] == 0 for a in dense))
    need("an FF-dense scan that ends behind a lone FF", any(a["code"] != 0 and a["ff00"] >= 0.95 for a in main.values()))
    need("an FF-dense scan with an early EOI that decodes",
         any(a["code"] == 0 and a["ff00"] >= 0.95 and len(a["hd"]["scan"]) < 3 * np.count_nonzero(a["coef"]) for a in main.values()))
    need("eight streams refused inside a photographic-density scan",
         sum(1 for a in main.values() if a["code"] != 0 and a["ff00"] < 0.5) >= 8)

    # ---- back half ----
    for sampling, group in (("420", main), ("other", {n: a for n, a in fs.items() if n not in main})):
        by_q = {}
        for a in group.values():
            q = _uniform_q(a)
            if len(q) == 1:
                by_q.setdefault(q.pop(), []).extend(_block_extremes(a))
        for q in (1, 128, 129):
            ex = by_q.get(q, [])
            want = {(sg * v, p) for v in (16383, 16384) if v % q == 0 for sg in (1, -1)
                    for p in (0, 1, 8, 63, 28)}
            need(f"block extremes +-16383 / +-16384 at DC, (0,1), (1,0), (7,7), (3,4); q = {q}; {sampling}",
                 want <= set(ex))
        signs = set()
        for a in group.values():
            full = (np.abs(a["deq"]) == 16383).all(1)
            signs |= {tuple(r) for r in np.sign(a["deq"][full])}
        need(f"65 sign patterns of 64 values of magnitude 16383; {sampling}", len(signs) >= 65)
        g22 = set()
        colgate, pairs, exempt, full_wrap, shl_wrap = set(), set(), set(), False, False
        for a in group.values():
            d = a["deq"].reshape(-1, 8, 8)
            for v in (4194240, 4194495, -4194240, -4194495):
                for blk, r, c in zip(*np.nonzero(d == v)):
                    if np.count_nonzero(d[blk]) == 1:
                        g22.add((v, int(c)))
                    elif np.count_nonzero(d[blk]) == 2 and abs(v) == 4194240:
                        pairs.add((v, tuple(int(x) for x in np.nonzero(d[blk, r])[0])))
            big = np.abs(d) >= 1 << 22
            exempt |= {int(c) for blk, r, c in zip(*np.nonzero(big)) if np.count_nonzero(d[blk]) <= 2 and c in (0, 4)}
            small = np.abs(d).reshape(len(d), -1).max(1) < 1 << 22
            rows = J.row_pass(d[small])
            for blk, r, c in zip(*np.nonzero(np.abs(rows) >= 1 << 22)):
                if r:
                    colgate.add(int(r))
            full_wrap |= bool((np.abs(d).reshape(len(d), -1) == 32767 * 255).all(1).any())
            shl_wrap |= bool(((d[:, :, 0] << 11) != J._w32(d[:, :, 0] << 11)).any())
        need(f"+-16448 * 255 and +-16449 * 255 alone in slots 1, 2, 3, 5, 6, 7; {sampling}",
             {(v, c) for v in (4194240, 4194495, -4194240, -4194495) for c in (1, 2, 3, 5, 6, 7)} <= g22)
        need(f"the summed pairs (1,7), (3,5), (2,6) at +-16448 * 255; {sampling}",
             {(v, p) for v in (4194240, -4194240) for p in ((1, 7), (3, 5), (2, 6))} <= pairs)
        need(f"values past 2^22 in the exempt slots 0 and 4; {sampling}", {0, 4} <= exempt)
        need(f"row outputs past 2^22 from inputs below it, rows 1, 2, 3, 5, 6, 7; {sampling}",
             {1, 2, 3, 5, 6, 7} <= colgate)
        need(f"r[0] << 11 wraps; {sampling}", shl_wrap)
        need(f"64 values of +-32767 * 255; {sampling}", full_wrap)
        dense = sum(int((np.count_nonzero(a["deq"], 1) >= 60).sum()) for a in group.values() if len(_uniform_q(a)) >= 50)
        need(f"200 dense blocks under per-position quantisers; {sampling}", dense >= 200)
        px, ycc = set(), set()
        for a in group.values():
            if _uniform_q(a) != {1}:
                continue
            flat = ~a["coef"].any(1)
            px |= {((int(v) + 32) >> 6) + 128 for v in a["dc"][flat]}
            nc = len(a["hd"]["comps"])
            if flat.all() and nc == 3:
                per = [c[0] * c[1] for c in a["hd"]["comps"]]
                m = a["dc"].reshape(-1, sum(per))
                for row in m:
                    if len(set(row[:per[0]])) == 1:
                        ycc.add(tuple(((int(v) + 32) >> 6) + 128 for v in (row[0], row[per[0]], row[per[0] + per[1]])))
        need(f"DC-only pixels -2 .. 257; {sampling}", set(range(-2, 258)) <= px)
        need(f"the corners of the YCbCr cube; {sampling}", set(J.YCC) <= ycc)
    wide = [a for a in main.values() if a["hd"]["w"] == 536 and len(a["hd"]["comps"]) == 3]
    ok = False
    for a in wide:  # luma block row 0 in raster order: neighbours on opposite sides of 2^14
        ex = np.abs(a["deq"]).max(1)
        row0 = [ex[6 * m + s] for m in range(34) for s in (0, 1)]
        ok |= all((row0[i] >= 1 << 14) != (row0[i + 1] >= 1 << 14) for i in range(len(row0) - 1))
    need("a 536-wide 4:2:0 block row that alternates across 2^14", ok)
    return fails


def test_crafted_set_reaches_the_gates():
    assert reach_failures() == []


@pytest.mark.parametrize("fam", J.FAMILIES)
def test_every_family_is_needed(fam):
    """Without any one family at least one reach condition fails: the conditions bind."""
    assert reach_failures(drop_family=fam) != []


def test_magnitude_histogram(capsys):
    """The histogram of magnitude sizes per family (the table in DESIGN.md is this output): the
    entropy families cover AC 11 .. 15 and DC 12 .. 15, which no other test's input does."""
    hist = {}
    for n, (d, a) in files().items():
        if n not in J.streams():
            continue
        h = hist.setdefault(J.family(n), [np.zeros(16, int), np.zeros(17, int)])
        for v in a["coef"][a["coef"] != 0]:
            h[0][J.CJ._category(int(v))] += 1
        for v in a["diffs"]:
            h[1][min(16, J.CJ._category(int(v)))] += 1
    with capsys.disabled():
        print("\n| family | AC sizes 1-10 | 11 | 12 | 13 | 14 | 15 | DC sizes 0-11 | 12 | 13 | 14 | 15 |\n|---|---|---|---|---|---|---|---|---|---|---|---|")
        for f in J.FAMILIES:
            ac, dc = hist[f]
            print(f"| {f} | {ac[:11].sum()} | " + " | ".join(str(x) for x in ac[11:]) + f" | {dc[:12].sum()} | "
                  + " | ".join(str(x) for x in dc[12:16]) + " |")
    assert all(h[1][16] == 0 for h in hist.values())  # (no DC difference the format cannot hold)
    ac = sum(hist[f][0] for f in J.ENTROPY)
    dc = sum(hist[f][1] for f in J.ENTROPY)
    assert (ac[11:] > 0).all() and (dc[12:16] > 0).all()


def test_oracle_status():
    """Status 0 for every stream but the two error kinds, which the oracle refuses."""
    for n, (d, a) in files().items():
        code, w, h, nc, pix = O.decode(d)
        assert (code != 0) == n.startswith(J.ERRORS), (n, code)
        if code == 0:
            assert (w, h) == (a["hd"]["w"], a["hd"]["h"]) and len(pix) == w * h * nc, n
        assert len(d) < 256 * 1024 and w <= 536 and h <= 256, n


def test_oracle_matches_reference():
    """The oracle is a restatement; at these extremes it had never been compared with NanoJPEG."""
    if not O.ref_available():
        pytest.skip("the reference build (oracle/_ref) is not present")
    for n, (d, _) in files().items():
        got, want = O.decode(d), O.ref_decode(d)
        assert got[0] == want[0], (n, got[0], want[0])
        if want[0] == 0:
            assert got == want, n


def test_lane_emulator_agrees():
    """Both write-loop schedules of the host-compiled lanes equal the oracle's trace on every
    entropy-family stream (check() asserts it); the error and pair cases fall where they should."""
    stats = {n: E.check(d) for n, (d, _) in files().items() if J.family(n) in J.ENTROPY}
    assert all(s is not None for s in stats.values())
    pos = sorted(s["errpos"] for n, s in stats.items() if J.family(n) == "ac_run_size0")
    assert len(pos) == 8 and pos[0] == 1 and pos[-1] == 2, pos
    for n, s in stats.items():
        if J.family(n) == "pair_tot15":
            assert s["lookups"] - s["iters"] > 0 and s["by_bits"] > 0, (n, s)
        if not n.startswith(J.ERRORS):
            assert s["errpos"] == 0 and s["errblk"] == -1, (n, s)
