"""Crafted baseline JPEG streams for the decoder's numeric gates -- TEST HELPER, not a test.

The entropy side has field widths that photographic input never fills (icx_step.h: a 5-bit tot1
whose maximum 31 is a 16-bit code plus 15 magnitude bits, a pair's second symbol refused past a
total of 15, run extension up to 31 bits; icx_spec_core.h: extend_mag's mask, write_decode's bit
field extracts; icx_internal.h: the int16 DC cell and its escape value), and the back half has
branches that only coefficients no pixel encoder writes can reach (block_transform's 2^14 gate,
idct_fast_ok's 2^22 gate, 32-bit wrap-around, both clip ends). NanoJPEG decodes all of it
deterministically (njGetVLC takes `value & 15` magnitude bits and never bounds a coefficient), so
the oracle's pixels are the reference.

    streams() -> {"<family>__<variant>": bytes}      everything, the IDCT families at 4:2:0
    idct_streams(sampling) -> {...}                  the IDCT families at "444" / "422" / "gray"
    family(name), ENTROPY, IDCT, FAMILIES, ERRORS

Built from seeded numpy through tools/coefjpeg.py (coefficient arrays) and gw2_craft.stream()
(symbol by symbol); nothing is read from disk. Every file stays under 256 KiB, so ICX_GW=1 cuts it
into 512-byte lanes.
"""
from __future__ import annotations

import math

import numpy as np

from tools import coefjpeg as CJ
import gw2_craft as G
from jpegenc_craft import DEZIGZAG

NAT2ZZ = np.argsort(DEZIGZAG)  # zig-zag position of each natural (row-major) index

ENTROPY = ("cat_edges", "pair_tot15", "dc_wide", "dc_escape", "ff_dense", "ac_run_size0")
IDCT = ("gate14", "fast14_worst", "gate22", "wrap32", "random16", "dc_clip", "ycc_corners")
FAMILIES = ENTROPY + IDCT
# variants NanoJPEG refuses (name prefixes): a size-0 AC symbol that is neither EOB nor ZRL
# (jpeg_dec.h:667), and data that ends behind a lone FF
ERRORS = ("ac_run_size0__", "ff_dense__cutff")


def family(name: str) -> str:
    return name.split("__")[0]


def zz(r: int, c: int) -> int:
    """Zig-zag position of the coefficient in row r, column c."""
    return int(NAT2ZZ[8 * r + c])


def block(cells: dict | None = None, dc: int = 0) -> np.ndarray:
    """A zig-zag block from {(row, column): value}."""
    b = np.zeros(64, np.int64)
    b[0] = dc
    for (r, c), v in (cells or {}).items():
        b[zz(r, c)] = v
    return b


# ------------------------------------------------------------------ coefficient-array files
def _scan_order(w, h, comps):
    """Per component the (by, bx) of its blocks in scan order."""
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mbw, mbh = (w + 8 * hmax - 1) // (8 * hmax), (h + 8 * vmax - 1) // (8 * vmax)
    out = [[] for _ in comps]
    for _m, ci, by, bx in CJ._mcu_blocks(comps, mbw, mbh):
        out[ci].append((by, bx))
    return out


def capacity(w, h, sampling):
    """Blocks of a list that pack() places in the luma plane AND in a chroma plane."""
    order = _scan_order(w, h, CJ.sampling_comps(sampling))
    return len(order[0]) if len(order) == 1 else min(len(order[0]), len(order[1]) + len(order[2]))


def pack(w, h, sampling, qt, blocks, bridge=True):
    """A file whose components each walk the list `blocks` (zig-zag arrays, absolute DC at 0) in
    scan order: luma and Cb from its start, Cr from where Cb stopped, all cyclically -- so with
    len(blocks) <= capacity() every block goes through the luma code and through the chroma code.
    A DC step NanoJPEG's 15 magnitude bits cannot hold gets an all-zero block in between (`bridge`;
    without it such a step is an error of the caller's)."""
    comps = CJ.sampling_comps(sampling)
    order = _scan_order(w, h, comps)
    arr = CJ.empty_blocks(w, h, comps)
    n = len(blocks)
    for ci, cells in enumerate(order):
        k = len(order[1]) % n if ci == 2 else 0
        pred = 0
        for by, bx in cells:
            b = blocks[k % n]
            if abs(int(b[0]) - pred) > 32767:
                assert bridge, "DC step beyond 15 bits"
                pred = 0
                continue
            arr[ci][by, bx] = b
            pred = int(b[0])
            k += 1
    return CJ.write(w, h, comps, qt, arr, huff="optimal")


def _uniform_q(q):
    return {0: [q] * 64, 1: [q] * 64}


def _files(out, fam, sampling, blocks, qt, w=64, h=48, tag=""):
    """The list in as many w x h files as capacity() asks for."""
    per = capacity(w, h, sampling)
    for i in range(0, len(blocks), per):
        out[f"{fam}__{sampling}{tag}_{i // per}"] = pack(w, h, sampling, qt, blocks[i:i + per])


def _noise(rng, b, amp=50, n=10):
    pos = rng.choice(np.arange(1, 64), n, replace=False)
    free = pos[b[pos] == 0]
    b[free] = rng.integers(1, amp + 1, len(free)) * rng.choice([-1, 1], len(free))
    return b


GATE14_POS = ((0, 0), (0, 1), (1, 0), (7, 7), (3, 4))


def gate14_blocks(rng, below, above):
    """Blocks whose largest magnitude is +below, +above, -below, -above in turn (neighbours of a
    block row on opposite sides of block_transform's gate), carried at DC and at four AC
    positions, the rest of the block empty or small noise."""
    out = []
    for pos in GATE14_POS:
        for noisy in (False, True):
            for v in (below, above, -below, -above):
                b = block(dc=v) if pos == (0, 0) else block({pos: v}, dc=int(rng.integers(-20, 21)) if noisy else 0)
                out.append(_noise(rng, b) if noisy else b)
    return out


def _cos_sign(n, k):
    return 1 if math.cos((2 * n + 1) * k * math.pi / 16) > 0 else -1


def fast14_blocks(mag=16383):
    """All 64 values of magnitude `mag`. Block (n, m): the sign of the coefficient in row j, column
    i is sign(cos((2n+1) i pi/16)) sign(cos((2m+1) j pi/16)), so every term of the row pass adds at
    output n and every term of the column pass at output m: the largest intermediates the fast
    path can see. Block (0, 0) is all plus and block (7, 7) the checkerboard; all minus follows."""
    out = []
    for m in range(8):
        for n in range(8):
            out.append(block({(j, i): mag * _cos_sign(n, i) * _cos_sign(m, j) for j in range(8) for i in range(8)}))
    assert (out[0] > 0).all() and all(out[63][zz(j, i)] == mag * (-1) ** (i + j) for j in range(8) for i in range(8))
    out.append(block({(j, i): -mag for j in range(8) for i in range(8)}))
    return out


GATE22_BELOW, GATE22_ABOVE = 16448, 16449  # x 255: 4,194,240 < 2^22 <= 4,194,495


def gate22_blocks():
    """Cells for q = 255 around idct_fast_ok's 2^22 (the gate looks at slots 1, 2, 3, 5, 6, 7 of a
    row or column)."""
    out = []
    for s in (1, 2, 3, 5, 6, 7):  # one gated slot of a row, both sides, both signs
        for v in (GATE22_BELOW, GATE22_ABOVE, -GATE22_BELOW, -GATE22_ABOVE):
            out.append(block({(s % 4, s): v}))
    for a, b in ((1, 7), (5, 3), (2, 6)):  # the pairs idct_row sums: the largest 24-bit operand
        for sg in (1, -1):
            out.append(block({(2, a): sg * GATE22_BELOW, (2, b): sg * GATE22_BELOW}))
    for v in (GATE22_ABOVE, 32767):  # slots 0 and 4 are exempt and must still be exact
        for sg in (1, -1):
            out.append(block({(1, 0): sg * v}))
            out.append(block({(1, 4): sg * v}))
            out.append(block({(1, 0): sg * v, (1, 4): -sg * v}))
    for r in (1, 2, 3, 5, 6, 7):  # the column gate: inputs below 2^22, row outputs past it
        for v in (2000, 8000, -2000, -8000):
            out.append(block({(r, 0): v, (r, 1): v, (r, 2): v, (r, 3): v}))
    return out


def wrap32_blocks(rng):
    """+-32767 (x 255) at 1, 2, 8 and 64 positions: r[0] << 11 and the W products wrap."""
    big = 32767
    out = []
    for pos in ((0, 0), (0, 1), (1, 0), (7, 7), (4, 4)):
        for sg in (1, -1):
            out.append(block(dc=sg * big) if pos == (0, 0) else block({pos: sg * big}))
    for p1, p2 in (((0, 0), (0, 1)), ((2, 0), (2, 4)), ((1, 1), (6, 6))):
        for s1, s2 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            cells = {p1: s1 * big, p2: s2 * big}
            dc = cells.pop((0, 0), 0)
            out.append(block(cells, dc=dc))
    lines = [[(0, i) for i in range(8)], [(3, i) for i in range(8)], [(j, 0) for j in range(8)],
             [(j, 5) for j in range(8)], [(i, i) for i in range(8)]]
    for line in lines:
        for _ in range(2):
            cells = {p: big * int(rng.choice([-1, 1])) for p in line}
            dc = cells.pop((0, 0), 0)
            out.append(block(cells, dc=dc))
    every = [(j, i) for j in range(8) for i in range(8)]
    signs = [lambda j, i: 1, lambda j, i: -1, lambda j, i: 1 if (i + j) % 2 == 0 else -1]
    signs += [None] * 3
    for f in signs:
        cells = {(j, i): big * (f(j, i) if f else int(rng.choice([-1, 1]))) for j, i in every}
        dc = cells.pop((0, 0))
        out.append(block(cells, dc=dc))
    return out


def random16_blocks(rng, n):
    """Uniform coefficients -32767 .. 32767; the DC is a clamped random walk (a DC difference has
    at most 15 magnitude bits)."""
    out = []
    dc = 0
    for _ in range(n):
        b = rng.integers(-32767, 32768, 64).astype(np.int64)
        dc = int(rng.integers(max(-32767, dc - 32767), min(32767, dc + 32767) + 1))
        b[0] = dc
        out.append(b)
    return out


def dc_clip_blocks():
    """DC-only blocks (q = 1) whose pixel ((v + 32) >> 6) + 128 takes every value -2 .. 257, both
    ends of the bucket next to the clip limits."""
    out = []
    for t in range(-2, 258):
        lo = 64 * (t - 128) - 32
        out.append(block(dc=lo))
        if t in (-2, -1, 0, 1, 254, 255, 256, 257):
            out.append(block(dc=lo + 63))
    return out


YCC = [(y, cb, cr) for y in (0, 255) for cb in (0, 255) for cr in (0, 255)] + [(128, 128, 128), (255, 0, 128), (0, 255, 128)]


def _dc_for(p):
    return 64 * (p - 128)  # ((v + 32) >> 6) + 128 == p


def ycc_corners_file(sampling, w=64, h=48):
    """DC-only MCUs (q = 1), each one (Y, Cb, Cr) of YCC: the colour conversion's corners."""
    comps = CJ.sampling_comps(sampling)
    order = _scan_order(w, h, comps)
    arr = CJ.empty_blocks(w, h, comps)
    nmcu = len(order[-1])
    for ci, cells in enumerate(order):
        per = len(cells) // nmcu
        for k, (by, bx) in enumerate(cells):
            arr[ci][by, bx, 0] = _dc_for(YCC[(k // per) % len(YCC)][ci])
    return CJ.write(w, h, comps, _uniform_q(1), arr, huff="optimal")


def _random_qt(rng):
    return {0: [int(x) for x in rng.integers(1, 256, 64)], 1: [int(x) for x in rng.integers(1, 256, 64)]}


def _idct_into(out, sampling, wide):
    """The IDCT families at one sampling. `wide`: the 536-wide gate14 case (4:2:0: plane_units'
    64-block units get a full wave, a clamped tail and lanes on both sides of the gate)."""
    rng = np.random.default_rng(20261)
    g = gate14_blocks(rng, 16383, 16384)
    if wide:
        out[f"gate14__{sampling}_536x32_q1"] = pack(536, 32, sampling, _uniform_q(1), g, bridge=False)
    else:
        _files(out, "gate14", sampling, g, _uniform_q(1), 96, 64, "_q1")
    # the gate is on the product, not the cell: 128 * 128 = 16384, 127 * 129 = 16383
    _files(out, "gate14", sampling, gate14_blocks(rng, 127, 128), _uniform_q(128), 96, 64, "_q128")
    _files(out, "gate14", sampling, gate14_blocks(rng, 127, 128), _uniform_q(129), 96, 64, "_q129")
    # the same sign patterns just past the gate and at the cell's limit
    above = [b for m in (16384, 32767) for b in (fast14_blocks(m)[k] for k in (0, 9, 18, 27, 36, 45, 54, 63, 64))]
    _files(out, "gate14", sampling, above, _uniform_q(1), 96, 64, "_above")
    _files(out, "fast14_worst", sampling, fast14_blocks(), _uniform_q(1))
    _files(out, "gate22", sampling, gate22_blocks(), _uniform_q(255))
    _files(out, "wrap32", sampling, wrap32_blocks(rng), _uniform_q(255))
    rb = random16_blocks(rng, 200)
    per = capacity(64, 48, sampling)
    for i in range(0, 200, per):
        out[f"random16__{sampling}_{i // per}"] = pack(64, 48, sampling, _random_qt(rng), rb[i:i + per])
    _files(out, "dc_clip", sampling, dc_clip_blocks(), _uniform_q(1), 128, 80)
    out[f"ycc_corners__{sampling}"] = ycc_corners_file(sampling)


def idct_streams(sampling):
    out = {}
    _idct_into(out, sampling, wide=False)
    return out


# ------------------------------------------------------------------ entropy families
def cat_values():
    """+-2^(s-1) and +-(2^s - 1): both ends of each magnitude category 11 .. 15."""
    return [sg * v for s in range(11, 16) for v in (1 << (s - 1), (1 << s) - 1) for sg in (1, -1)]


# 0x0D, 0x0E, 0x0F, 0x1F, 0x2E behind 16-bit codes: tot1 = 29, 30, 31, 31, 30
SKEW_SYMS = [0x00, 0x01, 0x02, 0x03, 0x11, 0xF0, 0x0B, 0x0D, 0x0E, 0x0F, 0x1F, 0x2E]


def _cat_edges(out, rng):
    vals = cat_values()
    for sampling in ("420", "gray"):
        comps = CJ.sampling_comps(sampling)
        arr = CJ.empty_blocks(64, 64, comps)
        k = 0
        for a in arr:
            a[..., 0] = rng.integers(-300, 301, a.shape[:2])
            for by in range(a.shape[0]):
                for bx in range(a.shape[1]):
                    pos = rng.choice(np.arange(1, 64), int(rng.integers(3, 9)), replace=False)
                    for p in pos:
                        a[by, bx, p] = vals[k % len(vals)]
                        k += 1
        out[f"cat_edges__opt_{sampling}"] = CJ.write(64, 64, comps, G.QT, arr, huff="optimal")
    skew = CJ.skewed_table(SKEW_SYMS, short=2)
    codes = CJ._codes(*skew)
    assert all(codes[s][1] == 16 for s in (0x0D, 0x0E, 0x0F, 0x1F, 0x2E)), codes
    tabs = {("dc", 0): CJ.STD_DC_L, ("ac", 0): skew, ("dc", 1): CJ.STD_DC_C, ("ac", 1): skew}
    by_sym = {0x0D: (0, 13), 0x0E: (0, 14), 0x0F: (0, 15), 0x1F: (1, 15), 0x2E: (2, 14), 0x0B: (0, 11)}
    state = {"k": 0}

    def fn(n, ci):
        items = [G.dc(int(rng.integers(-9, 10)))]
        for _ in range(int(rng.integers(2, 7))):
            sym = list(by_sym)[state["k"] % len(by_sym)]
            run, s = by_sym[sym]
            lohi = (1 << (s - 1), (1 << s) - 1)[(state["k"] // len(by_sym)) % 2]
            sg = 1 if (state["k"] // (2 * len(by_sym))) % 2 == 0 else -1
            state["k"] += 1
            items.append(G.ac(run, sg * lohi))
            if rng.integers(0, 2):
                items.append(G.ac(0, int(rng.choice([-1, 1]))))
        return items + [G.EOB]
    for sampling in ("420", "gray"):
        out[f"cat_edges__skew_{sampling}"] = G.stream(64, 64, sampling, tabs, fn)


# 0x01, 0x0D, 0x0E at 2 bits; EOB, 0x0F at 3 bits: after a +-1 (3 bits) the second symbol's total
# is 15 (paired), 16 or 18 (refused: the pair's total is a 4-bit field)
PAIR_AC = ([0, 3, 2] + [0] * 13, [0x01, 0x0D, 0x0E, 0x00, 0x0F])


def _pair_tot15(out, rng):
    tabs = {("dc", 0): CJ.STD_DC_L, ("ac", 0): PAIR_AC, ("dc", 1): CJ.STD_DC_C, ("ac", 1): PAIR_AC}
    for k in range(8):
        def fn(n, ci, k=k):
            items = [G.dc(1 << k) if n == 0 else G.dc(int(rng.integers(-5, 6)))]
            for _ in range(int(rng.integers(1, 4))):
                for s in (13, 14, 15):
                    items.append(G.ac(0, int(rng.choice([-1, 1]))))
                    v = int(rng.integers(1 << (s - 1), 1 << s))
                    items.append(G.ac(0, v if rng.integers(0, 2) else -v))
            return items + [G.EOB]
        out[f"pair_tot15__420_v{k}"] = G.stream(64, 48, "420", tabs, fn)


# sixteen 4-bit DC codes, sizes 0 .. 15 (Kraft-complete: 1111 is size 15); the second table's
# symbols carry a high nibble that NanoJPEG masks off (value & 15)
DC_WIDE = ([0, 0, 0, 16] + [0] * 12, list(range(16)))
DC_NIBBLE = ([0, 0, 0, 16] + [0] * 12, [0x00] + [(((s * 7) % 15 + 1) << 4) | s for s in range(1, 16)])
DC_WIDE_DIFFS = (32767, -32767, -16384, 16384, 8191, -8191, -2048, 2048, -32767, 32767, 16384, -16384, -8191, 8191,
                 2048, -2048)


def _dc_wide(out, rng):
    for tag, dct in (("plain", DC_WIDE), ("nibble", DC_NIBBLE)):
        tabs = {("dc", 0): dct, ("ac", 0): CJ.STD_AC_L, ("dc", 1): dct, ("ac", 1): CJ.STD_AC_C}
        count = [0, 0, 0]

        def fn(n, ci, count=count, dct=dct):
            d = DC_WIDE_DIFFS[count[ci] % len(DC_WIDE_DIFFS)]  # (per component: the sum stays in int16)
            count[ci] += 1
            s, e = G._mag(d)
            return [("dc", dct[1][s], e, s)] + G._fat(rng)[1:]
        out[f"dc_wide__{tag}_420"] = G.stream(64, 48, "420", tabs, fn)


DC_WALK = [-16385, -32770, -32769, -32768, -32767, -32766, -16383, 0, 16383, 32766, 32767, 32768, 32769, 32770, 16385, 0]
DC_ESCAPE_VALUES = tuple(range(-32770, -32765)) + tuple(range(32766, 32771))


def _dc_escape(out, rng):
    """The absolute DC of one component walks through kDcEscape's neighbourhood, over and over:
    in the first 512-byte lane, in later ones and in the last MCU row."""
    def noisy(arr):
        for a in arr:
            a[..., 0] = rng.integers(-100, 101, a.shape[:2])
            for by in range(a.shape[0]):
                for bx in range(a.shape[1]):
                    pos = rng.choice(np.arange(1, 64), int(rng.integers(6, 20)), replace=False)
                    a[by, bx, pos] = rng.integers(1, 32, len(pos)) * rng.choice([-1, 1], len(pos))
    comps = CJ.sampling_comps("420")
    order = _scan_order(64, 64, comps)
    for ci in (0, 2):
        for q0 in (1, 255):
            arr = CJ.empty_blocks(64, 64, comps)
            noisy(arr)
            for k, (by, bx) in enumerate(order[ci]):
                arr[ci][by, bx, 0] = DC_WALK[k % len(DC_WALK)]
            qt = {0: [q0] + [2] * 63, 1: [q0] + [3] * 63}
            out[f"dc_escape__420_c{ci}_q{q0}"] = CJ.write(64, 64, comps, qt, arr, huff="optimal")
    # gray 256 x 128, every difference +32767 and q[0] = 255: dcpred * 255 passes 2^31
    comps = CJ.sampling_comps("gray")
    arr = CJ.empty_blocks(256, 128, comps)
    noisy(arr)
    for k, (by, bx) in enumerate(_scan_order(256, 128, comps)[0]):
        arr[0][by, bx, 0] = 32767 * (k + 1)
    out["dc_escape__gray_256x128_q255"] = CJ.write(256, 128, comps, {0: [255] + [2] * 63}, arr, huff="optimal")


# '0' = EOB, '1' = 0x0F: Kraft-complete. 0x0F with +32767 is sixteen 1 bits. With DC_WIDE the
# 1 bits NanoJPEG reads behind an early EOI decode too (DC size 15, +32767, then 0x0F, +32767, ...).
FF_AC = ([2] + [0] * 15, [0x00, 0x0F])


def _ff_dense(out):
    tabs = {("dc", 0): DC_WIDE, ("ac", 0): FF_AC, ("dc", 1): DC_WIDE, ("ac", 1): FF_AC}

    def blocks(ncoef):
        def fn(n, ci):  # (a small DC step per block: otherwise all blocks are alike and a misplaced one passes)
            return [G.dc(n % 7 - 3)] + [G.ac(0, 32767)] * ncoef + ([G.EOB] if ncoef < 63 else [])
        return fn
    for sampling in ("420", "gray"):
        for ncoef in (20, 63):
            out[f"ff_dense__{sampling}_{ncoef}"] = G.stream(64, 64, sampling, tabs, blocks(ncoef))
    # DC steps of -16384, -16384, +16384, +16384: a lane that enters at the first or the last of them
    # has a lane-local DC sum of exactly -32768, the escape value itself, two blocks later
    def stepped(nc):
        count = [0] * nc

        def fn(n, ci):
            d = (-16384, -16384, 16384, 16384)[count[ci] % 4]
            count[ci] += 1
            return [G.dc(d)] + [G.ac(0, 32767)] * 63
        return fn
    out["ff_dense__420_63_dcstep"] = G.stream(64, 64, "420", tabs, stepped(3))
    out["ff_dense__gray_63_dcstep"] = G.stream(64, 64, "gray", tabs, stepped(1))
    out["ff_dense__cutff_420_63"] = G.stream(64, 64, "420", tabs, blocks(63), cut=0.6, end=b"\xff")
    out["ff_dense__cuteoi_420_63"] = G.stream(64, 64, "420", tabs, blocks(63), cut=0.6)


RUN_SIZE0 = [r << 4 for r in range(1, 15)]  # 0x10 .. 0xE0


def _ac_run_size0(out, rng):
    """An AC symbol of size 0 and run 1 .. 14 in a fat valid scan, shifted bit by bit between the
    variants so it falls in either lookup position of the write loop."""
    freq = {0x00: 400, 0xF0: 2}
    for s in range(1, 6):
        freq[s] = 300
        freq[0x10 | s] = 200
    for s in RUN_SIZE0:
        freq[s] = 20
    act = CJ.optimal_table(freq)
    tabs = {("dc", 0): CJ.STD_DC_L, ("ac", 0): act, ("dc", 1): CJ.STD_DC_C, ("ac", 1): act}
    for k in range(8):
        few = [G.ac(0, 1)] * (k % 4)
        bad = [G.dc(-2)] + few + [G.ac(0, 5), ("ac", RUN_SIZE0[(5 * k + 4) % 14], 0, 0)]
        out[f"ac_run_size0__420_v{k}"] = G.stream(64, 64, "420", tabs, G._shifted(rng, k, 57, bad))


_CACHE = {}


def streams():
    if "all" not in _CACHE:
        out = {}
        rng = np.random.default_rng(20262)
        _cat_edges(out, rng)
        _pair_tot15(out, rng)
        _dc_wide(out, rng)
        _dc_escape(out, rng)
        _ff_dense(out)
        _ac_run_size0(out, rng)
        _idct_into(out, "420", wide=True)
        gray = {}
        _idct_into(gray, "gray", wide=False)  # (k_idct's gray unit shape in the mode runs as well)
        out.update({n: d for n, d in gray.items() if family(n) in ("gate14", "gate22")})
        assert all(len(d) < 256 * 1024 for d in out.values())
        _CACHE["all"] = out
    return dict(_CACHE["all"])


# ------------------------------------------------------------------ what a file holds
def parse(data: bytes):
    """Header fields of a baseline file: quant tables (natural order), components (hs, vs, tq, dc
    table, ac table), Huffman code lengths {("dc" | "ac", id): {symbol: length}}, size, scan bytes."""
    qt, huff, comps, p = {}, {}, [], 2
    w = h = 0
    while True:
        m, length = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        seg = data[p + 4:p + 2 + length]
        if m == 0xDB:
            nat = np.zeros(64, np.int64)
            nat[DEZIGZAG] = list(seg[1:65])
            qt[seg[0]] = nat
        elif m == 0xC0:
            h, w = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            comps = [[seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i], 0, 0] for i in range(seg[5])]
        elif m == 0xC4:
            bits, vals = list(seg[1:17]), list(seg[17:])
            huff[("ac" if seg[0] & 0x10 else "dc", seg[0] & 15)] = {s: ln for s, (_c, ln) in CJ._codes(bits, vals).items()}
        elif m == 0xDA:
            for i in range(seg[0]):
                comps[i][3], comps[i][4] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
            return {"qt": qt, "huff": huff, "comps": comps, "w": w, "h": h, "scan": data[p + 2 + length:]}
        p += 2 + length


def analyse(data: bytes, decode_trace):
    """The blocks NanoJPEG decodes from `data` (decode_trace: the oracle's), per block: component,
    dequantized coefficients (natural order, the DC product at 0, as Python-width integers), DC
    difference, and the AC symbols with their code + magnitude bit totals."""
    hd = parse(data)
    code, coef, dc = decode_trace(data, 1 << 14)
    cyc = [ci for ci, c in enumerate(hd["comps"]) for _ in range(c[0] * c[1])]
    n = len(coef)
    comp = np.array([cyc[i % len(cyc)] for i in range(n)], np.int64)
    deq = coef.astype(np.int64)
    diffs = np.zeros(n, np.int64)
    pred = [0] * len(hd["comps"])
    tots = []  # per block: [(symbol, code bits + magnitude bits)]
    for i in range(n):
        c = hd["comps"][comp[i]]
        deq[i] *= hd["qt"][c[2]]
        deq[i, 0] = int(dc[i]) * int(hd["qt"][c[2]][0])
        diffs[i] = int(dc[i]) - pred[comp[i]]
        pred[comp[i]] = int(dc[i])
        lens = hd["huff"][("ac", c[4])]
        z = coef[i].astype(np.int64)[DEZIGZAG]
        row, run = [], 0
        for k in range(1, 64):
            if z[k] == 0:
                run += 1
                continue
            s = (((run & 15) << 4) | CJ._category(int(z[k])))
            row.append((s, lens.get(s, 0) + (s & 15)))
            run = 0
        tots.append(row)
    scan = hd["scan"]
    return {"code": code, "n": n, "comp": comp, "coef": coef, "dc": dc.astype(np.int64), "deq": deq, "diffs": diffs,
            "tots": tots, "hd": hd, "ff00": 2 * scan.count(b"\xff\x00") / max(1, len(scan))}


def _w32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def row_pass(rows):
    """NanoJPEG's row IDCT (jpeg_dec.h:343-386) on int64 rows [..., 8] with explicit 32-bit
    wrap-around after every operation (what the reference's int arithmetic does on two's-complement
    machines). Shortcut rows included. Used to prove which inputs reach the column gate."""
    W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565
    r = np.asarray(rows, np.int64)
    x1 = _w32(r[..., 4] << 11)
    x2, x3, x4, x5, x6, x7 = r[..., 6], r[..., 2], r[..., 1], r[..., 7], r[..., 5], r[..., 3]
    short = (x1 | x2 | x3 | x4 | x5 | x6 | x7) == 0
    x0 = _w32(_w32(r[..., 0] << 11) + 128)
    x8 = _w32(W7 * _w32(x4 + x5))
    x4 = _w32(x8 + _w32((W1 - W7) * x4))
    x5 = _w32(x8 - _w32((W1 + W7) * x5))
    x8 = _w32(W3 * _w32(x6 + x7))
    x6 = _w32(x8 - _w32((W3 - W5) * x6))
    x7 = _w32(x8 - _w32((W3 + W5) * x7))
    x8 = _w32(x0 + x1)
    x0 = _w32(x0 - x1)
    x1 = _w32(W6 * _w32(x3 + x2))
    x2 = _w32(x1 - _w32((W2 + W6) * x2))
    x3 = _w32(x1 + _w32((W2 - W6) * x3))
    x1 = _w32(x4 + x6)
    x4 = _w32(x4 - x6)
    x6 = _w32(x5 + x7)
    x5 = _w32(x5 - x7)
    x7 = _w32(x8 + x3)
    x8 = _w32(x8 - x3)
    x3 = _w32(x0 + x2)
    x0 = _w32(x0 - x2)
    x2 = _w32(_w32(181 * _w32(x4 + x5)) + 128) >> 8
    x4 = _w32(_w32(181 * _w32(x4 - x5)) + 128) >> 8
    out = np.stack([_w32(x7 + x1) >> 8, _w32(x3 + x2) >> 8, _w32(x0 + x4) >> 8, _w32(x8 + x6) >> 8,
                    _w32(x8 - x6) >> 8, _w32(x0 - x4) >> 8, _w32(x3 - x2) >> 8, _w32(x7 - x1) >> 8], -1)
    flat = np.repeat(_w32(r[..., 0] << 3)[..., None], 8, -1)
    return np.where(short[..., None], flat, out)
