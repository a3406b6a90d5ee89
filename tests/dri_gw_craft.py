"""Crafted restart-interval (DRI) streams for the interval-aligned guess-write lanes (k_spec_plan's
kint > 0: lane_span, k_gw_lane, k_gw_count, k_gw_repair, k_gw_scan's interval branch). With
ICX_DRI_GW=1 an image qualifies from intervals averaging 512 bytes of scan data, each cut into
kint = clamp(ceil(average / 2560), 2, 64) lanes, so every stream here is small. Each named stream
states what it is meant to reach; tests/test_dri_gw_emu.py asserts from the CPU emulator's counters
that it does, and tests/test_gpu_dri_gw.py decodes the same bytes on the GPU.

    streams() -> {name: bytes}   undamaged streams (the guess-write lanes must decide them)
    controls() -> {name: bytes}  DRI streams the planner must leave to one lane per interval
    damaged() -> {name: bytes}   corrupt and truncated variants
    REACH                        {name: what the stream must reach}

All seeded. Written symbol by symbol (tests/gw2_craft.py's items) where a table or a bit position
matters, from coefficient arrays (tools/coefjpeg.py) or pixels (tools/synthpy.py) elsewhere."""
import functools

import numpy as np

from tools import coefjpeg as CJ
from tools import synthpy as S
from driutil import dri_corruptions, rst_markers, scan_start
from gw2_craft import EOB, QT, STD, ZRL, ac, dc

DRI_MIN = 512  # ICX_DRI_GW=1: kSubBytesSmall


def rstream(w, h, sampling, tabs, restart, block_fn, end=b"\xff\xd9"):
    """gw2_craft.stream with restart markers: block_fn(n, ci, m) gives block n's items (component ci,
    MCU m); DC items are differences, so a block_fn restarts its own predictors (a difference is
    all the stream holds). Each interval is padded with 1 bits and followed by RSTn."""
    comps = CJ.sampling_comps(sampling)
    head = CJ.write(w, h, comps, QT, CJ.empty_blocks(w, h, comps), huff=tabs, restart=restart)
    head = head[:scan_start(head)]
    codes = {k: CJ._codes(*v) for k, v in tabs.items()}
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    nmcu = ((w + 8 * hmax - 1) // (8 * hmax)) * ((h + 8 * vmax - 1) // (8 * vmax))
    bw = CJ._Bits()
    n = 0
    for m in range(nmcu):
        if m and m % restart == 0:
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + ((m // restart - 1) & 7)])
        for ci, (hs, vs, _tq) in enumerate(comps):
            for _ in range(hs * vs):
                for it in block_fn(n, ci, m):
                    c, length = codes[(it[0], 0 if ci == 0 else 1)][it[1]]
                    bw.put(c, length)
                    bw.put(it[2], it[3])
                n += 1
    bw.flush()
    return head + bytes(bw.out) + end


def dense(rng, size, ncoef=63):
    """A block of `ncoef` AC coefficients of `size` magnitude bits each (63: no EOB)."""
    def fn(n, ci, m):
        v = rng.integers(1 << (size - 1), 1 << size, ncoef) * rng.choice([-1, 1], ncoef)
        return [dc(int(rng.integers(-30, 31)))] + [ac(0, int(x)) for x in v] + ([] if ncoef == 63 else [EOB])
    return fn


def nmcu_of(w, h, sampling):
    mw, mh = {"gray": (8, 8), "444": (8, 8), "422": (16, 8), "420": (16, 16)}[sampling]
    return ((w + mw - 1) // mw) * ((h + mh - 1) // mh)


# kint by sampling: (size, AC magnitude bits, intervals). Standard tables: a size-s coefficient takes
# its code plus s bits (10 at s = 5, 18 at s = 8, 26 at s = 10), so a 63-coefficient block is about
# 80 / 142 / 205 bytes.
# (gray: the standard tables give a 6-bit flat MCU, which the planner refuses; GRAY_AC has EOB at 6 bits)
GRAY_AC = ([0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], [0x05, 0x00, 0x0A])
_KINT = {
    # name: (w, h, sampling, magnitude bits, intervals)
    "kint2_420": (64, 64, "420", 5, 4), "kint3_420": (64, 64, "420", 8, 2), "kint4_420": (64, 64, "420", 10, 2),
    "kint2_444": (64, 64, "444", 5, 4), "kint3_444": (64, 64, "444", 5, 2), "kint4_444": (64, 64, "444", 10, 3),
    "kint2_422": (64, 64, "422", 5, 4), "kint3_422": (64, 64, "422", 7, 2), "kint4_422": (64, 64, "422", 10, 2),
    "kint2_gray": (64, 64, "gray", 5, 4), "kint3_gray": (64, 64, "gray", 10, 2), "kint4_gray": (96, 96, "gray", 10, 2),
}

REACH = {
    **{n: "kint " + ("= " + n[4] if n[4] != "4" else ">= 4") + ", " + n.split("_")[1] for n in _KINT},
    "nint1_420": "one interval: restart >= the MCU count",
    "short_last_444": "a last interval with fewer than R MCUs",
    "wrap_gray": "more than 8 intervals: the marker number wraps",
    "ff00_end_420": "stuffed FF 00 as every interval's last data byte",
    "many_gray": "more than 256 intervals: k_gw_scan strides over them",
    "straddle_gray": "nint * kint > 256 with kint = 3: an interval's lanes straddle two 256-lane record groups",
    "search_r_420": "a lane whose guess never synchronises: repair walks that stop at the next interval's first lane",
    "advice2_gray": "one interval shorter than about kint^2 bytes among long ones",
    "advice4_gray": "7-bit MCUs under min_mcu_bits >= 8: two MCU starts inside [8 em - 7, 8 em]",
}


def _tabs(dc_l, ac_l, dc_c=None, ac_c=None):
    return {("dc", 0): dc_l, ("ac", 0): ac_l, ("dc", 1): dc_c or dc_l, ("ac", 1): ac_c or ac_l}


GRAY = _tabs(CJ.STD_DC_L, GRAY_AC)


# gw2_craft's search_* table: EOB at 1 bit, every other AC symbol at 12 bits (more 16-bit windows than
# the step tables' pool holds, and codes of one length: a lane that starts off the true path stays off)
_OTHERS = sorted({(r << 4) | s for r in range(16) for s in range(1, 11)} | {0xF0})
SEARCH_AC = ([1] + [0] * 10 + [len(_OTHERS)] + [0] * 4, [0x00] + _OTHERS)
# ADVICE low #4: DC category 0 and ZRL at 1 bit, 0xE1 at 2 bits, EOB at 8: min_mcu_bits = 1 + 8, yet
# DC 0, ZRL x 3, 0xE1 and its magnitude bit fill a block (48 + 14 + 1 = 63) in 7 bits
ODD_DC = ([1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 1, 2])
ODD_AC = ([1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0], [0xF0, 0xE1, 0x00])


@functools.lru_cache(maxsize=None)
def streams():
    out = {}
    rng = np.random.default_rng(20261)
    for name, (w, h, smp, size, nint) in _KINT.items():
        r = (nmcu_of(w, h, smp) + nint - 1) // nint
        out[name] = rstream(w, h, smp, GRAY if smp == "gray" else STD, r, dense(rng, size))
    out["nint1_420"] = rstream(64, 64, "420", STD, 16 + 5, dense(rng, 5))
    out["short_last_444"] = rstream(64, 64, "444", STD, 24, dense(rng, 5))  # 64 MCUs: 24, 24, 16
    out["wrap_gray"] = rstream(96, 96, "gray", GRAY, 7, dense(rng, 10))     # 144 MCUs: 21 intervals
    # every interval's last coefficient is +1023 (ten 1 bits) with no EOB after it: the last data
    # byte is FF whatever the bit position, stuffed, then the marker
    def ff_end(n, ci, m):
        b = dense(rng, 5)(n, ci, m)
        if ci == 2 and m % 4 == 3:
            b[-1] = ac(0, 1023)
        return b
    out["ff00_end_420"] = rstream(64, 64, "420", STD, 4, ff_end)
    out["many_gray"] = rstream(256, 256, "gray", GRAY, 3, dense(rng, 10))      # 1024 MCUs: 342 intervals of ~615 B
    out["straddle_gray"] = rstream(384, 384, "gray", GRAY, 26, dense(rng, 10))  # 2304 MCUs: 89 intervals of ~5.3 KB
    # (one DC and one AC table for all three components: block ends do not depend on the block's place
    # in the MCU, so a lane that guessed it wrong stays wrong to its end)
    ts = _tabs(CJ.STD_DC_L, SEARCH_AC)

    def search(n, ci, m):
        o = [dc(int(rng.integers(-30, 31)))]
        for _ in range(int(rng.integers(20, 41))):
            v = int(rng.integers(1, 16))
            o.append(ac(0, v if rng.integers(0, 2) else -v))
        return o + [EOB]
    out["search_r_420"] = rstream(256, 256, "420", ts, 64, search)  # 256 MCUs: 4 intervals
    # ADVICE low #2. 408 x 200 gray (51 x 25 MCUs), R = 255: five intervals, the second flat (DC 0 and
    # EOB: 8 bits an MCU with GRAY, its first 10: 2042 bits, 256 bytes ending 6 bits before the marker),
    # the others dense (about 205 bytes an MCU, 52 KB): kint = 17, lanes of ceil(256 / 17) = 16 bytes in
    # the flat interval, and 16 of them already cover it
    def flat_among(n, ci, m):
        if m // 255 != 1:
            return dense(rng, 10)(n, ci, m)
        return [dc(1 if m == 255 else 0), EOB]
    out["advice2_gray"] = rstream(408, 200, "gray", GRAY, 255, flat_among)
    # 320 x 320 gray: 1600 MCUs of 7 bits, two intervals of 800 (700 bytes each, ending on a byte
    # boundary: the last MCU of interval 0 starts at bit 8 em - 7 and the marker at 8 em)
    to = _tabs(ODD_DC, ODD_AC)

    def odd(n, ci, m):
        return [dc(0), ZRL, ZRL, ZRL, ac(14, 1 if rng.integers(0, 2) else -1)]
    out["advice4_gray"] = rstream(320, 320, "gray", to, 800, odd)
    return out


@functools.lru_cache(maxsize=None)
def controls():
    """DRI streams the planner leaves to one lane per interval."""
    return {
        # standard tables, gray: DC category 0 (2 bits) + EOB (4 bits) = 6 < 8 bits an MCU
        "ctl_minbits_gray": S.synth_jpeg(7300, 256, 256, "gray", 95, 1),
        # intervals averaging under 512 bytes
        "ctl_short_420": S.synth_jpeg(7301, 128, 128, "420", 60, 2),
    }


@functools.lru_cache(maxsize=None)
def damaged():
    out = {}
    rng = np.random.default_rng(20262)
    und = streams()
    for base in ("kint3_420", "wrap_gray"):
        for k, v in enumerate(dri_corruptions(und[base], rng, 16)):
            out[f"{base}_c{k}"] = v
    # truncation inside the last interval: its tail runs into the 0xFF padding
    for base, cut in (("kint4_444", 300), ("short_last_444", 40), ("kint2_gray", 7)):
        d = und[base]
        assert len(d) - cut > rst_markers(d)[-1] + 2
        out[f"{base}_cut"] = d[:len(d) - cut]
        out[f"{base}_cut_eoi"] = d[:len(d) - cut] + b"\xff\xd9"
    return out


def plain():
    """Images without restart markers for the mixed batch (the plain guess-write lanes)."""
    return {"plain_420": S.synth_jpeg(7310, 200, 152, "420", 85), "plain_gray": S.synth_jpeg(7311, 96, 120, "gray", 90)}
