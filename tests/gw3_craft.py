"""Crafted baseline streams for the guess-write lanes' second lookup on a partly filled window
(k_gw_lane / write_step_short: a window of nb <= 32 bits still serves the second lookup when the
first-level entry is a plain one and its symbols take no more than nb bits). Built with the helpers
of tests/gw2_craft.py from one AC table that has all three kinds of symbol:

    A  a 16-bit code with 10 magnitude bits (26 bits: it leaves the window at 7 .. 38 bits, and in
       the second position its code is longer than the 10-bit AC window: a slow entry),
    B  a 2-bit code with 9 magnitude bits (11 bits: a plain entry that a window of 7 .. 10 bits
       cannot serve),
    C  a 3-bit code with 1 magnitude bit (4 bits; C C is a pair entry of 8 bits, which a window of
       4 .. 7 bits holds only half of).

    streams() -> {name: bytes}, shared by tests/test_gw3_emu.py (CPU) and tests/test_gpu_gw3.py."""
import numpy as np

from tools import coefjpeg as CJ
import gw2_craft as G

#           code length:  1  2  3  4 ...                       15 16
AC3 = ([0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1], [0x09, 0x01, 0x00, 0x02, 0x1A, 0x0A])
TABS = {("dc", 0): CJ.STD_DC_L, ("ac", 0): AC3, ("dc", 1): CJ.STD_DC_C, ("ac", 1): AC3}


def _sym(rng, kind):
    lo, hi = {"A": (512, 1024), "B": (256, 512), "C": (1, 2)}[kind]
    v = int(rng.integers(lo, hi))
    return G.ac(0, v if rng.integers(0, 2) else -v)


def _blocks(rng, pattern):
    """block_fn: a DC code, then `pattern(n)`'s kinds (at most 63), then EOB."""
    def fn(n, ci):
        return [G.dc(int(rng.integers(-30, 31)))] + [_sym(rng, k) for k in pattern(n)] + [G.EOB]
    return fn


def streams():
    codes = CJ._codes(*AC3)
    assert [codes[s][1] for s in (0x0A, 0x09, 0x01)] == [16, 2, 3]
    out = {}
    rng = np.random.default_rng(20263)
    # 1. A then B, over and over (37 bits a round: the window's fill walks through every phase):
    # B after A is refused when fewer than 11 bits are left, and A after B is a slow entry
    out["short_ab_420_128"] = G.stream(128, 128, "420", TABS, _blocks(rng, lambda n: "AB" * (4 + n % 9)))
    # 2. A then one to three C (the rounds' lengths differ, so the fill takes every phase): the pair
    # C C after A does not fit a window of 4 .. 7 bits, though its first symbol would
    out["short_acc_420_128"] = G.stream(128, 128, "420", TABS,
                                        _blocks(rng, lambda n: "".join(rng.choice(["AC", "ACC", "ACCC"], 3 + n % 11))))
    # 3. A A: a code longer than the AC window right after a long first symbol
    out["short_aa_444_64"] = G.stream(64, 64, "444", TABS, _blocks(rng, lambda n: "A" * (2 + n % 17)))
    # 4. every order of the three, other samplings
    for name, w, h, sampling in (("short_mix_420_200x136", 200, 136, "420"), ("short_mix_444_96", 96, 96, "444"),
                                 ("short_mix_gray_160", 160, 160, "gray")):
        out[name] = G.stream(w, h, sampling, TABS,
                             _blocks(rng, lambda n: "".join(rng.choice(list("ABC"), int(rng.integers(3, 40))))))
    return out


def dri_streams():
    """The same mix with restart markers (tests/dri_gw_craft.py's rstream), for the interval-aligned
    guess-write lanes: 64 MCUs of 4:2:0 in 8 intervals of about 2 KB (from 512 bytes an interval the
    planner cuts each into lanes with ICX_DRI_GW=1; 6 blocks an MCU keep every MCU above 8 bits)."""
    from dri_gw_craft import rstream
    rng = np.random.default_rng(20264)
    mix = _blocks(rng, lambda n: "".join(rng.choice(list("ABC"), int(rng.integers(12, 40)))))
    return {"short_mix_dri_420_128": rstream(128, 128, "420", TABS, 8, lambda n, ci, m: mix(n, ci))}
