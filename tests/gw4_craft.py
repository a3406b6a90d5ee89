"""Crafted baseline streams for the guess-write lanes' third lookup of an iteration (k_gw_lane: after
the second lookup one more AC lookup of the same block under write_step_short's rule, without a
refill). Built with the helpers of tests/gw2_craft.py from tests/gw3_craft.py's AC table:

    A  a 16-bit code with 10 magnitude bits (26 bits; longer than the 10-bit AC window: a slow entry),
    B  a 2-bit code with 9 magnitude bits (11 bits: a plain entry, never half of a pair),
    C  a 3-bit code with 1 magnitude bit (4 bits; C C is a pair entry of 8 bits).

An iteration starts with 33 .. 64 bits in the window, so what the third lookup meets is set by the
two symbols before it: B B leaves 11 .. 42 bits, A B at most 27 (always a short window), A C at most
34. Each stream puts one kind of event there; the fills walk through every phase because the rounds'
lengths are no multiple of 32.

    streams() -> {name: bytes}, shared by tests/test_gw4_emu.py (CPU) and tests/test_gpu_gw4.py."""
import numpy as np

import gw2_craft as G
from gw3_craft import TABS, _blocks, _sym


def _bad(rng, k, bad_at, tail):
    """Valid blocks of B and C; block 0's DC difference has k + 1 magnitude bits (a k-bit shift of all
    that follows between variants); block `bad_at` is a DC code and then `tail`."""
    def fn(n, ci):
        if n == bad_at:
            return [G.dc(-2)] + tail
        body = [_sym(rng, s) for s in rng.choice(list("BC"), int(rng.integers(3, 20)))]
        return [G.dc(1 << k if n == 0 else int(rng.integers(-30, 31)))] + body + [G.EOB]
    return fn


def streams():
    out = {}
    rng = np.random.default_rng(20270)
    # 1. B B B ...: 33 bits a round, so the fill at the third lookup falls by one bit a round, from a
    # full window to one that B no longer fits (refused for bits), through the one it empties (nb == 0)
    out["third_bbb_420_128"] = G.stream(128, 128, "420", TABS, _blocks(rng, lambda n: "B" * (3 + n % 29)))
    # 2. B, then pairs C C: the third lookup commits a pair
    out["third_bcc_420_128"] = G.stream(128, 128, "420", TABS,
                                        _blocks(rng, lambda n: "".join(rng.choice(["BCCCC", "BCC", "BBCCCC"], 2 + n % 7))))
    # 3. A B A: the third lookup is a code longer than the AC window on a window of at most 27 bits
    # (a slow entry: refused); A C B: B on a window of 3 .. 34 bits
    out["third_aba_444_64"] = G.stream(64, 64, "444", TABS, _blocks(rng, lambda n: "ABA" * (1 + n % 6)))
    out["third_acb_420_128"] = G.stream(128, 128, "420", TABS,
                                        _blocks(rng, lambda n: "".join(rng.choice(["ACB", "ACCB"], 2 + n % 9))))
    # 4. short blocks: DC, one or two symbols, EOB -- the block ends at the third lookup, or at the
    # second (the third is then refused for the block end); C EOB is a pair entry, B EOB is not
    out["third_ends_420_256"] = G.stream(256, 256, "420", TABS,
                                         _blocks(rng, lambda n: str(rng.choice(["B", "C", "BB", "BC", "CB", "", "BBB"]))))
    # 5. every order of the three, other samplings
    for name, w, h, sampling in (("third_mix_420_200x136", 200, 136, "420"), ("third_mix_444_96", 96, 96, "444"),
                                 ("third_mix_gray_160", 160, 160, "gray")):
        out[name] = G.stream(w, h, sampling, TABS,
                             _blocks(rng, lambda n: "".join(rng.choice(list("ABBCCC"), int(rng.integers(3, 40))))))
    # 6. an invalid code (sixteen 1 bits: every code of the table starts with 0 or 10) as the third
    # lookup of its iteration: behind A B the window is short and the error entry is refused -- the
    # next iteration's full window decides it --, behind C C it is mostly a full one and fails there
    for k in range(8):
        bad = G.raw(0xFFFF, 16)
        out[f"third_invalid_ab_420_64_v{k}"] = G.stream(64, 64, "420", TABS, _bad(rng, k, 57, [
            _sym(rng, "B"), _sym(rng, "B"), _sym(rng, "A"), _sym(rng, "B"), bad]))
        out[f"third_invalid_cc_420_64_v{k}"] = G.stream(64, 64, "420", TABS, _bad(rng, k, 57, [
            _sym(rng, "B"), _sym(rng, "B"), _sym(rng, "B"), _sym(rng, "C"), _sym(rng, "B"), bad]))
    return out


ERRORS = ("third_invalid",)  # name prefixes of the streams NanoJPEG refuses


def dri_streams():
    """The mix with restart markers (tests/dri_gw_craft.py's rstream), for the interval-aligned
    guess-write lanes: 64 MCUs of 4:2:0 in 8 intervals of about 2 KB (from 512 bytes an interval the
    planner cuts each into lanes with ICX_DRI_GW=1; 6 blocks an MCU keep every MCU above 8 bits)."""
    from dri_gw_craft import rstream
    rng = np.random.default_rng(20271)
    mix = _blocks(rng, lambda n: "".join(rng.choice(list("ABBCCC"), int(rng.integers(20, 56)))))
    return {"third_mix_dri_420_128": rstream(128, 128, "420", TABS, 8, lambda n, ci, m: mix(n, ci))}
