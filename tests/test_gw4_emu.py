"""CPU check of the write loop's third lookup (k_gw_lane without the error-byte bounds: write_step,
then write_step_short while it is taken and the block goes on, three lookups an iteration at most)
on icx_spec_core.h compiled for the host (tests/emu/gw4_emu.cpp, the lookup cap a parameter): at
caps 3 and 4 the same coefficient blocks, DC values, block count, failing block and final bit
position as at cap 2 -- which is tests/emu/gw3_emu.cpp's walk -- and all equal to the oracle's
NanoJPEG trace, on every golden the guess-write path takes, the crafted streams of
tests/gw2_craft.py, tests/gw3_craft.py and tests/gw4_craft.py, and small synthetic images. The walk
counts by position what was taken, refused (by cause), ended, emptied and paired; the crafted
streams reach each of them at the third position, and the study image gives the iteration counts
the change was budgeted with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import pyoracle as O
from tools import synthpy as S
import gw2_craft
import gw3_craft
import gw4_craft
import test_gw2_emu as E2
import test_gw3_emu as E3

_L = None
MAX_CAP = 8
HEAD = ("blocks", "errblk", "endbit", "lookups", "iters", "total", "errpos", "touched", "overran")
AT = ("taken", "by_end", "by_entry", "by_fit", "ended", "emptied", "pairs", "invalid_wait")


def lib():
    global _L
    if _L is None:
        so = os.path.join(E2.EMU_DIR, "libgw4emu.so")
        # (the emulator Makefile's line)
        subprocess.run([E2.HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-fno-strict-aliasing",
                        "-shared", "gw4_emu.cpp", "-o", so], cwd=E2.EMU_DIR, check=True)
        import imagecodecs_amd
        imagecodecs_amd._share_hip_runtime_with_torch()
        _L = C.CDLL(so)
        _L.gw4_walk.restype = C.c_int
        _L.gw4_walk.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return _L


def walk4(data: bytes, lookups: int, cap: int = 1 << 17):
    """One walk with at most `lookups` lookups an iteration. The counters by position are lists
    indexed by the position (1-based; index 0 unused)."""
    coef = np.zeros((cap, 64), np.int16)
    dc = np.zeros(cap, np.int32)
    out = np.zeros(16 + 8 * MAX_CAP, np.int64)
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    rc = lib().gw4_walk(buf, len(data), lookups, coef.ctypes.data, dc.ctypes.data, cap, out.ctypes.data)
    st = dict(zip(HEAD, (int(v) for v in out)))
    for c, name in enumerate(AT):
        st[name] = [0] + [int(out[16 + 8 * p + c]) for p in range(MAX_CAP)]
    return rc, st, coef[: st["total"]], dc[: st["total"]]


def check(data: bytes, oracle: bool = True, cap: int = 1 << 17):
    """Caps 3 and 4 agree with cap 2, cap 2 with gw3_walk, and all with the oracle's trace; returns
    {cap: counters}, or None for a stream the guess-write path does not take."""
    rc2, s2, c2, d2 = walk4(data, 2, cap)
    rc0, s0, c0, d0 = E3.walk3(data, cap)
    assert rc0 == rc2
    if rc2 == 2:
        return None
    assert rc2 == 0
    for k in ("blocks", "errblk", "endbit", "total", "lookups", "iters", "errpos"):  # cap 2 is gw3_walk
        assert s0[k] == s2[k], (k, s0, s2)
    assert np.array_equal(c0, c2) and np.array_equal(d0, d2)
    assert (s2["by_end"][2], s2["by_entry"][2], s2["by_fit"][2], s2["ended"][2]) == \
           (s0["by_end"], s0["by_entry"], s0["by_fit"], s0["end2"]), (s0, s2)
    stats = {2: s2}
    for n in (3, 4):
        rc, s, c, d = walk4(data, n, cap)
        assert rc == 0
        for k in ("blocks", "errblk", "endbit", "total"):
            assert s[k] == s2[k], (n, k, s2, s)
        assert np.array_equal(c, c2) and np.array_equal(d, d2), n
        stats[n] = s
    for n, s in stats.items():
        assert s["touched"] == 0 and s["overran"] == 0, (n, s)  # a refused lane changes nothing; consume(n) only with n <= nb
        assert sum(s["taken"]) == s["lookups"] and s["taken"][1] == s["iters"], (n, s)
        assert sum(s["ended"]) == s["blocks"], (n, s)
        assert all(v == 0 for name in AT for v in s[name][n + 1:]), (n, s)  # nothing past the cap
        assert s["invalid_wait"][1] == 0 and all(a <= b for a, b in zip(s["invalid_wait"], s["by_entry"])), (n, s)
        for p in range(2, n + 1):  # a lookup taken at p - 1 is followed by one at p or by one refusal (or it failed)
            assert s["taken"][p] + s["by_end"][p] + s["by_entry"][p] + s["by_fit"][p] == s["taken"][p - 1] - (s["errpos"] == p - 1), (n, p, s)
    if oracle:
        oc, ocoef, odc = O.decode_trace(data)
        if oc == 0:
            assert s2["errblk"] == -1 and s2["blocks"] == s2["total"] == len(ocoef), s2
            assert np.array_equal(c2, ocoef) and np.array_equal(d2, odc)
        else:  # NanoJPEG's failing block: the last one its trace entered
            e = len(ocoef) - 1
            assert s2["errblk"] == e, (s2, e)
            assert np.array_equal(c2[:e], ocoef[:e]) and np.array_equal(d2[:e], odc[:e])
    return stats


def test_third_lookup_goldens():
    """Every golden without restart markers (the streams the guess-write path takes), corrupt ones
    included."""
    taken = [s for s in (check(open(os.path.join(GOLDEN, n), "rb").read()) for n in sorted(E2.MANIFEST)) if s is not None]
    assert len(taken) >= 40
    assert sum(s[3]["taken"][3] for s in taken) > 0 and sum(s[4]["taken"][4] for s in taken) > 0


def test_third_lookup_earlier_crafted():
    """The crafted streams of the two-lookup loop and of the short-window second lookup: long codes,
    block ends, a full block, a run past coefficient 63, an invalid code, truncated data, and every
    refusal of the second position."""
    stats = {n: check(d) for n, d in {**gw2_craft.streams(), **gw3_craft.streams()}.items()}
    assert all(s is not None for s in stats.values())
    bad = {n: s[3]["errpos"] for n, s in stats.items() if n.startswith(gw2_craft.ERRORS) and s[3]["errblk"] != -1}
    print(bad)
    assert set(bad.values()) == {1, 2, 3}, bad  # the variants' shifts put the failure in every position


def test_third_position_events_are_reached():
    """tests/gw4_craft.py: at the third position each cause of refusal, a block end, a committed pair,
    a window left empty and an invalid code that waits for the next full window -- each with a
    nonzero count."""
    stats = {n: check(d) for n, d in gw4_craft.streams().items()}
    assert all(s is not None for s in stats.values())
    s3 = {n: s[3] for n, s in stats.items()}
    print({n: {k: s[k][3] for k in AT} for n, s in s3.items()})
    for n, s in s3.items():
        assert (s["errblk"] != -1) == n.startswith(gw4_craft.ERRORS), (n, s)
    s = s3["third_bbb_420_128"]  # 1. refused for bits; drained to the last bit
    assert s["by_fit"][3] > 0 and s["emptied"][3] > 0 and s["taken"][3] > 0, s
    s = s3["third_bcc_420_128"]  # 2. a pair committed at the third lookup
    assert s["pairs"][3] > 0, s
    s = s3["third_aba_444_64"]  # 3. a slow entry on a short window
    assert s["by_entry"][3] > 0 and s["invalid_wait"][3] == 0, s
    s = s3["third_acb_420_128"]
    assert s["by_fit"][3] > 0 and s["taken"][3] > 0, s
    s = s3["third_ends_420_256"]  # 4. the block ends at the third lookup, or before it
    assert s["ended"][3] > 0 and s["by_end"][3] > 0, s
    for n, s in s3.items():
        if n.startswith("third_mix"):  # 5. everything at once
            assert min(s[k][3] for k in ("taken", "by_end", "by_entry", "by_fit", "ended", "pairs")) > 0, (n, s)
    assert sum(s["emptied"][3] for s in s3.values()) > 0
    # 6. the invalid code: refused on a short window and failing as the next iteration's first
    # lookup, and failing in place on a full one
    ab = [s for n, s in s3.items() if n.startswith("third_invalid_ab")]
    assert sum(s["invalid_wait"][3] for s in ab) > 0 and any(s["invalid_wait"][3] and s["errpos"] == 1 for s in ab), ab
    assert any(s["errpos"] == 3 for n, s in s3.items() if n.startswith("third_invalid")), s3


def test_third_lookup_dri_stream_intervals():
    """The restart-interval stream's mix of symbols reaches the third position's events. The walk
    takes scans without restart markers, so the counters come from the same generator and mix
    written without the markers (the markers byte-align each interval and reset the DC predictors,
    which moves the windows' phases and nothing else)."""
    rng = np.random.default_rng(20271)  # (gw4_craft.dri_streams' generator and mix)
    mix = gw3_craft._blocks(rng, lambda n: "".join(rng.choice(list("ABBCCC"), int(rng.integers(20, 56)))))
    s = check(gw2_craft.stream(128, 128, "420", gw3_craft.TABS, mix))[3]
    assert min(s[k][3] for k in ("taken", "by_end", "by_entry", "by_fit", "pairs")) > 0, s
    assert len(gw4_craft.dri_streams()) == 1


@pytest.mark.parametrize("sampling", ["420", "444", "gray"])
def test_third_lookup_synthetic(sampling):
    data = S.synth_jpeg(6300, 256, 256, sampling, 90)
    s = check(data)
    assert s[3]["errblk"] == -1 and s[3]["taken"][3] > 0 and s[4]["iters"] < s[3]["iters"] < s[2]["iters"], s


def test_schedule_study_counters():
    """The study behind the change (synth_jpeg 4096^2 4:2:0 q90 seed 1234, the flagship pool's
    generator): the same lookups at every cap, in 3,111,680 / 2,142,436 / 1,691,212 iterations at
    caps 2 / 3 / 4; the third lookup is taken in 87 % of iterations."""
    data = S.synth_jpeg(1234, 4096, 4096, "420", 90)
    s = check(data, oracle=False, cap=1 << 19)
    print({n: {"lookups": v["lookups"], "iters": v["iters"], **{k: v[k][2:n + 1] for k in AT}} for n, v in s.items()})
    assert s[2]["lookups"] == s[3]["lookups"] == s[4]["lookups"] == 6022236, s
    assert (s[2]["iters"], s[3]["iters"], s[4]["iters"]) == (3111680, 2142436, 1691212), s
    assert 0.86 < s[3]["taken"][3] / s[3]["iters"] < 0.88, s
