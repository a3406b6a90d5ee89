"""CPU check of the write loop's second lookup on a partly filled window (k_gw_lane without the
error-byte bounds: write_step, then write_step_short, which also serves a window of nb <= 32 bits
when the first-level entry is a plain one whose symbols take no more than nb bits) on
icx_spec_core.h compiled for the host (tests/emu/gw3_emu.cpp): same coefficient blocks, DC values,
block count, failing block and final bit position as the one-lookup schedule of
tests/emu/gw2_emu.cpp, and both equal to the oracle's NanoJPEG trace -- on every golden the
guess-write path takes, the crafted streams of tests/gw2_craft.py and tests/gw3_craft.py, and small
synthetic images. The walk counts the refusals by cause (block end, slow or error entry on a short
window, symbols longer than the window); the crafted streams reach each one, and the study image
shows the same lookups in fewer iterations than with full windows alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import pyoracle as O
from tools import synthpy as S
import gw2_craft
import gw3_craft
import test_gw2_emu as E2

_L = None


def lib():
    global _L
    if _L is None:
        so = os.path.join(E2.EMU_DIR, "libgw3emu.so")
        # (the emulator Makefile's line)
        subprocess.run([E2.HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-fno-strict-aliasing",
                        "-shared", "gw3_emu.cpp", "-o", so], cwd=E2.EMU_DIR, check=True)
        import imagecodecs_amd
        imagecodecs_amd._share_hip_runtime_with_torch()
        _L = C.CDLL(so)
        _L.gw3_walk.restype = C.c_int
        _L.gw3_walk.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return _L


KEYS = ("blocks", "errblk", "endbit", "lookups", "iters", "by_end", "by_entry", "by_fit", "total", "errpos", "end2",
        "shorts", "emptied", "touched", "overran", "fit_pair")


def walk3(data: bytes, cap: int = 1 << 17):
    coef = np.zeros((cap, 64), np.int16)
    dc = np.zeros(cap, np.int32)
    out = np.zeros(16, np.int64)
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    rc = lib().gw3_walk(buf, len(data), coef.ctypes.data, dc.ctypes.data, cap, out.ctypes.data)
    st = dict(zip(KEYS, (int(v) for v in out)))
    return rc, st, coef[: st["total"]], dc[: st["total"]]


def check(data: bytes, oracle: bool = True):
    """The short-window schedule agrees with the one-lookup schedule (and the oracle's trace); returns
    its counters, or None for a stream the guess-write path does not take."""
    rc3, s3, c3, d3 = walk3(data)
    rc1, s1, c1, d1 = E2.walk(data, False)
    assert rc1 == rc3
    if rc3 == 2:
        return None
    for k in ("blocks", "errblk", "endbit", "total"):
        assert s1[k] == s3[k], (k, s1, s3)
    assert np.array_equal(c1, c3) and np.array_equal(d1, d3)
    assert s3["touched"] == 0 and s3["overran"] == 0, s3  # a refused lane changes nothing; consume(n) only with n <= nb
    assert s3["shorts"] <= s3["lookups"] - s3["iters"] and s3["emptied"] <= s3["shorts"] and s3["fit_pair"] <= s3["by_fit"], s3
    # every iteration does a second lookup or is refused one (a failing first lookup ends the walk)
    assert (s3["lookups"] - s3["iters"] + s3["by_end"] + s3["by_entry"] + s3["by_fit"]
            == s3["iters"] - (s3["errpos"] == 1)), s3
    if oracle:
        oc, ocoef, odc = O.decode_trace(data)
        if oc == 0:
            assert s3["errblk"] == -1 and s3["blocks"] == s3["total"] == len(ocoef), s3
            assert np.array_equal(c3, ocoef) and np.array_equal(d3, odc)
        else:  # NanoJPEG's failing block: the last one its trace entered
            e = len(ocoef) - 1
            assert s3["errblk"] == e, (s3, e)
            assert np.array_equal(c3[:e], ocoef[:e]) and np.array_equal(d3[:e], odc[:e])
    return s3


def test_short_window_schedule_goldens():
    """Every golden without restart markers (the streams the guess-write path takes), corrupt ones
    included."""
    taken = [s for s in (check(open(os.path.join(GOLDEN, n), "rb").read()) for n in sorted(E2.MANIFEST)) if s is not None]
    assert len(taken) >= 40
    assert sum(s["shorts"] for s in taken) > 0


def test_short_window_schedule_gw2_crafted():
    """The two-lookup loop's crafted streams: long codes, block ends, a full block, a run past
    coefficient 63, an invalid code, long-code tables and truncated data."""
    stats = {n: check(d) for n, d in gw2_craft.streams().items()}
    assert all(s is not None for s in stats.values())
    # 16-bit codes with 10 magnitude bits one after the other: the second is a slow entry on a short window
    s = stats["long26_420_128"]
    assert s["by_entry"] > s["iters"] // 2, s
    for p in ("zrl_past63", "invalid", "cut_ff", "cut_marker"):  # the failure in both positions
        pos = sorted(s["errpos"] for n, s in stats.items() if n.startswith(p))
        assert pos[0] == 1 and pos[-1] == 2, (p, pos)


def test_short_window_refusals_are_reached():
    """tests/gw3_craft.py: each cause of refusal with a nonzero count, short lookups committed next to
    them, and windows drained to their last bit."""
    stats = {n: check(d) for n, d in gw3_craft.streams().items()}
    assert all(s is not None and s["errblk"] == -1 for s in stats.values())
    print({n: {k: s[k] for k in ("lookups", "iters", "shorts", "emptied", "by_end", "by_entry", "by_fit", "fit_pair")}
           for n, s in stats.items()})
    s = stats["short_ab_420_128"]  # 1. a symbol longer than the window; the long code after it is a slow entry
    assert s["by_fit"] > 100 and s["fit_pair"] == 0 and s["by_entry"] > 100 and s["shorts"] > 100, s
    s = stats["short_acc_420_128"]  # 2. a pair whose second symbol does not fit
    assert s["fit_pair"] > 50 and s["shorts"] > 100, s
    s = stats["short_aa_444_64"]  # 3. a code longer than the AC window right after a long first symbol
    assert s["by_entry"] > 100 and s["by_entry"] > 4 * s["by_fit"], s
    for n, s in stats.items():
        if n.startswith("short_mix"):  # 4. everything at once
            assert min(s["by_end"], s["by_entry"], s["by_fit"], s["fit_pair"], s["shorts"]) > 0, (n, s)
    assert sum(s["emptied"] for s in stats.values()) > 0  # nb == 0 after a short lookup: the next refill gives 32


@pytest.mark.parametrize("sampling", ["420", "444", "gray"])
def test_short_window_schedule_synthetic(sampling):
    data = S.synth_jpeg(6100, 256, 256, sampling, 90)
    s = check(data)
    _, s2, _, _ = E2.walk(data, True)
    assert s["errblk"] == -1 and s["shorts"] > 0 and s["iters"] < s2["iters"], (s, s2)


def test_schedule_study_counters():
    """The study behind the change, at a quarter of its size (synth_jpeg 2048^2 4:2:0 q90, the
    flagship pool's generator; at 4096^2, seeds 1234 / 1240: 9.2 % / 9.8 % fewer iterations, 1.935 /
    1.937 lookups an iteration): the same lookups as with full windows alone, in fewer iterations."""
    data = S.synth_jpeg(1234, 2048, 2048, "420", 90)
    s = check(data, oracle=False)
    _, s2, _, _ = E2.walk(data, True)
    print({k: s[k] for k in ("lookups", "iters", "shorts", "emptied", "by_end", "by_entry", "by_fit", "fit_pair")},
          {k: s2[k] for k in ("lookups", "iters", "by_end", "by_bits")})
    assert s["lookups"] == s2["lookups"], (s, s2)
    assert s["iters"] < s2["iters"], (s, s2)
    assert s["by_entry"] + s["by_fit"] < s2["by_bits"], (s, s2)  # (what was refused for bits is now mostly taken)
