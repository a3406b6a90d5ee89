"""CPU check of the write loop's two-lookup schedule (k_gw_lane: write_step, then write_step_more
for a second AC lookup of the same block when the block did not end and the reader's window still
holds more than 32 bits) against the one-lookup schedule, on icx_spec_core.h compiled for the host
(tests/emu/gw2_emu.cpp): same coefficient blocks, DC values, block count, failing block and final
bit position on every golden the guess-write path takes and on the crafted streams of
tests/gw2_craft.py -- and both equal to the oracle's NanoJPEG trace. The walk also returns the
counters of the schedule study (lookups, iterations, second lookups refused for block end / bits)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import pyoracle as O
from tools import synthpy as S
import gw2_craft

EMU_DIR = os.path.join(ROOT, "tests", "emu")
MANIFEST = json.load(open(os.path.join(GOLDEN, "decode_manifest.json")))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_L = None


def lib():
    global _L
    if _L is None:
        so = os.path.join(EMU_DIR, "libgw2emu.so")
        # (the emulator Makefile's line)
        subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-fno-strict-aliasing",
                        "-shared", "gw2_emu.cpp", "-o", so], cwd=EMU_DIR, check=True)
        import imagecodecs_amd
        imagecodecs_amd._share_hip_runtime_with_torch()
        _L = C.CDLL(so)
        _L.gw2_walk.restype = C.c_int
        _L.gw2_walk.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return _L


KEYS = ("blocks", "errblk", "endbit", "lookups", "iters", "by_end", "by_bits", "refill_moved", "total", "errpos",
        "end2", "pool2", "walk2")


def walk(data: bytes, two: bool, cap: int = 1 << 17):
    coef = np.zeros((cap, 64), np.int16)
    dc = np.zeros(cap, np.int32)
    out = np.zeros(16, np.int64)
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    rc = lib().gw2_walk(buf, len(data), int(two), coef.ctypes.data, dc.ctypes.data, cap, out.ctypes.data)
    st = dict(zip(KEYS, (int(v) for v in out)))
    return rc, st, coef[: st["total"]], dc[: st["total"]]


def check(data: bytes, oracle: bool = True):
    """Both schedules agree (and match the oracle's trace); returns the two-lookup walk's counters,
    or None for a stream the guess-write path does not take."""
    rc2, s2, c2, d2 = walk(data, True)
    rc1, s1, c1, d1 = walk(data, False)
    assert rc1 == rc2
    if rc2 == 2:
        return None
    for k in ("blocks", "errblk", "endbit", "total"):
        assert s1[k] == s2[k], (k, s1, s2)
    assert np.array_equal(c1, c2) and np.array_equal(d1, d2)
    assert s2["refill_moved"] == 0, s2
    assert s1["lookups"] == s1["iters"] and s2["lookups"] == s1["lookups"], (s1, s2)
    assert s2["iters"] + (s2["lookups"] - s2["iters"]) == s2["lookups"]
    # every iteration does a second lookup or is refused one (a failing first lookup ends the walk)
    assert s2["lookups"] - s2["iters"] + s2["by_end"] + s2["by_bits"] == s2["iters"] - (s2["errpos"] == 1), s2
    if oracle:
        oc, ocoef, odc = O.decode_trace(data)
        if oc == 0:
            assert s2["errblk"] == -1 and s2["blocks"] == s2["total"] == len(ocoef), s2
            assert np.array_equal(c2, ocoef) and np.array_equal(d2, odc)
        else:  # NanoJPEG's failing block: the last one its trace entered
            e = len(ocoef) - 1
            assert s2["errblk"] == e, (s2, e)
            assert np.array_equal(c2[:e], ocoef[:e]) and np.array_equal(d2[:e], odc[:e])
    return s2


def test_two_lookup_schedule_goldens():
    """Every golden without restart markers (the streams the guess-write path takes), corrupt ones
    included."""
    taken = [s for s in (check(open(os.path.join(GOLDEN, n), "rb").read()) for n in sorted(MANIFEST)) if s is not None]
    assert len(taken) >= 40
    assert sum(s["lookups"] - s["iters"] for s in taken) > 0


@pytest.fixture(scope="module")
def crafted():
    return gw2_craft.streams()


def _group(stats, prefix):
    g = [s for n, s in stats.items() if n.startswith(prefix)]
    assert g
    return g


def test_two_lookup_schedule_crafted(crafted):
    stats = {n: check(d) for n, d in crafted.items()}
    assert all(s is not None for s in stats.values())
    codes = {n: O.decode(d)[0] for n, d in crafted.items()}
    for n, c in codes.items():  # the cases are what their names say
        bad = n.startswith(("zrl_past63", "invalid", "cut_ff", "cut_marker"))
        assert (c != 0) == bad or n.startswith("cut_eoi"), (n, c)
    s = stats["long26_420_128"]  # 1. second lookups mostly refused for bits
    assert s["by_bits"] > s["iters"] // 2 and s["by_bits"] > 2 * (s["lookups"] - s["iters"]), s
    s = stats["short_eob_420_256"]  # 2. blocks end at the second lookup (unless it is refused for bits)
    assert s["end2"] + s["by_bits"] == s["blocks"] and s["end2"] > 4 * s["by_bits"], s
    for s in _group(stats, "full63"):  # 3. the cursor reaches 64 in both positions
        assert 0 < s["end2"] < s["blocks"], s
    for p in ("zrl_past63", "invalid", "cut_ff", "cut_marker"):  # 4, 5, 7: the failure in both positions
        pos = sorted(s["errpos"] for s in _group(stats, p))
        assert pos[0] == 1 and pos[-1] == 2, (p, pos)
    assert stats["pool_420_128"]["pool2"] > 100 and stats["pool_420_128"]["walk2"] == 0  # 6.
    assert stats["search_420_96"]["walk2"] > 100


def test_lane_failures_are_noted_per_stretch():
    """gw_lane_err: records carry the first failed block of the stretch before them (+ 1), the
    lane's err the one after the last record; a failure before the splice does not hide a later
    one on the true path (the crafted error streams above met exactly that in 512-byte lanes)."""
    NONE = 2 ** 31 - 1
    L = lib()
    L.gw2_lane_err.restype = C.c_int32

    def err(rec, gerr, m, c=0, cerr=NONE):
        b = (C.c_int32 * len(rec))(*[r[0] for r in rec])
        cnt = (C.c_int32 * len(rec))(*[r[1] for r in rec])
        return L.gw2_lane_err(b, cnt, len(rec), gerr, m, c, cerr)

    rec = [(2, 3), (0, 6), (8, 9)]  # block 1 failed before record 0, block 7 between records 1 and 2
    assert err(rec, NONE, -2) == 1          # synchronised at its start: the whole lane is true
    assert err(rec, NONE, 0, c=4) == 4 + (7 - 3)   # spliced at record 0: block 1 was speculative
    assert err(rec, NONE, 1, c=4) == 4 + (7 - 6)
    assert err(rec, NONE, 2, c=4) == NONE
    assert err(rec, 12, 2, c=4) == 4 + (12 - 9)     # after the last record
    assert err(rec, 12, 0, c=4, cerr=2) == 2        # the count lane's own blocks come first
    assert err(rec, 12, -1, c=4) == NONE            # never spliced: the count lane decoded it all
    assert err([(0, 3)], 5, 0, c=1) == 1 + (5 - 3) and err([], 5, -2) == 5


@pytest.mark.parametrize("sampling", ["420", "444", "gray"])
def test_two_lookup_schedule_synthetic(sampling):
    s = check(S.synth_jpeg(6100, 256, 256, sampling, 90))
    assert s["errblk"] == -1 and 1.3 < s["lookups"] / s["iters"] < 2.0, s


def test_schedule_study_counters():
    """The study behind the loop change, at a quarter of its size (synth_jpeg 2048^2 4:2:0 q90, the
    flagship pool's generator; at 4096^2, seeds 1234 / 1240: 1.757 / 1.746 lookups an iteration).
    About 1.75 lookups per iteration; block ends refuse a quarter of the second lookups not done,
    bits the rest."""
    s = check(S.synth_jpeg(1234, 2048, 2048, "420", 90), oracle=False)
    print({k: s[k] for k in ("lookups", "iters", "by_end", "by_bits")})
    assert 1.70 < s["lookups"] / s["iters"] < 1.80, s
    assert s["by_end"] < s["by_bits"], s
