"""CPU tests of restart intervals on the guess-write lanes (k_spec_plan's kint > 0) without a GPU.

tests/emu/spec_emu.cpp's emu_gw_dri_decode runs the kernels' own __host__ __device__ code
(icx_spec_core.h: dri_gw_plan, lane_span, gc_walk with bmax, dri_end_kind, gw_lane_total / gw_lane_err)
lane by lane as k_gw_lane, k_gw_check, k_gw_count, k_gw_repair and k_gw_scan's interval branch do,
and falls back to emu_dri_decode where they call dri_gw_fallback. Its status, coefficients and DC
values must equal the oracle's NanoJPEG trace whatever the outcome; its counters show that the
crafted streams of tests/dri_gw_craft.py reach what they are made for."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import pyoracle as O
from tools import synthpy as S
from driutil import dri_corruptions, rst_markers, scan_start
from test_spec_emu import emu_lib
import dri_gw_craft as CR

MANIFEST = json.load(open(os.path.join(GOLDEN, "decode_manifest.json")))
FOREIGN = json.load(open(os.path.join(GOLDEN, "foreign_manifest.json")))
STAT_KEYS = ("lanes", "synced", "counted", "spliced", "repaired", "stops", "unspliced", "unspliced_final", "kint",
             "nint", "queued", "empty")
Result = collections.namedtuple("Result", "ret status outcome coef dc stats residues")
_L = None


def lib():
    global _L
    if _L is None:
        L = emu_lib()
        L.emu_gw_dri_decode.restype = C.c_int
        L.emu_gw_dri_decode.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        L.emu_dri_gw_plan.restype = C.c_int
        L.emu_dri_gw_plan.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.emu_lane_span.restype = None
        L.emu_lane_span.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p]
        _L = L
    return _L


def plan(data: bytes, dri_min: int = CR.DRI_MIN):
    """k_spec_plan's decision (dri_gw_plan): {kint, sb, nint, min_mcu_bits}; kint 0 for a file the
    parallel decoder does not take."""
    out = np.zeros(4, np.int64)
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    lib().emu_dri_gw_plan(buf, len(data), dri_min, out.ctypes.data)
    return dict(zip(("kint", "sb", "nint", "min_mcu_bits"), (int(v) for v in out)))


def run(data: bytes, dri_min: int = CR.DRI_MIN, cap: int = 1 << 15) -> Result:
    coef = np.zeros((cap, 64), np.int16)
    dc = np.zeros(cap, np.int32)
    nb, st, oc = C.c_int64(), C.c_int32(), C.c_int32()
    stats = np.zeros(20, np.int64)
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    ret = lib().emu_gw_dri_decode(buf, len(data), dri_min, coef.ctypes.data, dc.ctypes.data, cap, C.byref(nb), C.byref(st),
                                  C.byref(oc), stats.ctypes.data)
    assert ret in (0, 1, 2), ret
    return Result(ret, st.value, oc.value, coef[: nb.value], dc[: nb.value],
                  dict(zip(STAT_KEYS, (int(v) for v in stats[:12]))), [int(v) for v in stats[12:20]])


def exact(data: bytes, r: Result):
    """The emulator's result is NanoJPEG's: its status, and up to the failing block its blocks."""
    oc, ocoef, odc = O.decode_trace(data)
    if r.ret != 0:  # the sequential kernel (1) or NanoJPEG's own header verdict (2) decides
        return oc
    assert r.status == (0 if oc == 0 else 5), (r.status, oc, r.outcome)
    if oc == 0:
        assert len(r.coef) == len(ocoef)
        assert np.array_equal(r.coef, ocoef) and np.array_equal(r.dc, odc), r.outcome
    return oc


@pytest.fixture(scope="module")
def crafted():
    """{name: (bytes, Result)} of every crafted stream, each run once."""
    out = {}
    for group in (CR.streams(), CR.controls(), CR.damaged()):
        for n, d in group.items():
            out[n] = (d, run(d))
    return out


def ulen_between(data, a, b):
    """Unstuffed bytes of data[a:b] (entropy-coded bytes between two markers)."""
    return (b - a) - data.count(b"\xff\x00", a, b)


def test_every_crafted_stream_equals_the_oracle(crafted):
    assert set(CR.REACH) == set(CR.streams())
    for n, (d, r) in crafted.items():
        assert r.ret == 0, n  # (nothing here goes to the sequential kernel)
        oc = exact(d, r)
        if n in CR.streams() or n in CR.controls():
            assert oc == 0, n


@pytest.mark.parametrize("dri_min", [CR.DRI_MIN, 1])
def test_every_golden_with_restart_markers_equals_the_oracle(dri_min):
    """dri_min = 1 plans even the goldens' tiny intervals with kint = 2 (lanes of a few bytes, many of
    them empty): not what the product does, but the same code at its smallest sizes."""
    outcomes = collections.Counter()
    for n in sorted(set(MANIFEST) | set(FOREIGN)):
        d = open(os.path.join(GOLDEN, n), "rb").read()
        if plan(d, dri_min)["nint"] == 0:
            continue
        r = run(d, dri_min)
        exact(d, r)
        outcomes[r.outcome] += 1
    assert sum(outcomes.values()) >= 80, outcomes
    if dri_min == 1:
        assert outcomes[0] >= 40 and outcomes[3] >= 1 and outcomes[2] >= 10, outcomes  # (2: the gray goldens, 6-bit MCUs)
    else:
        assert outcomes[0] >= 1, outcomes  # foreign/cat_q90_420_opt_rst_row.jpg


def test_undamaged_streams_are_decided_by_the_guess_write_lanes(crafted):
    """Outcome 0 for every undamaged stream -- advice2_gray included, which dropped to the interval
    lanes (outcome 3) before lane_span gave the interval-final rule to every lane that reaches the
    interval's end -- but for advice4_gray (below). The controls are not planned."""
    for n in CR.streams():
        if n != "advice4_gray":
            assert crafted[n][1].outcome == 0, n
    for n in CR.controls():
        assert crafted[n][1].outcome == 2 and plan(crafted[n][0])["kint"] == 0, n
    assert plan(crafted["ctl_minbits_gray"][0])["min_mcu_bits"] < 8
    p = plan(crafted["ctl_short_420"][0])
    assert p["min_mcu_bits"] >= 8 and p["nint"] > 0


def test_reach_kint_by_sampling(crafted):
    for n, (w, h, smp, _, nint) in CR._KINT.items():
        d, r = crafted[n]
        p = plan(d)
        want = int(n[4])
        assert (p["kint"] == want) if want < 4 else (p["kint"] >= 4), (n, p)
        assert p["nint"] == nint and r.stats["kint"] == p["kint"] and r.stats["lanes"] == nint * p["kint"], (n, p, r.stats)
        assert p["sb"] <= 2560
    assert {n.split("_")[1] for n in CR._KINT} == {"420", "444", "422", "gray"}


def test_reach_interval_counts(crafted):
    d, r = crafted["nint1_420"]
    assert plan(d)["nint"] == 1 and plan(d)["kint"] >= 2 and not rst_markers(d) and r.stats["lanes"] == plan(d)["kint"]
    d, r = crafted["short_last_444"]
    assert plan(d)["nint"] == 3 and CR.nmcu_of(64, 64, "444") % 24 == 16
    d, r = crafted["wrap_gray"]
    mk = rst_markers(d)
    assert len(mk) == plan(d)["nint"] - 1 > 8 and [d[k + 1] & 7 for k in mk] == [k & 7 for k in range(len(mk))]
    d, r = crafted["many_gray"]
    assert plan(d)["nint"] > 256 and plan(d)["kint"] == 2 and r.stats["nint"] == plan(d)["nint"]
    d, r = crafted["straddle_gray"]
    p = plan(d)
    assert p["kint"] == 3 and p["nint"] * 3 > 256 and 256 % 3 != 0  # interval 85 holds lanes 255, 256, 257


def test_reach_every_end_residue(crafted):
    """An interval's last MCU ends at every bit residue of the byte before the marker."""
    hist = np.zeros(8, np.int64)
    for n in CR.streams():
        hist += np.array(crafted[n][1].residues)
    print("interval-final exits by residue 8 em - p:", hist.tolist())
    assert (hist > 0).all(), hist
    # and singly in the stream with the most intervals
    assert all(v > 0 for v in crafted["many_gray"][1].residues)


def test_reach_stuffed_ff_before_the_marker(crafted):
    d, r = crafted["ff00_end_420"]
    mk = rst_markers(d)
    assert len(mk) == 3 and all(d[k - 2:k] == b"\xff\x00" for k in mk)
    assert d[-4:] == b"\xff\x00\xff\xd9"


def test_reach_unsynchronised_lanes_and_walks_stopped_at_intervals(crafted):
    d, r = crafted["search_r_420"]
    s = r.stats
    print(s)
    assert plan(d)["kint"] >= 3
    assert s["unspliced"] > 0 and s["queued"] > 0 and s["repaired"] > 0 and s["stops"] > 0, s
    assert s["unspliced_final"] > 0  # gc_walk left through its bmax test


def test_reach_short_interval_among_long_ones(crafted):
    """ADVICE low #2: (kint - 1) * ceil(len / kint) >= len for the flat interval."""
    d, r = crafted["advice2_gray"]
    p = plan(d)
    mk = rst_markers(d)
    ln = ulen_between(d, mk[0] + 2, mk[1])
    K = p["kint"]
    assert (K - 1) * -(-ln // K) >= ln and ln < K * K, (K, ln)
    assert d[mk[1] - 1] & 0x3F == 0x3F and d[mk[1] - 1] != 0xFF  # the interval ends 6 bits before the marker
    assert ulen_between(d, scan_start(d), mk[0]) > 20 * 2560
    assert r.stats["empty"] >= 1 and r.outcome == 0


def test_reach_two_mcu_starts_in_the_exit_window(crafted):
    """ADVICE low #4: min_mcu_bits says 9, the MCUs take 7, and interval 0 is 800 of them, ending on
    a byte boundary: MCU starts at 8 em - 7 and at 8 em. The lanes' result is exact either way;
    today the last lane leaves at the first of the two, k_gw_scan counts one MCU too few and the
    image goes to the interval lanes (outcome 3)."""
    d, r = crafted["advice4_gray"]
    p = plan(d)
    mk = rst_markers(d)
    assert p["min_mcu_bits"] >= 8 and p["kint"] == 2 and len(mk) == 1
    assert (mk[0] - scan_start(d)) * 8 == 800 * 7 and b"\xff" not in d[scan_start(d):mk[0]]
    print("advice4_gray outcome:", r.outcome)
    assert r.outcome in (0, 3)
    assert exact(d, r) == 0


def test_reach_damage(crafted):
    dm = CR.damaged()
    oc = {n: O.decode(d)[0] for n, d in dm.items()}
    out = collections.Counter(crafted[n][1].outcome for n in dm)
    assert out[3] >= 20 and out[2] == 0, out
    assert sum(1 for n in dm if oc[n] != 0) >= 20
    for n in dm:
        if "_cut" in n:  # the tail runs into the padding: NanoJPEG's syntax error, decided by the interval lanes
            assert oc[n] != 0 and crafted[n][1].outcome == 3, n


def test_planner_selects_most_of_the_gpu_test_batch():
    """tests/test_gpu_decode.py's guess-write DRI batch: its check of Batch.dri_stats() is not vacuous."""
    from driutil import dri_gw_jpegs
    assert sum(plan(j)["kint"] > 0 for j in dri_gw_jpegs()) >= 5


# ---- lane_span ----
def span(j, nsub, sb, ulen, kint, nint, rs):
    out = np.zeros(5, np.int64)
    a = np.array(rs if len(rs) else [0], np.int64)
    lib().emu_lane_span(j, nsub, sb, ulen, kint, nint, a.ctypes.data, len(rs), out.ctypes.data)
    return dict(zip(("start", "end", "floor", "bmax", "first"), (int(v) for v in out)))


def ref_span(j, ulen, kint, nint, rs):
    """lane_span's kint > 0 rule, restated."""
    m, ii = divmod(j, kint)
    at = lambda k: (rs[k] >> 3) if k < len(rs) else ulen
    sm = 0 if m == 0 else min(at(m - 1) + 2, ulen)
    em = max(at(m), sm) if m + 1 < nint else ulen
    sub = max(1, -(-(em - sm) // kint))
    st = min(sm + ii * sub, em)
    eb = em if ii == kint - 1 else min(sm + (ii + 1) * sub, em)
    if eb == em and m + 1 < nint:
        fe = max(em * 8 - 7, sm * 8)
        return dict(start=min(st * 8, fe), end=fe, floor=sm * 8, bmax=0, first=int(ii == 0))
    return dict(start=st * 8, end=eb * 8, floor=sm * 8, bmax=255, first=int(ii == 0))


def test_lane_span_properties():
    rng = np.random.default_rng(20263)
    seen = collections.Counter()
    for t in range(400):
        nint = int(rng.integers(1, 12))
        kint = int(rng.integers(2, 20))
        ulen = int(rng.integers(2, 4000)) if t % 4 else int(rng.integers(2, 60))
        kind = t % 5
        pos = sorted(int(v) for v in rng.integers(0, max(1, ulen - 1), nint - 1))
        if kind == 1:  # markers missing
            pos = pos[: int(rng.integers(0, nint))]
        elif kind == 2 and len(pos) > 1:  # out of order: at(m) <= sm
            rng.shuffle(pos)
        elif kind == 3 and len(pos) > 1:  # adjacent markers: empty intervals
            pos[1] = pos[0] + int(rng.integers(0, 3))
        rs = [(p << 3) | (k & 7) for k, p in enumerate(pos)]
        nsub = nint * kint
        L = [span(j, nsub, 512, ulen, kint, nint, rs) for j in range(nsub)]
        for j, s in enumerate(L):
            m, ii = divmod(j, kint)
            assert s == ref_span(j, ulen, kint, nint, rs), (t, j, s)
            assert 0 <= s["floor"] <= s["start"] <= s["end"] <= 8 * ulen, (t, j, s)
            assert s["first"] == (ii == 0)
            last_int = m + 1 == nint
            if ii == 0:
                assert s["start"] == s["floor"]
            if ii == kint - 1:  # the interval's last lane
                assert s["bmax"] == (255 if last_int else 0)
                if last_int:
                    assert s["end"] == 8 * ulen
            if ii + 1 < kint:
                nx = L[j + 1]
                assert nx["floor"] == s["floor"]
                if s["bmax"] == 255:  # lanes meet at a byte boundary
                    assert s["end"] % 8 == 0 and nx["start"] == s["end"], (t, j, s, nx)
                else:  # the interval-final rule reached early: the rest of the interval's lanes are empty, at its end
                    assert not last_int and nx["start"] == nx["end"] == s["end"] and nx["bmax"] == 0, (t, j, s, nx)
                    seen["early_final"] += 1
            if s["bmax"] == 0:  # 7 bits before the marker's byte (or an interval without a byte: its start)
                em8 = max(s["floor"], ((rs[m] >> 3) if m < len(rs) else ulen) * 8)
                assert s["end"] == max(em8 - 7, s["floor"]), (t, j, s)
            seen["empty"] += s["start"] == s["end"]
        seen["missing"] += len(rs) < nint - 1
    assert seen["early_final"] > 50 and seen["empty"] > 50 and seen["missing"] > 20, seen


def test_lane_span_plain_cut():
    rng = np.random.default_rng(20264)
    for _ in range(200):
        sb = int(rng.integers(1, 3000))
        ulen = int(rng.integers(1, 100000))
        nsub = (ulen + sb - 1) // sb
        for j in {0, nsub - 1, int(rng.integers(0, nsub))}:
            s = span(j, nsub, sb, ulen, 0, int(rng.integers(0, 5)), [8, 16])
            assert s == dict(start=j * sb * 8, end=ulen * 8 if j == nsub - 1 else (j + 1) * sb * 8, floor=0, bmax=255,
                             first=int(j == 0))
