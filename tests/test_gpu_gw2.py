"""GPU parity of the guess-write lanes' two-lookup write loop (k_gw_lane: a second AC lookup of the
same block per iteration when the block did not end and the reader's window still holds more than
32 bits). Small images forced onto the guess-write path (ICX_GW=1); the planner cuts scans of up
to 256 KiB into 512-byte lanes, the shortest (what ICX_SUB_BYTES=512 would fix: not set here, the
library reads it once per process, and it would cut every later test's large images the same way),
so every image spans several lanes: coefficient-array images (tools/coefjpeg.py), small
synthetic ones, and the crafted streams of tests/gw2_craft.py, which put long codes, block ends,
a full block, a run past coefficient 63, an invalid code, long-code tables and truncated data where
the second lookup meets them (tests/test_gw2_emu.py checks on the CPU that they do). Status and
pixels equal the oracle's, bit for bit, and every image stays on the parallel path."""
import numpy as np
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
from tools import coefjpeg as CJ
from tools import synthpy as S
import gw2_craft

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def _coef_image(seed, w, h, sampling, huff):
    """Random sparse blocks (3 .. 20 coefficients of up to 6 magnitude bits) through coefjpeg."""
    rng = np.random.default_rng(seed)
    comps = CJ.sampling_comps(sampling)
    bl = CJ.empty_blocks(w, h, comps)
    for b in bl:
        by, bx = b.shape[:2]
        b[..., 0] = rng.integers(-200, 201, (by, bx))
        for y in range(by):
            for x in range(bx):
                pos = rng.choice(np.arange(1, 64), int(rng.integers(3, 21)), replace=False)
                b[y, x, pos] = rng.integers(1, 64, len(pos)) * rng.choice([-1, 1], len(pos))
    return CJ.write(w, h, comps, gw2_craft.QT, bl, huff=huff)


@pytest.fixture(scope="module")
def inputs():
    out = dict(gw2_craft.streams())
    out["coef_420_64"] = _coef_image(1, 64, 64, "420", "std")
    out["coef_420_200x136_opt"] = _coef_image(2, 200, 136, "420", "optimal")
    out["coef_444_96"] = _coef_image(3, 96, 96, "444", "std")
    out["coef_gray_256"] = _coef_image(4, 256, 256, "gray", "optimal")
    for k, sampling in enumerate(("420", "444", "gray")):
        out[f"synth_{sampling}_256"] = S.synth_jpeg(6100 + k, 256, 256, sampling, 90)
    return {n: (d, O.decode(d)) for n, d in sorted(out.items())}  # the oracle's result, once


def test_two_lookup_lanes_match_oracle(ctx, monkeypatch, inputs):
    monkeypatch.setenv("ICX_GW", "1")
    names = list(inputs)
    assert all(len(inputs[n][0]) < 256 * 1024 for n in names)  # 512-byte lanes
    b = icx.Batch(ctx, len(names), 256, 256)
    res = b.decode_host([inputs[n][0] for n in names])
    stats = b.path_stats()
    b.close()
    print(stats)
    # no silent fallback: every image decided by the lanes (NanoJPEG's syntax errors included)
    assert stats == {"parallel": len(names), "fallback": 0, "sequential": 0}, stats
    for n, (code, w, h, c, pix) in zip(names, res):
        ocode, ow, oh, on, opix = inputs[n][1]
        assert code == ocode, (n, code, ocode)
        if ocode == 0:
            assert (w, h, c) == (ow, oh, on), n
            assert pix.tobytes() == opix, n


def test_inputs_are_what_they_claim(inputs):
    """The error cases fail in the oracle, the others decode: the comparison above is not vacuous."""
    for n, (_, (ocode, *_rest)) in inputs.items():
        bad = n.startswith(("zrl_past63", "invalid", "cut_ff", "cut_marker"))
        assert (ocode != 0) == bad or n.startswith("cut_eoi"), (n, ocode)
