"""GPU parity of restart intervals on the guess-write lanes (k_spec_plan's kint > 0) on the crafted
streams of tests/dri_gw_craft.py, forced onto that path (ICX_GW=1, ICX_DRI_GW=1: intervals from 512
bytes). Status and pixels equal the oracle's bit for bit, and -- what the pixels cannot tell, since
every failure of the lanes ends in a fallback that decodes the same image -- Batch.dri_stats() equals
what the CPU emulator (tests/test_dri_gw_emu.py: the same __host__ __device__ code, lane by lane)
says became of each image: decided by the guess-write lanes, or sent back to one lane per interval."""
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
import dri_gw_craft as CR
from test_dri_gw_emu import run as emu_run

pytestmark = pytest.mark.gpu

W, H = 512, 512  # every crafted image fits (the largest: 408 x 200 and 384 x 384)


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def expected(r):
    """The counters one image adds, from the emulator's result: (gw, gw_fallback, fallback)."""
    return (int(r.outcome == 0), int(r.outcome == 3 and r.ret == 0), int(r.ret == 1))


@pytest.fixture(scope="module")
def inputs():
    """{name: (bytes, oracle result, emulator result)}: crafted, controls, damaged, then images
    without restart markers -- each reference computed once."""
    out = {}
    for group in (CR.streams(), CR.controls(), CR.damaged(), CR.plain()):
        for n, d in group.items():
            out[n] = (d, O.decode(d), None if n in CR.plain() else emu_run(d))
    return out


def same_as_oracle(name, got, want):
    code, w, h, c, pix = got
    ocode, ow, oh, on, opix = want
    assert code == ocode, (name, code, ocode)
    if ocode == 0:
        assert (w, h, c) == (ow, oh, on), name
        assert pix.tobytes() == opix, name


def test_each_crafted_stream_alone(ctx, monkeypatch, inputs):
    monkeypatch.setenv("ICX_GW", "1")
    monkeypatch.setenv("ICX_DRI_GW", "1")
    b = icx.Batch(ctx, 1, W, H)
    seen = set()
    for n, (d, want, r) in inputs.items():
        if r is None:
            continue
        (got,) = b.decode_host([d])
        same_as_oracle(n, got, want)
        gw, fb, seq = expected(r)
        assert b.dri_stats() == {"gw": gw, "gw_fallback": fb}, (n, b.dri_stats(), r.outcome)
        assert b.path_stats() == {"parallel": 1 - seq, "fallback": seq, "sequential": 0}, (n, b.path_stats())
        seen.add((gw, fb))
    b.close()
    assert seen == {(1, 0), (0, 1), (0, 0)}  # decided by the lanes, sent back, not planned


@pytest.fixture(scope="module")
def batch_runs(ctx, inputs):
    """The whole set in one batch, with the guess-write DRI lanes on and off."""
    names = list(inputs)
    out = {}
    for env in ("1", "0"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("ICX_GW", "1")
            mp.setenv("ICX_DRI_GW", env)
            b = icx.Batch(ctx, len(names), W, H)
            res = b.decode_host([inputs[n][0] for n in names])
            out[env] = (res, b.path_stats(), b.dri_stats())
            b.close()
    return names, out


def test_mixed_batch_matches_oracle_and_emulator(inputs, batch_runs):
    names, runs = batch_runs
    res, paths, dri = runs["1"]
    for n, got in zip(names, res):
        same_as_oracle(n, got, inputs[n][1])
    exp = [expected(inputs[n][2]) for n in names if inputs[n][2] is not None]
    want = {"gw": sum(e[0] for e in exp), "gw_fallback": sum(e[1] for e in exp)}
    print(dri, paths)
    assert want["gw"] >= 20 and want["gw_fallback"] >= 20  # (the emulator's: both kinds are in the batch)
    assert dri == want, (dri, want)
    assert paths == {"parallel": len(names) - sum(e[2] for e in exp), "fallback": sum(e[2] for e in exp), "sequential": 0}


def test_mixed_batch_without_the_guess_write_dri_lanes(inputs, batch_runs):
    names, runs = batch_runs
    res, paths, dri = runs["0"]
    assert dri == {"gw": 0, "gw_fallback": 0}, dri
    assert paths["sequential"] == 0 and paths["parallel"] + paths["fallback"] == len(names), paths
    for n, got, ref in zip(names, res, runs["1"][0]):
        same_as_oracle(n, got, inputs[n][1])
        assert got[:4] == ref[:4], n
        if got[0] == 0:
            assert got[4].tobytes() == ref[4].tobytes(), n
