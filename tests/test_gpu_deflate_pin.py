"""GPU: the bytes of the two deflate writers (PNG encode, OpenEXR ZIP write), pinned. Every case is
a small input of the existing GPU tests (their generators, imported), encoded through
Context.png_encode / Context.exr_encode; the file's length and SHA-256 must equal
tests/golden/deflate_pin/digests.json.

The JSON was recorded once from a build of the commit it names ("parent": the commit before the
writers came to share icx_deflate_core.h / icx_deflate_wave.h), by running this module with
ICX_DEFLATE_PIN_RECORD=<that commit's hash>: the cases then write the file instead of asserting.
It is never regenerated from a later tree: a refactor of the writers that changes a byte fails here.

(The colour-mode images are test_gpu_png.py's constructions under a fixed seed: that test seeds
them with Python's per-process string hash.)

Not reached by any small input: the emit kernels' overflow branch (a segment whose bits exceed the
2048-word LDS image goes straight to the output); both writers call the one emit_segment there."""
import hashlib
import json
import os

import numpy as np
import pytest

import imagecodecs_amd as icx
from conftest import GOLDEN
import exrw_util as U
import pngutil as P
import test_gpu_exr_write as E
import test_gpu_png as G
import test_gpu_png_deflate as D

pytestmark = pytest.mark.gpu

PIN = os.path.join(GOLDEN, "deflate_pin", "digests.json")
RECORD = os.environ.get("ICX_DEFLATE_PIN_RECORD")  # the parent commit's hash: record, do not assert


def _png(px, seam=None):
    def enc(ctx, monkeypatch):
        if seam is not None:
            monkeypatch.setenv("ICX_PNG_SEAM", seam)
        a = px()
        h, w, d = a.shape
        return ctx.png_encode(w, h, d, a.tobytes())
    return enc


def _pal(idx, seam=None):
    return _png(lambda: D.pal8(idx()), seam)


def _colour_mode(case):
    rng = np.random.default_rng({"pal16": 16, "grey1": 1, "grey_alpha": 2}[case])
    w, h = 45, 31
    if case == "pal16":
        return G._palette_img(rng, 16, w, h)
    g = rng.integers(0, 2 if case == "grey1" else 256, (h, w, 1))
    if case == "grey1":
        return np.repeat((g * 255).astype(np.uint8), 3, axis=2)
    return np.concatenate([np.repeat(g.astype(np.uint8), 3, axis=2), rng.integers(0, 256, (h, w, 1)).astype(np.uint8)], axis=2)


def _exr(a, fp16=False):
    return lambda ctx, monkeypatch: ctx.exr_encode(a(), fp16=fp16)


def _exr_golden(name):
    def enc(ctx, monkeypatch):
        a, fp16, _ = U.load_golden(name)
        return ctx.exr_encode(a, fp16=fp16)
    return enc


def _exr_batch(ctx, monkeypatch):
    """Three sizes in one exr_encode_device_batch call, slots at odd offsets: the files, joined."""
    import torch
    imgs = [U.smooth(70, 37, 4, 40), U.smooth(9, 8, 4, 41), U.smooth(300, 20, 4, 42)]
    srcs = [E._dev(a) for a in imgs]
    caps = [icx.lib().icx_exr_encode_bound(a.shape[1], a.shape[0], 4, 0) for a in imgs]
    slots, at = [], 1
    for c in caps:
        slots.append(at)
        at += c + c % 2
    out = torch.zeros(at + 64, dtype=torch.uint8, device=srcs[0].device)
    codes, sizes = ctx.exr_encode_device_batch([s.data_ptr() for s in srcs], [a.shape[1] for a in imgs],
                                               [a.shape[0] for a in imgs], 4, False,
                                               [out.data_ptr() + s for s in slots], caps)
    assert list(codes) == [0, 0, 0]
    host = out.cpu().numpy()
    return b"".join(host[s:s + int(n)].tobytes() for s, n in zip(slots, sizes))


_CL_GROUPS = [(5, 24), (4, 1), (6, 2), (7, 3), (8, 5), (9, 8), (10, 13), (11, 21), (12, 34), (13, 55), (14, 89)]
_JOINS = [(1, 40, 1), (2, 40, 2), (3, 40, 3), (4, 1, 300), (5, 100, 100)]
_CUTS = [(1, 1, 60), (2, 2, 60), (3, 3, 60)]

CASES = {
    # PNG: sizes of the parse (one literal; one segment; several segments; two base blocks; merged blocks)
    "png_rgba_1x1": _png(lambda: P.synth_rgba(8, 1, 1)),
    "png_rgba_37x23": _png(lambda: P.synth_rgba(37 * 7 + 23, 37, 23)),
    "png_rgba_64x64": _png(lambda: P.synth_rgba(64 * 7 + 64, 64, 64)),
    "png_rgba_300x300": _png(lambda: P.synth_rgba(300, 300, 300)),
    "png_merged_blocks": _pal(lambda: D._banded(1023, 768)),
    # ... the paths test_gpu_png_deflate.py steers
    "png_limiter_15": _pal(lambda: D.skewed(1, 511, 511, D.flat_and_tail())),
    "png_limiter_7": _pal(lambda: D.skewed(3, 511, 511, [2.0 ** -l for l, n in _CL_GROUPS for _ in range(n)], lead=True)),
    "png_no_match": _pal(lambda: D.noise(3, (60, 64))),
    "png_window_edge_32768": _pal(lambda: D._rows3(32767, 0, 40 + 32767)),
    "png_window_edge_32769": _pal(lambda: D._rows3(32767, 1, 40 + 32768)),
    "png_seam_joins": _pal(lambda: D._planted(5, 100, _JOINS)),
    "png_seam_cuts": _pal(lambda: D._const(127, 100)),
    "png_seam_cut_to_literals": _pal(lambda: D._planted(6, 100, _CUTS), seam="0"),
    # ... colour modes (pixel widths under a byte, two bytes)
    "png_pal16": _png(lambda: _colour_mode("pal16")),
    "png_grey1": _png(lambda: _colour_mode("grey1")),
    "png_grey_alpha": _png(lambda: _colour_mode("grey_alpha")),
    # EXR
    "exr_zip_33x17_rgb_half": _exr_golden("zip_33x17_rgb_half"),
    "exr_half_edges_64x16_rgba": _exr_golden("half_edges_64x16_rgba"),
    "exr_smooth_300x100": _exr(lambda: U.smooth(300, 100, 4, 320)),
    "exr_wide_4200x16": _exr(lambda: U.smooth(4200, 16, 4, 30)),
    "exr_flat_float": _exr(lambda: np.full((50, 200, 4), 0.25, np.float32)),
    "exr_flat_half": _exr(lambda: np.full((50, 200, 4), 0.25, np.float32), fp16=True),
    "exr_limiter_1.8": _exr(lambda: E.from_predictor_bytes(
        np.concatenate([E.flat_and_geometric_tail(65536, 64, 1.8, 1000, 50 + k) for k in range(2)]), 2048)),
    "exr_no_match": _exr(lambda: E.from_predictor_bytes(np.random.default_rng(51).integers(40, 200, 64 * 512), 512)),
    "exr_device_batch": _exr_batch,
}


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def test_case_list_is_the_pinned_one():
    if not RECORD:
        assert set(json.load(open(PIN))["cases"]) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_pinned_bytes(ctx, monkeypatch, name):
    data = CASES[name](ctx, monkeypatch)
    got = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
    print("deflate pin:", name, got)
    if RECORD:
        os.makedirs(os.path.dirname(PIN), exist_ok=True)
        pin = json.load(open(PIN)) if os.path.exists(PIN) else {}
        if pin.get("parent") != RECORD:
            pin = {"parent": RECORD, "cases": {}}
        pin["cases"][name] = got
        with open(PIN, "w") as f:
            json.dump(pin, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    pin = json.load(open(PIN))
    assert got == pin["cases"][name], (name, "differs from the bytes of", pin["parent"])
