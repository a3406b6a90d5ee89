"""The TIFF read without a GPU: the restatement of tests/tiffutil.py against PIL / libtiff (the
reference's data/test.tif, PIL-written files, crafted tiled and MM files), the LZW writer against
libtiff's strip bytes, icx_tiff_probe's codes, and icx_tiff_core.h's serial decode through
tests/cxx/tiff_core_demo.cpp, built with g++ and again with -fsanitize=address,undefined as a
program of its own, over the crafted corpus."""
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import imagecodecs_amd as icx
import tiffutil as T

FIXTURE = open(os.path.join(GOLDEN, "tiff", "test.tif"), "rb").read()
FIXTURE_FILE_SHA256 = "49cf24f891f3665d608fb63a974e756f11050f9fccfa9f097b1278eb09a44268"
FIXTURE_SHA256 = "197f6b862531f4b81f313584cae00ba3ab2cdafe8ddccefb67ead15189d38b78"  # of PIL's 499 x 289 x 3 pixels


def _pil(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    if im.mode == "P":
        im = im.convert("RGB")
    a = np.asarray(im)
    return a[:, :, None] if a.ndim == 2 else a


def _pil_written():
    """(name, file, the array PIL was given as the restatement's output must show it)."""
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    rng = np.random.default_rng(11)
    out = []
    for comp in ("raw", "packbits", "tiff_lzw", "tiff_adobe_deflate"):
        for pred in (1, 2):
            for mode in ("L", "P", "RGB", "RGBA"):
                for strips in (False, True):
                    ch = {"L": 1, "P": 1, "RGB": 3, "RGBA": 4}[mode]
                    a = T.smooth(ch + pred, 33, 29, ch)
                    a = (a + rng.integers(0, 3, a.shape, dtype=np.uint8)).astype(np.uint8)
                    im = Image.fromarray(a, mode)
                    if mode == "P":
                        im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
                    info = {}
                    if pred == 2:
                        info[317] = 2
                    if strips:
                        info[278] = 4
                    b = io.BytesIO()
                    im.save(b, "TIFF", compression=comp, tiffinfo=info)
                    out.append((f"pil_{comp}_p{pred}_{mode}_{'s4' if strips else 'one'}", b.getvalue()))
    return out


def test_codes_match_the_header():
    assert (icx.TIFF_OK, icx.TIFF_NOT_TIFF, icx.TIFF_BAD_HEADER, icx.TIFF_UNSUPPORTED, icx.TIFF_MALFORMED, icx.TIFF_BAD_DATA,
            icx.TIFF_TRUNCATED, icx.TIFF_TOO_LARGE, icx.TIFF_INTERNAL_ERR) == (
                T.OK, T.NOT_TIFF, T.BAD_HEADER, T.UNSUPPORTED, T.MALFORMED, T.BAD_DATA, T.TRUNCATED, T.TOO_LARGE, T.INTERNAL_ERR)
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    for name, v in (("OK", 0), ("NOT_TIFF", 1), ("BAD_HEADER", 2), ("UNSUPPORTED", 3), ("MALFORMED", 4), ("BAD_DATA", 5),
                    ("TRUNCATED", 6), ("TOO_LARGE", 7), ("INTERNAL_ERR", -1)):
        assert f"ICX_TIFF_{name} = {v}," in src or f"ICX_TIFF_{name} = {v} " in src, name


def test_fixture_is_the_reference_file():
    assert len(FIXTURE) == 432901 and hashlib.sha256(FIXTURE).hexdigest() == FIXTURE_FILE_SHA256
    code, H = T.parse(FIXTURE)
    assert code == T.OK
    assert (H["w"], H["h"], H["spp"], H["comp"], H["photo"], H["ch"], H["nchunks"], H["tiled"]) == (499, 289, 3, 1, 2, 128, 3, False)
    code, w, h, d, px = T.decode(FIXTURE)
    assert (code, w, h, d) == (T.OK, 499, 289, 3)
    assert hashlib.sha256(px.tobytes()).hexdigest() == FIXTURE_SHA256
    assert hashlib.sha256(_pil(FIXTURE).tobytes()).hexdigest() == FIXTURE_SHA256


def test_restatement_equals_pil_on_pil_written_files():
    files = _pil_written()
    assert len(files) == 64
    seen = set()
    for name, data in files:
        code, H = T.parse(data)
        assert code == T.OK, name
        seen.add((H["comp"], H["pred"], H["photo"], H["nchunks"] > 1))
        if "_s4" in name:
            assert H["nchunks"] == 9 and H["ch"] == 4, name
        code, w, h, d, px = T.decode(data)
        assert code == T.OK and (w, h) == (29, 33), name
        np.testing.assert_array_equal(px, _pil(data), err_msg=name)
    assert {c for c, _, _, _ in seen} == {1, 5, 8, 32773}
    # the predictor is honoured under LZW and zlib only (libtiff stores plain samples otherwise)
    assert {(c, p) for c, p, _, _ in seen} == {(1, 1), (32773, 1), (5, 1), (5, 2), (8, 1), (8, 2)}


def test_restatement_equals_pil_on_crafted_files():
    """Tiles of 16 x 16 on 17 x 33 (clipped both ways), MM files, LONG and shuffled tags, odd chunk
    offsets: wherever PIL reads the file, it reads the restatement's pixels."""
    read = 0
    files = T.corpus()
    for comp in (1, 5, 8, 32773):
        for spp in (1, 3):
            files.append((f"tiled_{comp}_{spp}", T.make_tiff(T.smooth(2, 33, 17, spp), comp=comp, pred=2, tile=(16, 16), data_at=13)))
            files.append((f"mm_{comp}_{spp}", T.make_tiff(T.smooth(3, 9, 11, spp), comp=comp, be=True, rps=2, data_at=9)))
    for name, data in files:
        code, w, h, d, px = T.decode(data)
        assert code == T.OK, name
        if d == 4 or "miniswhite" in name or "32946" in name or "planar2" in name:
            continue  # (PIL premultiplies / keeps MinIsWhite as stored / refuses these)
        try:
            ref = _pil(data)
        except Exception:
            continue
        np.testing.assert_array_equal(px, ref, err_msg=name)
        read += 1
    assert read >= 40


def test_lzw_writer_equals_libtiff():
    """One strip of 97 x 131 noise: the widths step 9 -> 10 -> 11 -> 12 and libtiff clears at entry
    4094 several times. The writer's bytes are libtiff's; so the closed form is libtiff's rule."""
    Image = pytest.importorskip("PIL.Image")
    a = T.noise(30, 131, 97)
    b = io.BytesIO()
    Image.fromarray(a, "L").save(b, "TIFF", compression="tiff_lzw")
    data = b.getvalue()
    code, H = T.parse(data)
    assert code == T.OK and H["nchunks"] == 1 and H["comp"] == 5
    strip = data[H["offsets"][0]:H["offsets"][0] + H["counts"][0]]
    mine = T.lzw_encode(a.tobytes())
    assert len(strip) > 15000 and mine == strip
    assert T.lzw_decode(mine, a.size) == (T.OK, a.tobytes())
    flat = np.full((8, 200), 9, np.uint8)  # KwKwK runs
    b = io.BytesIO()
    Image.fromarray(flat, "L").save(b, "TIFF", compression="tiff_lzw")
    data = b.getvalue()
    code, H = T.parse(data)
    assert T.lzw_encode(flat.tobytes()) == data[H["offsets"][0]:H["offsets"][0] + H["counts"][0]]


def test_crafter_and_restatement_know_their_inputs():
    a = T.noise(50, 131, 97)
    raw = a.tobytes()
    for kw in ({}, {"eoi": False}, {"clear_every": 300}, {"clear_every": 1}):
        assert T.lzw_decode(T.lzw_encode(raw, **kw), len(raw)) == (T.OK, raw), kw
    assert T.lzw_decode(T.lzw_encode(raw, lead_clear=False), len(raw))[0] == T.BAD_DATA
    never = T.lzw_encode(raw, never_clear=True)
    assert T.lzw_decode(never, len(raw))[0] == T.BAD_DATA
    assert T.lzw_decode(never, 3000) == (T.OK, raw[:3000])  # (not before the table's end)
    assert T.decode(T.lzw_never_clear_file())[0] == T.BAD_DATA
    s, out = T.packbits_packets([("lit", b"a"), ("rep", 2, 7), ("nop",), ("lit", bytes(range(128))), ("rep", 128, 9)])
    assert T.packbits_decode(s, len(out)) == (T.OK, out)
    for name, data, want in T.status_cases():
        assert T.decode(data)[0] == want, name
    for name, data in T.corpus():
        assert T.decode(data)[0] == T.OK, name
    assert {c for _, _, c in T.status_cases()} == set(range(8))


def _all_files():
    base = T.base_file()
    files = [("fixture", FIXTURE)] + T.corpus() + [(n, f) for n, f, _ in T.status_cases()]
    files += [("never_clear", T.lzw_never_clear_file())]
    files += [(f"prefix{k}", base[:k]) for k in range(len(base) + 1)] + T.mutants(base)
    return files


def test_probe_codes():
    """The probe gives the walk's code (the chunks are the decode's), never a crash."""
    assert icx.tiff_probe(FIXTURE) == (icx.TIFF_OK, 499, 289, 3)
    seen = set()
    for name, data in _all_files():
        code, H = T.parse(data)
        seen.add(code)
        want = (code, H["w"], H["h"], H["d"]) if code == T.OK else (code, 0, 0, 0)
        assert icx.tiff_probe(data) == want, name
    assert seen == set(range(8)) - {T.BAD_DATA}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "tiff_core_demo.cpp"), "-lz", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "tiff_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "tiff_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_program(which, demo, demo_san, tmp_path):
    """icx_tiff_core.h's walk and serial decode over the fixture, the corpus, every status case,
    every prefix of one file and 200 mutants of it, each read from a buffer of exactly the file's
    size: code, size and pixels equal the restatement's. And the closed form for code offsets and
    widths against a reader that counts entries."""
    exe = demo if which == "plain" else demo_san
    files = _all_files()
    paths = []
    for k, (name, data) in enumerate(files):
        p = tmp_path / f"{k}.tif"
        p.write_bytes(data)
        paths.append(str(p))
    lines = []
    for q in range(0, len(paths), 500):
        r = subprocess.run([exe, "decode", *paths[q:q + 500]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines += r.stdout.splitlines()
    assert len(lines) == len(files)
    seen = set()
    for (name, data), line, p in zip(files, lines, paths):
        got = tuple(int(v) for v in line.split())
        code, w, h, d, px = T.decode(data)
        seen.add(code)
        assert got == (code, w, h, d), name
        if code == T.OK:
            assert open(p + ".px", "rb").read() == px.tobytes(), name
    assert seen == set(range(8))
    # the decoder's rule, entry by entry: widen when the next free entry is 2^w - 1
    want, off, width, nxt = [], 0, 9, 258
    for t in range(3900):
        want.append((off, width))
        off += width
        if t >= 1:
            nxt += 1
        if nxt >= (1 << width) - 1 and width < 12:
            width += 1
    r = subprocess.run([exe, "codes", "0", "3900"], capture_output=True, text=True, check=True)
    assert [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()] == want
    assert [T.code_width(t) for t in range(3900)] == [w for _, w in want]
