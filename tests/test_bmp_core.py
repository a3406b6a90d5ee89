"""The BMP read and write without a GPU: icx_bmp_core.h (header walk, mask helper, packet step, serial
decode, header and row writers) through icx_bmp_probe and through tests/cxx/bmp_core_demo.cpp (built
with g++, and again with -fsanitize=address,undefined as a program of its own), against the numpy
restatement in tests/bmputil.py, the reference's data/test.bmp and PIL."""
import hashlib
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import imagecodecs_amd as icx
import bmputil as B

FIXTURE = open(os.path.join(GOLDEN, "bmp", "test.bmp"), "rb").read()
KBMP_TILE = 4096  # icx_bmp.hip kBmpTile


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "bmp_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "bmp_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "bmp_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def corpus():
    """(name, file) of every shared case list, the fixture, prefixes and bit flips included."""
    files = [("fixture", FIXTURE)] + B.raw_cases() + B.offbits_cases() + B.header_cases() + B.palette_cases() + B.mask_cases()
    for rle in (8, 4):
        files += B.rle_shape_cases(rle) + B.edge_cases(rle, KBMP_TILE) + [(f"tiled{rle}", B.tiled_case(rle, KBMP_TILE))]
    files += [(n, f) for n, f, _ in B.error_cases()]
    for k, src in enumerate(B.fuzz_sources()):
        files += [(f"prefix{k}_{len(p)}", p) for p in B.prefixes(src)]
        files += [(f"flip{k}_{j}", p) for j, p in enumerate(B.bit_flips(src, 77 + k))]
    return files


@pytest.fixture(scope="module")
def expected(corpus):
    """The restatement's result for every file of the corpus, computed once."""
    return [B.decode(f) for _, f in corpus]


def test_codes_match_the_header():
    assert (icx.BMP_OK, icx.BMP_NOT_BMP, icx.BMP_BAD_HEADER, icx.BMP_UNSUPPORTED, icx.BMP_TRUNCATED, icx.BMP_TOO_LARGE,
            icx.BMP_INVALID_ARGUMENT, icx.BMP_INTERNAL_ERR) == (B.OK, B.NOT_BMP, B.BAD_HEADER, B.UNSUPPORTED, B.TRUNCATED,
                                                                 B.TOO_LARGE, B.INVALID_ARGUMENT, -1)
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    for name, v in (("OK", 0), ("NOT_BMP", 1), ("BAD_HEADER", 2), ("UNSUPPORTED", 3), ("TRUNCATED", 4), ("TOO_LARGE", 5),
                    ("INVALID_ARGUMENT", 6), ("INTERNAL_ERR", -1)):
        assert f"ICX_BMP_{name} = {v}," in src or f"ICX_BMP_{name} = {v} " in src, name


def test_fixture_is_the_reference_file():
    assert len(FIXTURE) == 433554 and struct.unpack_from("<iiHH", FIXTURE, 18) == (499, 289, 1, 24)
    code, w, h, d, px = B.decode(FIXTURE)
    assert (code, w, h, d) == (B.OK, 499, 289, 3)
    assert hashlib.sha256(px.tobytes()).hexdigest() == B.FIXTURE_SHA256
    ppm = open(os.path.join(GOLDEN, "pnm", "test.ppm"), "rb").read()
    assert ppm[-499 * 289 * 3:] == px.tobytes()


def test_probe_fixture():
    assert icx.bmp_probe(FIXTURE) == (icx.BMP_OK, 499, 289, 3)
    assert icx.bmp_probe(b"") == (icx.BMP_NOT_BMP, 0, 0, 0)


def test_probe_equals_restatement(corpus):
    """Size, channels and code of the host header walk, every file of the corpus."""
    for name, f in corpus:
        assert icx.bmp_probe(f) == B.probe(f), name


@pytest.mark.parametrize("case", B.error_cases(), ids=lambda c: c[0])
def test_error_cases_are_what_they_say(case):
    name, f, code = case
    assert B.decode(f)[0] == code
    want = code if not (code == B.TRUNCATED and name.startswith("rle")) else B.OK  # (the packets are the decode's)
    assert icx.bmp_probe(f)[0] == want


def test_encode_bound():
    assert icx.bmp_encode_bound(499, 289, 3) == len(FIXTURE) == B.encode_bound(499, 289, 3)
    assert icx.bmp_encode_bound(5, 2, 1) == 1078 + 16 and icx.bmp_encode_bound(5, 2, 4) == 122 + 40
    assert icx.bmp_encode_bound(65535, 65535, 4) == 122 + 4 * 65535 * 65535
    for w, h, d in ((0, 4, 3), (4, 0, 3), (65536, 1, 3), (1, 65536, 1), (4, 4, 2), (4, 4, 0), (4, 4, 5), (-1, 4, 3)):
        assert icx.bmp_encode_bound(w, h, d) == 0 == B.encode_bound(w, h, d)


def _pil(data):
    from PIL import Image  # (no skip: the comparison is part of what these tests check)
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_restatement_equals_pil():
    """On the forms PIL reads as the contract does. Every listed case must open: the lists are a
    condition on the form, not a tolerance."""
    cases = [("fixture", FIXTURE)] + B.pil_raw_cases() + B.pil_rle_cases()
    assert len(cases) == 1 + 340 + 16, len(cases)
    for name, f in cases:
        code, w, h, d, px = B.decode(f)
        assert code == B.OK, name
        a = np.asarray(_pil(f).convert({1: "L", 3: "RGB", 4: "RGBA"}[d]))
        assert (a.reshape(px.shape) == px).all(), name


def test_written_files_open_in_pil():
    for d in (1, 3, 4):
        for w in (1, 2, 3, 4, 5, 499):
            px = B.synth(10 * d + w, w, 3, d)
            im = _pil(B.encode(px))
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[d]
            assert (np.asarray(im).reshape(px.shape) == px).all(), (d, w)


def _demo_decode(exe, tmp_path, files):
    lines = []
    for k, f in enumerate(files):
        p = tmp_path / f"{k}.bmp"
        p.write_bytes(f)
        lines.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "decode", str(tmp_path / "list.txt"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    heads = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    return heads, (tmp_path / "out.bin").read_bytes()


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_program(which, demo, demo_san, tmp_path, corpus, expected):
    """The C++ core as a program of its own: serial decode == restatement on the whole corpus; the
    writers == the restatement's; composing cursor transforms is associative. The sanitized build
    runs the same inputs clean."""
    exe = demo if which == "plain" else demo_san
    heads, blob = _demo_decode(exe, tmp_path, [f for _, f in corpus])
    assert len(heads) == len(corpus)
    at = 0
    for (name, _), got, (code, w, h, d, px) in zip(corpus, heads, expected):
        assert got == (code, w, h, d), name
        if code == B.OK:
            assert blob[at:at + px.size] == px.tobytes(), name
            at += px.size
    assert at == len(blob)
    for d in (1, 3, 4):
        for w, h in ((1, 1), (2, 3), (3, 2), (4, 1), (5, 3), (499, 2)):
            px = B.synth(d + w, w, h, d)
            (tmp_path / "px.bin").write_bytes(px.tobytes())
            subprocess.run([exe, "write", str(tmp_path / "px.bin"), str(w), str(h), str(d), str(tmp_path / "w.bmp")], check=True)
            assert (tmp_path / "w.bmp").read_bytes() == B.encode(px), (w, h, d)
    r = subprocess.run([exe, "moves"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr


def test_writing_the_fixture_reproduces_it():
    """The restatement's writer on the fixture's pixels: the reference file's raster and header
    fields; bfSize and the pels-per-metre fields are where they may differ."""
    px = B.decode(FIXTURE)[4]
    out = B.encode(px)
    assert out[54:] == FIXTURE[54:54 + len(out) - 54] and len(out) == len(FIXTURE)
    for at, fmt in ((18, "<i"), (22, "<i"), (28, "<H"), (34, "<I")):  # biWidth, biHeight, biBitCount, biSizeImage
        assert struct.unpack_from(fmt, out, at) == struct.unpack_from(fmt, FIXTURE, at), at
