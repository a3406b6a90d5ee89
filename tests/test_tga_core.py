"""The Targa read and write without a GPU: icx_tga_core.h (header walk, packet step, serial decode,
greedy row packer, header writer) through icx_tga_probe and through tests/cxx/tga_core_demo.cpp
(built with g++, and again with -fsanitize=address,undefined as a program of its own), against the
numpy restatement in tests/tgautil.py, the reference's data/test.tga and, where it imports, PIL."""
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import imagecodecs_amd as icx
import tgautil as T

FIXTURE = open(os.path.join(GOLDEN, "tga", "test.tga"), "rb").read()


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "tga_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "tga_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "tga_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def fixture_px():
    code, w, h, d, px = T.decode(FIXTURE)
    assert (code, w, h, d) == (T.OK, 499, 289, 3)
    return px


def test_codes_match_the_header():
    assert (icx.TGA_OK, icx.TGA_BAD_HEADER, icx.TGA_UNSUPPORTED, icx.TGA_NO_IMAGE, icx.TGA_MALFORMED, icx.TGA_TRUNCATED,
            icx.TGA_TOO_LARGE, icx.TGA_INVALID_ARGUMENT) == (T.OK, T.BAD_HEADER, T.UNSUPPORTED, T.NO_IMAGE, T.MALFORMED,
                                                             T.TRUNCATED, T.TOO_LARGE, T.INVALID_ARGUMENT)
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    for name, v in (("OK", 0), ("BAD_HEADER", 1), ("UNSUPPORTED", 2), ("NO_IMAGE", 3), ("MALFORMED", 4), ("TRUNCATED", 5),
                    ("TOO_LARGE", 6), ("INVALID_ARGUMENT", 7), ("INTERNAL_ERR", -1)):
        assert f"ICX_TGA_{name} = {v}," in src or f"ICX_TGA_{name} = {v} " in src, name


def test_fixture_is_the_reference_file(fixture_px):
    assert len(FIXTURE) == 11898 and hashlib.sha256(FIXTURE).hexdigest().startswith("0b457e12")
    assert FIXTURE[:18] == T.header(10, 499, 289, 24) and FIXTURE[-26:] == T.FOOTER
    assert hashlib.sha256(fixture_px.tobytes()).hexdigest() == T.FIXTURE_SHA256


def test_probe_fixture():
    assert icx.tga_probe(FIXTURE) == (icx.TGA_OK, 499, 289, 3)


@pytest.mark.parametrize("case", T.header_cases(), ids=lambda c: c[0])
def test_probe_crafted_headers(case):
    name, data, code = case
    got = icx.tga_probe(data)
    assert got[0] == code
    assert T.decode(data)[0] == code or (code == T.OK and data[2] >= 9)  # (RLE: the packets are the decode's)
    if code == T.OK:
        assert got[1:3] == (4, 4)
    else:
        assert got[1:] == (0, 0, 0)


def test_probe_valid_cases():
    for name, data, px in T.valid_cases():
        assert icx.tga_probe(data) == (icx.TGA_OK, px.shape[1], px.shape[0], px.shape[2]), name


def test_encode_bound():
    assert icx.tga_encode_bound(499, 289, 3) == 18 + 499 * 289 * 4 == T.encode_bound(499, 289, 3)
    assert icx.tga_encode_bound(65535, 65535, 4) == 18 + 65535 * 65535 * 5
    for w, h, d in ((0, 4, 3), (4, 0, 3), (65536, 1, 3), (1, 65536, 1), (4, 4, 2), (4, 4, 0), (4, 4, 5), (-1, 4, 3)):
        assert icx.tga_encode_bound(w, h, d) == 0


def test_restatement_knows_its_inputs():
    """The builder's pixels are what the restatement decodes, for every valid case."""
    for name, data, px in T.valid_cases():
        code, w, h, d, got = T.decode(data)
        assert code == T.OK and (got == px).all(), name
    for name, data in T.rle_shape_cases():
        assert T.decode(data)[0] == T.OK, name
    names = dict(T.edge_cases())
    for name, code in (("overshoot_last_packet", T.MALFORMED), ("overshoot_run_128", T.MALFORMED), ("mono_overshoot", T.MALFORMED),
                       ("cut_at_header_byte", T.TRUNCATED), ("cut_at_first_header_byte", T.TRUNCATED),
                       ("cut_in_run_pixel", T.TRUNCATED), ("cut_in_last_run_pixel", T.TRUNCATED),
                       ("cut_in_literal_payload", T.TRUNCATED), ("cut_in_last_literal", T.TRUNCATED),
                       ("cut_in_colour_map", T.TRUNCATED), ("cut_after_colour_map", T.TRUNCATED),
                       ("mono_run_then_missing", T.TRUNCATED), ("exact_end", T.OK), ("type_0", T.NO_IMAGE),
                       ("right_to_left", T.UNSUPPORTED)):
        assert T.decode(names[name])[0] == code, name


def test_restatement_equals_pil(fixture_px):
    Image = pytest.importorskip("PIL.Image")

    def pil(data):
        im = Image.open(io.BytesIO(data))
        im.load()
        return im

    im = pil(FIXTURE)
    assert im.mode == "RGB" and (np.asarray(im) == fixture_px).all()
    seen = 0
    for name, data, px in T.valid_cases():
        if "stray" in name or "unused_map" in name:
            continue  # (indices outside the map and an unused map are this contract's, not PIL's)
        try:
            im = pil(data)
        except Exception:
            continue  # (a form PIL does not read, e.g. 16-bit indices)
        want = {1: "L", 3: "RGB", 4: "RGBA"}[px.shape[2]]
        if im.mode == "P":
            im = im.convert(want)
        if im.mode != want:
            continue
        assert (np.asarray(im).reshape(px.shape) == px).all(), name
        seen += 1
    assert seen >= 12


def _demo_decode(exe, tmp_path, data):
    src, dst = tmp_path / "in.tga", tmp_path / "out.bin"
    src.write_bytes(data)
    r = subprocess.run([exe, "decode", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    code, w, h, d = (int(x) for x in r.stdout.split())
    return code, w, h, d, dst.read_bytes()


def _demo_pack(exe, tmp_path, px):
    h, w, d = px.shape
    src, dst = tmp_path / "px.bin", tmp_path / "pk.bin"
    src.write_bytes(px.tobytes())
    r = subprocess.run([exe, "pack", str(src), str(w), str(h), str(d), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dst.read_bytes()


def _pack_inputs():
    out = [T.synth(500 + w + d, w, 3, d) for w in (1, 2, 3, 127, 128, 129, 130, 257, 385) for d in (1, 3, 4)]
    out.append(np.full((2, 300, 3), 4, np.uint8))
    out.append(np.full((1, 257, 1), 4, np.uint8))  # two full runs and a single pixel
    alt = np.zeros((1, 300, 4), np.uint8)
    alt[0, ::2] = 9
    out.append(alt)
    mix = np.random.default_rng(1).integers(0, 256, (1, 400, 3), dtype=np.uint8)
    mix[0, 100:229] = 7  # 129 equal pixels inside noise: a run of 128 and a literal that joins the noise
    out.append(mix)
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_program(which, demo, demo_san, tmp_path, fixture_px):
    """The C++ core as a program of its own: serial decode == restatement on valid, shape and edge
    files; row packer == greedy restatement; the fixture's rows in file order pack to the fixture's
    own packet bytes; the header writer. The sanitized build runs the same inputs clean."""
    exe = demo if which == "plain" else demo_san
    files = [(n, f) for n, f, _ in T.valid_cases()] + T.rle_shape_cases() + T.edge_cases() + [("fixture", FIXTURE)]
    files.append(("tiled", T.tiled_case(4096)[0]))
    for name, data in files:
        code, w, h, d, px = T.decode(data)
        got = _demo_decode(exe, tmp_path, data)
        assert got[:4] == (code, w, h, d), name
        assert got[4] == (px.tobytes() if code == T.OK else b""), name
    for px in _pack_inputs():
        assert _demo_pack(exe, tmp_path, px) == b"".join(T.greedy_row(r) for r in px), px.shape
    assert _demo_pack(exe, tmp_path, np.ascontiguousarray(fixture_px[::-1])) == FIXTURE[18:11872]
    for w, h, d, rle in ((499, 289, 3, 0), (1, 65535, 4, 1), (300, 2, 1, 0), (300, 2, 1, 1)):
        r = subprocess.run([exe, "header", str(w), str(h), str(d), str(rle)], capture_output=True, text=True, check=True)
        hexs, bound = r.stdout.split()
        assert bytes.fromhex(hexs) == T.encode(np.zeros((h, w, d), np.uint8), bool(rle))[:18]
        assert int(bound) == T.encode_bound(w, h, d)


def test_greedy_restatement_reproduces_the_fixture(fixture_px):
    """The reference's file was not made by this project: packing its own pixels row by row with
    the greedy rule gives its 11,854 packet bytes."""
    assert T.encode(np.ascontiguousarray(fixture_px[::-1]), True)[18:] == FIXTURE[18:11872]
    assert len(FIXTURE[18:11872]) == 11854
