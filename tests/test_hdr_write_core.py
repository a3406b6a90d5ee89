"""The Radiance .hdr write without a GPU: icx_hdrw_core.h (float -> RGBE for d = 4 and d = 3, header
writer, serial row packer, serial whole-file encode) through tests/cxx/hdrw_core_demo.cpp (built
with g++, and again with -fsanitize=address,undefined as a program of its own), against the
independent restatement in tests/hdrwutil.py. The restatement's decoder (decrunchHDR restated)
reads every file back to the quantised RGBE."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import hdrwutil as U


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "hdrw_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "hdrw_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "hdrw_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def core_encode(exe, tmp_path, jobs):
    """jobs: [(float pixels (h, w, d), rle)] -> [(file bytes, bound)] from one run of the program."""
    src, dst = tmp_path / "jobs.bin", tmp_path / "files.bin"
    with open(src, "wb") as f:
        for px, rle in jobs:
            h, w, d = px.shape
            f.write(struct.pack("<4i", w, h, d, int(rle)))
            f.write(np.ascontiguousarray(px, np.float32).tobytes())
    r = subprocess.run([exe, "encode", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob, at, out = dst.read_bytes(), 0, []
    for _ in jobs:
        size, bound = struct.unpack_from("<2Q", blob, at)
        out.append((blob[at + 16:at + 16 + size], bound))
        at += 16 + size
    assert at == len(blob)
    return out


def core_planes(exe, tmp_path, planes):
    src, dst = tmp_path / "planes.bin", tmp_path / "packed.bin"
    with open(src, "wb") as f:
        for p in planes:
            f.write(struct.pack("<i", len(p)))
            f.write(p)
    r = subprocess.run([exe, "planes", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob, at, out = dst.read_bytes(), 0, []
    for _ in planes:
        (n,) = struct.unpack_from("<i", blob, at)
        out.append(blob[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(blob)
    return out


def unpack_plane(b: bytes) -> bytes:
    out, at = bytearray(), 0
    while at < len(b):
        code = b[at]
        if code > 128:
            out += bytes([b[at + 1]]) * (code & 127)
            at += 2
        else:
            assert 1 <= code
            out += b[at + 1:at + 1 + code]
            at += 1 + code
    assert at == len(b)
    return bytes(out)


def _plane_inputs():
    planes = [(f"const_{w}", bytes([0x5A]) * w) for w in U.KNOWN_PLANES]
    planes += U.stretch_planes()
    rng = np.random.default_rng(11)
    for w in U.WIDTHS + (258, 1000, 32767):
        planes.append((f"noise_{w}", U.rgbe_noise(900 + w, w, 1)[0, :, 1].tobytes()))
        planes.append((f"few_{w}", rng.integers(0, 3, w, dtype=np.uint8).tobytes()))
    return planes


def test_restatement_known_answers_and_rule():
    """The stretch formulation gives the issue's known planes, equals the serial rule as icx.h prints
    it, unpacks to its input and stays within w + ceil(w/128)."""
    for w in U.KNOWN_PLANES:
        assert U.pack_plane(bytes([7]) * w) == U.known_plane(w, 7), w
    for name, p in _plane_inputs():
        got = U.pack_plane(p)
        assert got == U.pack_plane_rule(p), name
        assert unpack_plane(got) == p, name
        assert len(got) <= len(p) + -(-len(p) // 128), name


def test_restatement_inverts_the_read():
    """d = 4: the read's floats of every E against mantissas 0, 1, 127, 128, 255 quantise back to
    the same four bytes; d = 3: the largest mantissa is 128..255 unless E was clamped."""
    q = U.d4_inverse_pixels()
    assert (U.quantise(U.floats_of(q)) == q).all()
    # the numpy form of the restatement equals the scalar one, pixel by pixel
    for px in (U.floats_of(q), U.d4_value_pixels(), U.d3_value_pixels(), U.shape_cases()[-1][1], U.shape_cases()[-2][1]):
        assert (U.quantise(px) == U.quantise_scalar(px)).all()
    rng = np.random.default_rng(3)
    rgb = (10.0 ** rng.uniform(-20, 20, (1, 2000, 3))).astype(np.float32)
    got = U.quantise(rgb)
    assert (got[..., :3].max(axis=-1) >= 128).all() and got[..., 3].max() < 255


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_planes(which, demo, demo_san, tmp_path):
    exe = demo if which == "plain" else demo_san
    planes = _plane_inputs()
    got = core_planes(exe, tmp_path, [p for _, p in planes])
    for (name, p), g in zip(planes, got):
        assert g == U.pack_plane(p), name
    for w in U.KNOWN_PLANES:
        assert got[list(U.KNOWN_PLANES).index(w)] == U.known_plane(w, 0x5A), w


def _check_files(exe, tmp_path, cases, decode=True):
    jobs = [(px, rle) for _, px in cases for rle in (False, True)]
    files = core_encode(exe, tmp_path, jobs)
    k = 0
    for name, px in cases:
        q = U.quantised(name, px)
        h, w, d = px.shape
        for rle in (False, True):
            data, bound = files[k]
            k += 1
            assert data == U.encode_rgbe(q, rle), (name, rle)
            assert bound == U.encode_bound(w, h, d, rle) and len(data) <= bound, (name, rle)
            if not (rle and U.packed_width(w)):
                assert len(data) == bound == len(U.header(w, h)) + 4 * w * h, (name, rle)
            if decode and not (U.ambiguous(q) and not (rle and U.packed_width(w))):
                assert (U.decode(data) == q).all(), (name, rle)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_files_shapes(which, demo, demo_san, tmp_path):
    """Widths 1 .. 300, 32767 (the widest run-length coded row) and 32768 (flat whatever rle says),
    each at h = 1, 2, 3, d = 4 and d = 3, flat and run-length coded: the core's file == the
    restatement's, within the bound, and the restated decrunchHDR reads it back."""
    exe = demo if which == "plain" else demo_san
    cases = U.shape_cases() + U.wide_cases()
    assert {px.shape[:2] for _, px in U.wide_cases()} == {(h, w) for w in (32767, 32768) for h in (1, 2, 3)}
    for name, px in cases:
        assert not U.ambiguous(U.quantised(name, px)), name
    _check_files(exe, tmp_path, cases)
    for h in (1, 2, 3):
        assert U.encode_bound(32768, h, 4, True) == len(U.header(32768, h)) + 4 * 32768 * h
        assert U.encode_bound(32767, h, 3, True) == len(U.header(32767, h)) + h * (4 + 4 * (32767 + 256))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_files_values(which, demo, demo_san, tmp_path):
    """d = 4: every E x mantissas 0, 1, 127, 128, 255 come back as the same bytes; Ef -1, 0.9, 255.5,
    256, 1e9, NaN; components +-0, negative, NaN, +-inf, FLT_MAX, subnormals, one ulp around a
    mantissa step. d = 3: the same specials, mx around 1e-32f and in [2^127, 2^128)."""
    exe = demo if which == "plain" else demo_san
    inv = U.d4_inverse_pixels()
    cases = [("d4_inverse", U.floats_of(inv)), ("d4_values", U.d4_value_pixels()), ("d3_values", U.d3_value_pixels())]
    _check_files(exe, tmp_path, cases)
    data, _ = core_encode(exe, tmp_path, [(cases[0][1], False)])[0]
    assert data[len(U.header(5, 256)):] == inv.tobytes()  # the parity pin: epsilon = 0
    # spot values of the contract, written out
    assert U.rgbe4(1.0, 0.5, 0.0, 128.0) == (255, 128, 0, 128)
    assert U.rgbe4(1.0, 2.0 ** -149, -1.0, 0.9) == (255, 0, 0, 0)
    assert U.rgbe4(2.0 ** -136, 2.0 ** -137, float("inf"), 0.0) == (1, 0, 255, 0)
    assert U.rgbe3(1.0, 0.5, 0.25) == (128, 64, 32, 129)
    assert U.rgbe3(float("inf"), 0.0, float("nan")) == (255, 0, 0, 255)
    assert U.rgbe3(9e-33, 0.0, 0.0) == (0, 0, 0, 0)


def test_core_bound_program(demo):
    for w, h, d, rle in ((4, 4, 4, 0), (300, 2, 3, 1), (32767, 1, 4, 1), (32768, 1, 4, 1), (7, 5, 4, 1), (1 << 15, 1 << 15, 4, 0)):
        r = subprocess.run([demo, "bound", str(w), str(h), str(d), str(rle)], capture_output=True, text=True, check=True)
        bound, head = (int(x) for x in r.stdout.split())
        assert bound == U.encode_bound(w, h, d, bool(rle)) and head == len(U.header(w, h)), (w, h, d, rle)
    for w, h, d in ((0, 4, 4), (4, 0, 4), (-1, 4, 4), (4, 4, 2), (4, 4, 5), (4, 4, 1), (1 << 15, (1 << 15) + 1, 4)):
        r = subprocess.run([demo, "bound", str(w), str(h), str(d), "0"], capture_output=True, text=True, check=True)
        assert r.stdout.split()[0] == "0", (w, h, d)
