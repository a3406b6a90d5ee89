"""include/imagecodecs/codecs.h: Image::read(".bmp") and the public writeBmp(path) of the drop-in,
compiled with g++ against libicx.so (tests/cxx/bmp_demo.cpp). write()'s dispatch does not know
".bmp": earlier tests hold that write("x.bmp") throws std::invalid_argument, so files are written
by calling writeBmp.

CPU: the demo builds and links; without a GPU read(".bmp") throws std::runtime_error naming the
missing device and writeBmp throws nothing, leaves lastWriteOk() false and writes no file.
GPU: the reference's test.bmp reads as 499 x 289 x 3 UBYTE with the known SHA-256; read -> write ->
read gives identical pixels, and the written file equals the fixture except for bfSize, the
pels-per-metre fields and anything past the raster; d = 4 and d = 1 round trips keep their channels."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import bmputil as B

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
SRC_BMP = os.path.join(GOLDEN, "bmp", "test.bmp")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "bmp_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "bmp_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_bmp_never_falls_back(demo, tmp_path):
    """Without a GPU the read throws std::runtime_error and the write reports its failure (nothing
    thrown, no file written on the CPU); with one both succeed."""
    out, a = tmp_path / "t.bmp", tmp_path / "a.bin"
    r = run(demo, "read", SRC_BMP, str(a))
    w = run(demo, "load", str(out))
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "read ok", r.stdout + r.stderr
        assert w.returncode == 0 and w.stdout.startswith("write ok") and out.read_bytes()[:2] == b"BM", w.stdout + w.stderr
    else:
        assert r.returncode == 1 and r.stdout.startswith("runtime_error: ") and "no HIP device" in r.stdout, r.stdout + r.stderr
        assert not a.exists()
        assert w.returncode == 1 and w.stdout.startswith("write failed") and "no HIP device" in w.stdout, w.stdout + w.stderr
        assert not out.exists()


@pytest.mark.gpu
def test_dropin_bmp_read_fixture(demo, tmp_path):
    a = str(tmp_path / "a.bin")
    r = run(demo, "read", SRC_BMP, a)
    assert r.returncode == 0, r.stdout + r.stderr
    ra = open(a, "rb").read()
    assert tuple(np.frombuffer(ra[:16], np.int32)) == (499, 289, 3, 0)  # Type::UBYTE
    assert hashlib.sha256(ra[16:]).hexdigest() == B.FIXTURE_SHA256


@pytest.mark.gpu
def test_dropin_bmp_round_trip(demo, tmp_path):
    out, a, b = str(tmp_path / "out.bmp"), str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    r = run(demo, "copy", SRC_BMP, out, a, b)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    ra, rb = open(a, "rb").read(), open(b, "rb").read()
    assert ra == rb and len(ra) == 16 + 499 * 289 * 3
    written, fixture = bytearray(open(out, "rb").read()), bytearray(open(SRC_BMP, "rb").read())
    raster_end = 54 + 1500 * 289
    assert len(written) == raster_end and int.from_bytes(written[2:6], "little") == raster_end
    for buf in (written, fixture):
        buf[2:6] = bytes(4)     # bfSize
        buf[38:46] = bytes(8)   # biXPelsPerMeter, biYPelsPerMeter
    assert written == fixture[:raster_end]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [4, 1])
def test_dropin_bmp_channels_round_trip(demo, tmp_path, d):
    out = tmp_path / f"rt{d}.bmp"
    r = run(demo, "load", str(out), str(d))
    assert r.returncode == 0 and r.stdout.splitlines()[1] == f"21 5 {d} same", r.stdout + r.stderr
    px = (np.arange(21 * 5 * d) * 7).astype(np.uint8).reshape(5, 21, d)
    assert out.read_bytes() == B.encode(px)


@pytest.mark.gpu
def test_dropin_bmp_refused_file_throws(demo, tmp_path):
    p = tmp_path / "none.bmp"
    p.write_bytes(dict((n, f) for n, f, _ in B.error_cases())["jpeg"])
    r = run(demo, "read", str(p), str(tmp_path / "x.bin"))
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", r.stdout
