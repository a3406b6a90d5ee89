"""include/imagecodecs/codecs.h: Image::read(".tga") / write(".tga") of the drop-in, compiled with
g++ against libicx.so (tests/cxx/tga_demo.cpp).

CPU: the demo builds and links; without a GPU read(".tga") throws std::runtime_error and
write(".tga") throws nothing and leaves lastWriteOk() false.
GPU: the reference's test.tga reads as 499 x 289 x 3 with the known SHA-256; read -> write ->
read gives identical pixels; the written file is the reference's 18 header bytes and the B,G,R
rows top-down."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import tgautil as T

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
SRC_TGA = os.path.join(GOLDEN, "tga", "test.tga")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "tga_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "tga_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_tga_never_falls_back(demo, tmp_path):
    """Without a GPU the read throws std::runtime_error and the write reports its failure (nothing
    thrown, no file written on the CPU); with one both succeed."""
    out, a = tmp_path / "t.tga", tmp_path / "a.bin"
    r = run(demo, "read", SRC_TGA, str(a))
    w = run(demo, "load", str(out))
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "read ok", r.stdout + r.stderr
        assert w.returncode == 0 and w.stdout.startswith("write ok") and out.read_bytes()[:3] == b"\0\0\2", w.stdout + w.stderr
    else:
        assert r.returncode == 1 and r.stdout.startswith("runtime_error: ") and "no HIP device" in r.stdout, r.stdout + r.stderr
        assert not a.exists()
        assert w.returncode == 1 and w.stdout.startswith("write failed") and "no HIP device" in w.stdout, w.stdout + w.stderr
        assert not out.exists()


@pytest.mark.gpu
def test_dropin_tga_read_fixture(demo, tmp_path):
    a = str(tmp_path / "a.bin")
    r = run(demo, "read", SRC_TGA, a)
    assert r.returncode == 0, r.stdout + r.stderr
    ra = open(a, "rb").read()
    assert tuple(np.frombuffer(ra[:16], np.int32)) == (499, 289, 3, 0)  # Type::UBYTE
    assert hashlib.sha256(ra[16:]).hexdigest() == T.FIXTURE_SHA256


@pytest.mark.gpu
def test_dropin_tga_round_trip(demo, tmp_path):
    out, a, b = str(tmp_path / "out.tga"), str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    r = run(demo, "copy", SRC_TGA, out, a, b)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    ra, rb = open(a, "rb").read(), open(b, "rb").read()
    assert ra == rb and len(ra) == 16 + 499 * 289 * 3
    px = np.frombuffer(ra[16:], np.uint8).reshape(289, 499, 3)
    written = open(out, "rb").read()
    assert written[:18] == bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 499 % 256, 499 // 256, 289 % 256, 289 // 256, 24, 0x20])
    assert written[18:] == px[:, :, ::-1].tobytes()


@pytest.mark.gpu
def test_dropin_tga_type_0_throws(demo, tmp_path):
    p = tmp_path / "none.tga"
    p.write_bytes(T.header(0, 4, 4, 24) + b"\0" * 48)
    r = run(demo, "read", str(p), str(tmp_path / "x.bin"))
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", r.stdout
