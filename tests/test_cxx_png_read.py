"""include/imagecodecs/codecs.h: Image::read(".png") of the drop-in, compiled with g++ against
libicx.so (tests/cxx/png_read_demo.cpp).

CPU: the demo builds and links; without a GPU the read throws (no CPU fallback).
GPU: the reference's test.png reads as 8-bit RGBA, bit-exact to tests/pngutil.decode_rgba; a damaged
file throws the reference's "Could not read image data"."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import pngutil as P

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
REF_PNG = os.path.join(GOLDEN, "png", "test.png")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "png_read_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "png_read_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def test_dropin_png_read_never_falls_back(demo, tmp_path):
    """With a GPU the read succeeds; without one it fails loudly instead of decoding on the CPU."""
    r = run(demo, REF_PNG, str(tmp_path / "t.bin"))
    line = r.stdout.splitlines()[0]
    assert (r.returncode == 0 and line == "read ok") or \
           (r.returncode == 1 and "runtime_error" in line and "no HIP device" in line), r.stdout + r.stderr


@pytest.mark.gpu
def test_dropin_png_read_bit_exact(demo, tmp_path):
    out = str(tmp_path / "t.bin")
    r = run(demo, REF_PNG, out)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    w, h, d, t = np.frombuffer(raw[:16], np.int32)
    assert (w, h, d, t) == (499, 289, 4, 0)  # Type::UBYTE
    assert raw[16:] == P.decode_rgba(open(REF_PNG, "rb").read()).tobytes()


@pytest.mark.gpu
def test_dropin_png_read_failure_message(demo, tmp_path):
    data = open(REF_PNG, "rb").read()
    cut = tmp_path / "cut.png"
    cut.write_bytes(data[: len(data) // 2])
    r = run(demo, str(cut), str(tmp_path / "t.bin"))
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", r.stdout
