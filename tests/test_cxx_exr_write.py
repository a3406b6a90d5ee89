"""include/imagecodecs/codecs.h: Image::write(".exr") of the drop-in, compiled with g++ against
libicx.so (tests/cxx/exr_write_demo.cpp).

CPU: the demo builds and links; without a GPU the write fails loudly (lastWriteOk() false, the
library's error names the missing HIP device) and throws nothing, as the reference's writeExr.
GPU: read(.exr) -> write(.exr) -> read(.exr) gives the same floats; write(".bmp") still throws
std::invalid_argument."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
SRC_EXR = os.path.join(GOLDEN, "exr", "scan_zip_half.exr")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "exr_write_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "exr_write_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def test_dropin_exr_write_never_falls_back(demo, tmp_path):
    """With a GPU the write succeeds and leaves an OpenEXR file; without one it reports the
    failure (nothing thrown, no file written on the CPU)."""
    out = tmp_path / "t.exr"
    r = run(demo, "load", str(out))
    line = r.stdout.splitlines()[0]
    if r.returncode == 0:
        assert line.startswith("write ok") and out.read_bytes()[:4] == b"\x76\x2f\x31\x01", r.stdout + r.stderr
    else:
        assert r.returncode == 1 and line.startswith("write failed") and "no HIP device" in line, r.stdout + r.stderr
        assert "no HIP device" in r.stderr and not out.exists()


@pytest.mark.gpu
def test_dropin_exr_write_round_trip(demo, tmp_path):
    out, a, b = str(tmp_path / "out.exr"), str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    r = run(demo, "copy", SRC_EXR, out, a, b)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    ra, rb = open(a, "rb").read(), open(b, "rb").read()
    assert tuple(np.frombuffer(ra[:16], np.int32)) == (61, 37, 4, 2)  # Type::FLOAT
    assert ra == rb and len(ra) == 16 + 61 * 37 * 16
    # the written file: FLOAT samples, ZIP, four channels (a 331-byte header)
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import exrw_util as U
    px = np.frombuffer(ra[16:], np.float32).reshape(37, 61, 4)
    U.check_file(px, False, open(out, "rb").read())


@pytest.mark.gpu
def test_dropin_write_other_extension_still_throws(demo, tmp_path):
    r = run(demo, "bmp", SRC_EXR, str(tmp_path / "x.bmp"))
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "invalid_argument: Cannot parse filetype", r.stdout
