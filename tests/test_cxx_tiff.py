"""include/imagecodecs/codecs.h: Image::read(".tif" / ".tiff") of the drop-in, compiled with g++
against libicx.so (tests/cxx/tiff_demo.cpp).

CPU: the demo builds and links; without a GPU read(".tif") throws std::runtime_error;
write(".tif") throws std::invalid_argument with or without one.
GPU: the reference's test.tif, and a copy named .TIFF, read as 499 x 289 x 3 with PIL's pixels; a
file the read refuses throws "Could not read image data"."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import tiffutil as T

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
SRC_TIF = os.path.join(GOLDEN, "tiff", "test.tif")
PIL_SHA256 = "197f6b862531f4b81f313584cae00ba3ab2cdafe8ddccefb67ead15189d38b78"  # of PIL's 499 x 289 x 3 pixels of test.tif


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "tiff_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "tiff_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_tiff_never_falls_back(demo, tmp_path):
    """Without a GPU the read throws std::runtime_error (no CPU decode takes over); with one it
    succeeds. write(".tif") throws std::invalid_argument either way and writes nothing."""
    out, a = tmp_path / "x.tif", tmp_path / "a.bin"
    r = run(demo, "read", SRC_TIF, str(a))
    w = run(demo, "write", str(out))
    assert w.returncode == 1 and w.stdout.splitlines()[0] == "invalid_argument: Cannot parse filetype", w.stdout + w.stderr
    assert not out.exists()
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "read ok", r.stdout + r.stderr
    else:
        assert r.returncode == 1 and r.stdout.startswith("runtime_error: ") and "no HIP device" in r.stdout, r.stdout + r.stderr
        assert not a.exists()


@pytest.mark.gpu
def test_dropin_tiff_read_fixture(demo, tmp_path):
    copy = str(tmp_path / "copy.TIFF")
    shutil.copyfile(SRC_TIF, copy)
    for src in (SRC_TIF, copy):
        a = str(tmp_path / "a.bin")
        r = run(demo, "read", src, a)
        assert r.returncode == 0, r.stdout + r.stderr
        ra = open(a, "rb").read()
        assert tuple(np.frombuffer(ra[:16], np.int32)) == (499, 289, 3, 0)  # channels() == 3, Type::UBYTE
        assert hashlib.sha256(ra[16:]).hexdigest() == PIL_SHA256


@pytest.mark.gpu
def test_dropin_tiff_refused_file_throws(demo, tmp_path):
    names = dict((n, f) for n, f, _ in T.status_cases())
    for name in ("lzw_code_above_next", "chunk_past_file", "bps_16", "palette_without_map"):
        p = tmp_path / (name + ".tif")
        p.write_bytes(names[name])
        r = run(demo, "read", str(p), str(tmp_path / "x.bin"))
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", (name, r.stdout)
