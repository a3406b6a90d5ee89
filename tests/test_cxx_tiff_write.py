"""include/imagecodecs/codecs.h: Image::writeTiff of the drop-in, compiled with g++ against
libicx.so (tests/cxx/tiff_write_demo.cpp).

CPU: the demo builds and links; without a GPU writeTiff fails without writing a file (no CPU
encoder takes over); a USHORT image writes nothing; write(".tif") still throws
std::invalid_argument.
GPU: writeTiff with the defaults and with explicit arguments gives the bytes of
icx_tiff_save_to_file, which PIL reads back to the pixels."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import tiffutil as T
import tiffwutil as W

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "tiff_write_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "tiff_write_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_tiff_write_never_falls_back(demo, tmp_path):
    a = T.smooth(1, 5, 20, 3)
    px, out = tmp_path / "px.bin", tmp_path / "x.tif"
    px.write_bytes(a.tobytes())
    r = run(demo, "writeTiff", px, 20, 5, 3, out)
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    else:
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "write failed" and "no HIP device" in r.stderr, r.stdout + r.stderr
        assert not out.exists()
    u = run(demo, "ushort", tmp_path / "u.tif")
    assert u.returncode == 0 and u.stdout.splitlines()[0] == "write failed", u.stdout + u.stderr
    assert "only UBYTE" in u.stderr and not (tmp_path / "u.tif").exists()
    w = run(demo, "write", tmp_path / "y.tif")
    assert w.returncode == 1 and w.stdout.splitlines()[0] == "invalid_argument: Cannot parse filetype", w.stdout + w.stderr
    assert not (tmp_path / "y.tif").exists()


@pytest.mark.gpu
def test_dropin_write_tiff_equals_abi(demo, tmp_path):
    for d, args in ((3, ()), (1, (5, 2, 2)), (4, (32773, 1, 1)), (3, (8, 2, 3)), (1, (1, 1, 0))):
        a = T.smooth(d, 7, 19, d).reshape(7, 19, d)
        px, out, ref = tmp_path / "px.bin", tmp_path / "x.tif", tmp_path / "ref.tif"
        px.write_bytes(a.tobytes())
        r = run(demo, "writeTiff", px, 19, 7, d, out, *args)
        assert r.returncode == 0, r.stdout + r.stderr
        r = run(demo, "abi", px, 19, 7, d, ref, *(args or (8, 1, 0)))
        assert r.returncode == 0, r.stdout + r.stderr
        f = out.read_bytes()
        assert f == ref.read_bytes(), (d, args)
        np.testing.assert_array_equal(W.pil_pixels(f), a)
