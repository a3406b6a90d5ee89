"""include/imagecodecs/codecs.h: Image::writeGif of the drop-in, compiled with g++ against
libicx.so (tests/cxx/gif_write_demo.cpp).

CPU: the demo builds and links; without a GPU writeGif fails as writeTiff does, without writing a
file (no CPU encoder takes over); a USHORT image is refused with a message and writes nothing;
write(".gif") still throws std::invalid_argument.
GPU: writeGif with the defaults and with explicit arguments gives the restatement's bytes
(tests/gifwutil.py), which are those of icx_gif_save_to_file."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gifwutil as W

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "gif_write_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "gif_write_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_gif_write_never_falls_back(demo, tmp_path):
    a = W.image(1, 5, 20, 3, 7, "noise")
    px, out = tmp_path / "px.bin", tmp_path / "x.gif"
    px.write_bytes(a.tobytes())
    r = run(demo, "writeGif", px, 20, 5, 3, out)
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    else:
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "write failed" and "no HIP device" in r.stderr, r.stdout + r.stderr
        assert not out.exists()
    u = run(demo, "ushort", tmp_path / "u.gif")
    assert u.returncode == 0 and u.stdout.splitlines()[0] == "write failed", u.stdout + u.stderr
    assert "only UBYTE" in u.stderr and not (tmp_path / "u.gif").exists()
    w = run(demo, "write", tmp_path / "y.gif")
    assert w.returncode == 1 and w.stdout.splitlines()[0] == "invalid_argument: Cannot parse filetype", w.stdout + w.stderr
    assert not (tmp_path / "y.gif").exists()


@pytest.mark.gpu
def test_dropin_write_gif_equals_restatement(demo, tmp_path):
    many = W.many_colours(5, 7, 60, 3)
    for a, args in ((W.image(3, 7, 19, 3, 9, "noise"), ()), (W.image(1, 7, 19, 1, 200, "smooth"), (64, 0)),
                    (W.image(4, 7, 19, 4, 2, "flat"), (-1, 1)), (many, (128, 1)), (many, (0, 0))):
        h, w, d = a.shape
        px, out, ref = tmp_path / "px.bin", tmp_path / "x.gif", tmp_path / "ref.gif"
        px.write_bytes(a.tobytes())
        r = run(demo, "writeGif", px, w, h, d, out, *args)
        assert r.returncode == 0, r.stdout + r.stderr
        r = run(demo, "abi", px, w, h, d, ref, *(args or (0, 0)))
        assert r.returncode == 0, r.stdout + r.stderr
        f = out.read_bytes()
        seg, dither = args or (0, 0)
        assert f == W.write_gif(a, seg, dither), (d, args)
        assert f == ref.read_bytes(), (d, args)
        W.reads_back(f, a, dither)
