"""include/imagecodecs/codecs.h: Image::read(".gif") of the drop-in, compiled with g++ against
libicx.so (tests/cxx/gif_demo.cpp).

CPU: the demo builds and links; without a GPU read(".gif") throws std::runtime_error;
write(".gif") throws std::invalid_argument with or without one.
GPU: the reference's test.gif reads as 499 x 289 x 3 with the restatement's pixels; a file the
read refuses throws "Could not read image data"."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import gifutil as G

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
SRC_GIF = os.path.join(GOLDEN, "gif", "test.gif")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "gif_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "gif_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_dropin_gif_never_falls_back(demo, tmp_path):
    """Without a GPU the read throws std::runtime_error (no CPU decode takes over); with one it
    succeeds. write(".gif") throws std::invalid_argument either way and writes nothing."""
    out, a = tmp_path / "t.gif", tmp_path / "a.bin"
    r = run(demo, "read", SRC_GIF, str(a))
    w = run(demo, "write", str(out))
    assert w.returncode == 1 and w.stdout.splitlines()[0] == "invalid_argument: Cannot parse filetype", w.stdout + w.stderr
    assert not out.exists()
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "read ok", r.stdout + r.stderr
    else:
        assert r.returncode == 1 and r.stdout.startswith("runtime_error: ") and "no HIP device" in r.stdout, r.stdout + r.stderr
        assert not a.exists()


@pytest.mark.gpu
def test_dropin_gif_read_fixture(demo, tmp_path):
    a = str(tmp_path / "a.bin")
    r = run(demo, "read", SRC_GIF, a)
    assert r.returncode == 0, r.stdout + r.stderr
    ra = open(a, "rb").read()
    assert tuple(np.frombuffer(ra[:16], np.int32)) == (499, 289, 3, 0)  # Type::UBYTE
    assert ra[16:] == G.decode(open(SRC_GIF, "rb").read())[3].tobytes()


@pytest.mark.gpu
def test_dropin_gif_refused_file_throws(demo, tmp_path):
    names = dict((n, f) for n, f, _ in G.status_cases())
    for name in ("code_above_next", "cut_in_data", "no_palette"):
        p = tmp_path / (name + ".gif")
        p.write_bytes(names[name])
        r = run(demo, "read", str(p), str(tmp_path / "x.bin"))
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", (name, r.stdout)
