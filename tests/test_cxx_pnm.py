"""include/imagecodecs/codecs.h: Image::read / write of .pbm / .pgm / .ppm / .pnm / .pfm in the
drop-in, compiled with g++ against libicx.so (tests/cxx/pnm_demo.cpp).

CPU: the demo builds and links; without a GPU read(".ppm") throws std::runtime_error and a write
throws nothing and leaves lastWriteOk() false.
GPU: each fixture reads with the restatement's size, type and pixels, an upper-case name works, a P5
file named .pnm gives one channel, read -> write -> read is the identity for each of the five
extensions, write(".pfm") of UBYTE data throws the reference's message and write(".pgm") of an RGB
image only reports its failure."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import pnmutil as U

LIBDIR = os.path.join(ROOT, "imagecodecs_amd", "lib")
FIXTURE = {".pbm": "test.pbm", ".pgm": "test.pgm", ".ppm": "test.ppm", ".pnm": "test.pnm", ".pfm": "test_48rows.pfm"}


def _fixture(ext):
    return os.path.join(GOLDEN, "pnm", FIXTURE[ext])


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    import imagecodecs_amd as icx
    if not os.path.exists(icx.LIB_PATH):
        icx.build()
    exe = str(tmp_path_factory.mktemp("cxx") / "pnm_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "pnm_demo.cpp"), "-L" + LIBDIR, "-licx",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, timeout=300)


def _gpu():
    import torch
    return torch.cuda.is_available()


def _dumped(path):
    raw = open(path, "rb").read()
    return tuple(int(v) for v in np.frombuffer(raw[:16], np.int32)), raw[16:]


def test_dropin_pnm_never_falls_back(demo, tmp_path):
    """Without a GPU the read throws std::runtime_error and the write reports its failure (nothing
    thrown, no file written on the CPU); with one both succeed."""
    out, a = tmp_path / "t.ppm", tmp_path / "a.bin"
    r = run(demo, "read", _fixture(".ppm"), a)
    w = run(demo, "load", out, 3, 0)
    if _gpu():
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "read ok", r.stdout + r.stderr
        assert w.returncode == 0 and w.stdout.startswith("write ok") and out.read_bytes()[:14] == b"P6\n20 5\n255\n\x00\x07\x0e", w.stdout + w.stderr
    else:
        assert r.returncode == 1 and r.stdout.startswith("runtime_error: ") and "no HIP device" in r.stdout, r.stdout + r.stderr
        assert not a.exists()
        assert w.returncode == 1 and w.stdout.startswith("write failed") and "no HIP device" in w.stdout, w.stdout + w.stderr
        assert not out.exists()


def test_dropin_pnm_leaves_other_extensions_alone(demo, tmp_path):
    """.webp and .bmp still reach the unknown-extension branch, in both directions."""
    p = tmp_path / "x.webp"
    p.write_bytes(b"RIFF")
    r = run(demo, "read", p, tmp_path / "a.bin")
    assert r.returncode == 1 and r.stdout.startswith("invalid_argument: Cannot parse filetype"), r.stdout + r.stderr
    w = run(demo, "load", tmp_path / "x.bmp", 3, 0)
    assert w.returncode == 1 and w.stdout.startswith("invalid_argument: Cannot parse filetype"), w.stdout + w.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("ext", sorted(FIXTURE))
def test_dropin_pnm_read_fixture(demo, tmp_path, ext):
    ref = U.decode(open(_fixture(ext), "rb").read())
    a = tmp_path / "a.bin"
    r = run(demo, "read", _fixture(ext), a)
    assert r.returncode == 0, r.stdout + r.stderr
    head, px = _dumped(a)
    assert head == (ref[1], ref[2], ref[3], ref[4]) and px == ref[6].tobytes()


@pytest.mark.gpu
def test_dropin_pnm_names(demo, tmp_path):
    """An upper-case extension works, and the magic decides: a P5 file named .pnm has one channel."""
    data = open(_fixture(".pgm"), "rb").read()
    ref = U.decode(data)
    for name in ("X.PGM", "grey.pnm", "grey.ppm"):
        p = tmp_path / name
        p.write_bytes(data)
        a = tmp_path / (name + ".bin")
        r = run(demo, "read", p, a)
        assert r.returncode == 0, r.stdout + r.stderr
        head, px = _dumped(a)
        assert head == (499, 289, 1, 0) and px == ref[6].tobytes(), name
    bad = tmp_path / "cut.ppm"
    bad.write_bytes(open(_fixture(".ppm"), "rb").read()[:5000])
    r = run(demo, "read", bad, tmp_path / "x.bin")
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Could not read image data", r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("ext", sorted(FIXTURE))
def test_dropin_pnm_round_trip(demo, tmp_path, ext):
    out, a, b = tmp_path / ("out" + ext), tmp_path / "a.bin", tmp_path / "b.bin"
    r = run(demo, "copy", _fixture(ext), out, a, b)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "write ok", r.stdout + r.stderr
    assert a.read_bytes() == b.read_bytes()
    head, px = _dumped(a)
    ref = U.decode(open(_fixture(ext), "rb").read())
    assert px == ref[6].tobytes()
    fmt = {".pbm": U.P4, ".pgm": U.P5, ".ppm": U.P6, ".pnm": U.P6, ".pfm": U.PF}[ext]
    assert out.read_bytes() == U.encode(ref[6], fmt)


@pytest.mark.gpu
def test_dropin_pnm_write_rules(demo, tmp_path):
    r = run(demo, "load", tmp_path / "x.pfm", 3, 0)  # UBYTE data
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "runtime_error: Cannot write non-float data to .pfm", r.stdout
    r = run(demo, "load", tmp_path / "x.pgm", 3, 0)  # an RGB image is not a PGM: nothing thrown
    assert r.returncode == 1 and r.stdout.startswith("write failed"), r.stdout + r.stderr
    assert not (tmp_path / "x.pgm").exists()
    px = bytes((i * 7) & 255 for i in range(20 * 5 * 4))
    r = run(demo, "load", tmp_path / "f.pfm", 1, 2)  # FLOAT through the five-argument load
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "f.pfm").read_bytes() == U.encode(np.frombuffer(px, np.float32).reshape(5, 20, 1), U.PF)
    r = run(demo, "load", tmp_path / "g.pnm", 1, 1)  # USHORT, d = 1: .pnm is written as P5
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "g.pnm").read_bytes() == U.encode(np.frombuffer(px[:200], np.uint16).reshape(5, 20, 1), U.P5)
