"""The TIFF write's contract without a GPU: the Python restatement (tests/tiffwutil.py) is read back
by PIL (libtiff) and by the read's restatement (tiffutil.decode); the C++ core
(imagecodecs_amd/csrc/icx_tiffw_core.h), compiled with g++ as a stand-alone program -- once plainly,
once with -fsanitize=address,undefined -- gives the restatement's header, arrays, IFD, LZW and
PackBits streams on the crafted inputs; icx_tiff_encode_bound refuses what the contract refuses and
bounds the restatement's files."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
import tiffutil as T
import tiffwutil as W

SRC = os.path.join(ROOT, "tests", "cxx", "tiffw_core_demo.cpp")


def _img(seed, h, w, d, kind="smooth"):
    a = T.smooth(seed, h, w, d) if kind == "smooth" else T.noise(seed, h, w, d)
    return a.reshape(h, w, d)


def _reads_back(f, a, name):
    code, w, h, d, px = T.decode(f)
    assert (code, w, h, d) == (T.OK, a.shape[1], a.shape[0], a.shape[2]), (name, code)
    np.testing.assert_array_equal(px, a, err_msg=str(name))
    np.testing.assert_array_equal(W.pil_pixels(f), a, err_msg="PIL " + str(name))


def test_restatement_reads_back_everywhere():
    """Every compression x legal predictor x d x rps in {0, 1, 2, h-1, h, h+5}, widths 1..21 x
    heights 1..9: PIL and tiffutil.decode read the restatement's file to the input's pixels. (The
    widths and heights alternate between the d and rps so that each pair is met with each.)"""
    n = 0
    for w in range(1, 22):
        for h in range(1, 10):
            for comp, pred in W.combos():
                d = (1, 3, 4)[(w + h + n) % 3]
                for rps in W.rps_set(h):
                    a = _img(w * 31 + h, h, w, d, "smooth" if (w + h) & 1 else "noise")
                    _reads_back(W.write_tiff(a, comp, pred, rps), a, (w, h, d, comp, pred, rps))
                    n += 1
    assert n > 5000


@pytest.mark.parametrize("d", (1, 3, 4))
def test_restatement_reads_back_every_d(d):
    for comp, pred in W.combos():
        for w, h in ((1, 1), (2, 9), (21, 9), (13, 4), (7, 5)):
            for rps in W.rps_set(h):
                a = _img(w + h, h, w, d)
                _reads_back(W.write_tiff(a, comp, pred, rps), a, (w, h, d, comp, pred, rps))


def test_layout_of_the_restatement():
    """The layout's words, on one file: data at 8, even strip offsets with a zero pad, arrays in
    tag order, the IFD last, nothing after it."""
    a = _img(3, 5, 3, 3, "noise")  # rows of 9 bytes: odd strips
    f = W.write_tiff(a, W.NONE, 1, 1)
    ifd = struct.unpack("<I", f[4:8])[0]
    ne = struct.unpack("<H", f[ifd:ifd + 2])[0]
    assert f[:4] == b"II*\0" and ne == 10 and len(f) == ifd + 2 + 12 * ne + 4 and f[-4:] == b"\0\0\0\0"
    H, pay = W.file_strips(f)
    assert H["offsets"] == [8, 18, 28, 38, 48] and H["counts"] == [9] * 5 and all(f[o + 9] == 0 for o in H["offsets"])
    tags = [struct.unpack("<H", f[ifd + 2 + 12 * e:][:2])[0] for e in range(ne)]
    assert tags == [256, 257, 258, 259, 262, 273, 277, 278, 279, 284]
    at = {t: struct.unpack("<I", f[ifd + 2 + 12 * e + 8:][:4])[0] for e, t in enumerate(tags)}
    assert (at[258], at[273], at[279], ifd) == (58, 64, 84, 104)
    f4 = W.write_tiff(_img(3, 2, 2, 4), W.LZW, 2, 0)
    ifd = struct.unpack("<I", f4[4:8])[0]
    assert [struct.unpack("<H", f4[ifd + 2 + 12 * e:][:2])[0] for e in range(12)][-2:] == [317, 338]


# ------------------------------------------------------------------------------ the C++ core
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def demo(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tiffw") / ("tiffw_core_demo_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True)
    return exe


def _core_file(demo, tmp_path, a, comp, pred, rps, payloads=None):
    a = np.asarray(a, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, d = a.shape
    px, out, pay = tmp_path / "px.bin", tmp_path / "out.tif", tmp_path / "pay.bin"
    px.write_bytes(a.tobytes())
    args = [demo, "file", str(w), str(h), str(d), str(comp), str(pred), str(rps), str(px), str(out)]
    if payloads is not None:
        pay.write_bytes(b"".join(struct.pack("<I", len(p)) + p for p in payloads))
        args.append(str(pay))
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr[-2000:])
    return out.read_bytes()


def test_core_equals_restatement_small(demo, tmp_path):
    """Header, arrays, IFD and payloads over d x compression x predictor x rps at small odd sizes;
    Deflate with zlib's payloads handed in."""
    for d in (1, 3, 4):
        for comp, pred in W.combos():
            for (w, h) in ((1, 1), (5, 3), (21, 9)):
                for rps in W.rps_set(h):
                    a = _img(d + w, h, w, d)
                    pays = None
                    if comp == W.DEFLATE:
                        r, _ = W.geometry(w, h, d, comp, pred, rps)
                        pays = [zlib.compress(s, 6) for s in W.strips_raw(a, pred, r)]
                    ref = W.write_tiff(a, comp, pred, rps, payloads=pays)
                    assert _core_file(demo, tmp_path, a, comp, pred, rps, pays) == ref, (d, comp, pred, w, h, rps)


def test_core_lzw_edges(demo, tmp_path):
    for name, a in W.lzw_edge_images():
        assert _core_file(demo, tmp_path, a, W.LZW, 1, 0) == W.write_tiff(a, W.LZW, 1, 0), name
    name, a = W.lzw_edge_images()[-2]
    assert _core_file(demo, tmp_path, a, W.LZW, 2, 64) == W.write_tiff(a, W.LZW, 2, 64), name


def test_core_packbits_edges(demo, tmp_path):
    for name, a in W.packbits_edge_images():
        for rps in (0, 1):
            assert _core_file(demo, tmp_path, a, W.PACKBITS, 1, rps) == W.write_tiff(a, W.PACKBITS, 1, rps), name


REFUSED = [
    (4, 4, 2, 1, 1, 0), (4, 4, 0, 1, 1, 0), (4, 4, 5, 1, 1, 0),          # d
    (0, 4, 3, 1, 1, 0), (4, 0, 3, 1, 1, 0), (-1, 4, 3, 1, 1, 0),         # width, height
    (4, 4, 3, 7, 1, 0), (4, 4, 3, 32946, 1, 0), (4, 4, 3, 0, 1, 0),      # compression
    (4, 4, 3, 1, 2, 0), (4, 4, 3, 32773, 2, 0), (4, 4, 3, 5, 3, 0), (4, 4, 3, 8, 0, 0),  # predictor
    (4, 4, 3, 1, 1, -1),                                                 # rows per strip
    (1, 4097, 1, 1, 1, 1), (1, 8194, 1, 5, 1, 2),                        # more than 4096 strips
    (32769, 32768, 1, 1, 1, 1 << 20),                                    # more than 2^30 pixels
    (1 << 29, 2, 4, 1, 1, 1),                                            # a strip of 2^31 bytes
    (1 << 15, 1 << 15, 4, 1, 1, 8),                                      # a file of 2^32 bytes
]
ACCEPTED = [(1, 4096, 1, 1, 1, 1), (1, 8192, 1, 5, 1, 2), (1 << 15, 1 << 15, 3, 1, 1, 8), (1, 1, 1, 8, 2, 0)]


def test_core_bound_refuses(demo):
    for args in REFUSED + ACCEPTED:
        r = subprocess.run([demo, "bound", *map(str, args)], capture_output=True, text=True, check=True)
        assert (int(r.stdout) == 0) == (args in REFUSED), (args, r.stdout)


def test_library_bound_refuses_and_bounds():
    """icx_tiff_encode_bound (host only): 0 for every refused set; at least the restatement's size
    on noise, zlib level 0 standing in for Deflate (stored blocks: the most a sane coder makes)."""
    import imagecodecs_amd as icx
    for args in REFUSED:
        assert icx.tiff_encode_bound(*args) == 0, args
    for args in ACCEPTED:
        assert icx.tiff_encode_bound(*args) > 0, args
    for d in (1, 3, 4):
        for comp, pred in W.combos():
            for (w, h) in ((1, 1), (7, 3), (21, 9), (300, 40), (4097, 3)):
                for rps in W.rps_set(h)[:4]:
                    a = _img(w + d, h, w, d, "noise")
                    size = len(W.write_tiff(a, comp, pred, rps, zlevel=0))
                    assert icx.tiff_encode_bound(w, h, d, comp, pred, rps) >= size, (d, comp, pred, w, h, rps)
            f = W.write_tiff(_img(1, 3, 7, d, "noise"), comp, pred, 0) if comp == W.NONE else None
            if f is not None:
                assert icx.tiff_encode_bound(7, 3, d, comp, pred, 0) == len(f)  # none: exact
