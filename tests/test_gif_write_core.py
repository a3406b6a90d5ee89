"""The GIF write's contract without a GPU: the Python restatement (tests/gifwutil.py) is read back by
PIL and by the read's restatement (gifutil.decode) over the grid the GPU test uses; the C++ core
(imagecodecs_amd/csrc/icx_gifw_core.h), compiled with g++ as a stand-alone program -- once plainly,
once with -fsanitize=address,undefined -- gives the restatement's bytes on the same grid;
icx_gif_encode_bound refuses what the contract refuses and bounds every file."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gifutil as G
import gifwutil as W

SRC = os.path.join(ROOT, "tests", "cxx", "gifw_core_demo.cpp")


def test_restatement_reads_back_over_the_grid():
    """PIL and gifutil.decode read every file of the shared corpus back to the palette's colours at
    the restatement's indices (for 256 colours or fewer: the input's own pixels)."""
    for case in W.corpus():
        name, a, seg, dither, mode = case
        W.reads_back(W.restated(case), a, dither, mode, name)
        if mode == W.AUTO and len(np.unique(W.rgb_of(a).reshape(-1, 3), axis=0)) <= 256:
            np.testing.assert_array_equal(W.expected_pixels(a), W.rgb_of(a), err_msg=name)


@pytest.mark.parametrize("m", (2, 3, 8))
def test_restatement_reads_back_rows(m):
    """1 x N, N = 1..600, whole and in segments of 64: the last code before a Clear or the stop
    code on every side of every width step."""
    for a in W.row_cases(m):
        for seg in (-1, 64):
            W.reads_back(W.write_gif(a, seg), a, name=(m, a.shape[1], seg), pil=a.shape[1] % 7 == 0)


def test_layout_of_the_restatement():
    """The container's words on one file: flags, table size, m, sub-block sizes, terminator, trailer."""
    a = W.image(5, 30, 40, 3, 5, "noise")  # 5 colours: tb = 3, m = 3
    f = W.write_gif(a, 64)
    assert f[:6] == b"GIF89a" and f[6:10] == bytes([40, 0, 30, 0]) and f[10] == (0x80 | 2 << 4 | 2) and f[11:13] == b"\0\0"
    table = np.frombuffer(f[13:13 + 24], np.uint8).reshape(8, 3).astype(np.int64)
    keys = table[:, 0] << 16 | table[:, 1] << 8 | table[:, 2]
    assert (np.diff(keys[:5]) > 0).all() and (keys[5:] == 0).all()
    at = 13 + 24
    assert f[at:at + 10] == b"," + bytes([0, 0, 0, 0, 40, 0, 30, 0, 0]) and f[at + 10] == 3
    p, sizes = at + 11, []
    while f[p]:
        sizes.append(f[p])
        p += 1 + f[p]
    assert len(sizes) >= 2 and all(s == 255 for s in sizes[:-1]) and 1 <= sizes[-1] <= 255
    assert f[p:] == b"\0;" and sum(sizes) == W.payload_size(a, 64)
    one = W.write_gif(np.full((1, 1, 1), 9, np.uint8))  # one colour: tb = 1, m = 2
    assert one[10] == 0x80 and one[13:19] == bytes([9, 9, 9, 0, 0, 0]) and one[19 + 10] == 2 and len(one) == 19 + 11 + 1 + 2 + 2
    # a payload of a multiple of 255 bytes: no empty sub-block before the terminator
    for case in W.corpus():
        if case[0].startswith(("payload255", "payload510")):
            f = W.restated(case)
            p, sizes = 13 + 3 * (1 << ((f[10] & 7) + 1)) + 11, []
            while f[p]:
                sizes.append(f[p])
                p += 1 + f[p]
            assert sizes == [255] * (len(sizes)) and len(sizes) in (1, 2) and f[p:] == b"\0;", case[0]


def test_corpus_meets_every_segment_alignment():
    """The segments' bit offsets in the shared corpus meet all eight residues mod 8: boundaries
    that share a byte between two segments (seven ways) and boundaries that do not."""
    seen = set()
    for name, a, seg, dither, mode in W.corpus():
        seen |= {o % 8 for o in W.segment_offsets(a, seg, dither, mode)[1:]}
    assert seen == set(range(8)), seen


# ------------------------------------------------------------------------------ the C++ core
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def demo(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gifw") / ("gifw_core_demo_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True)
    return exe


def _core_file(demo, tmp_path, a, seg, dither, mode):
    a = np.asarray(a, np.uint8)
    h, w, d = a.shape
    px, out = tmp_path / "px.bin", tmp_path / "out.gif"
    px.write_bytes(a.tobytes())
    r = subprocess.run([demo, "file", str(w), str(h), str(d), str(seg), str(dither), str(mode), str(px), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[:200], r.stderr[-2000:])
    return out.read_bytes(), [int(v) for v in r.stdout.splitlines()[1].split()]


def test_core_equals_restatement_over_the_grid(demo, tmp_path):
    for case in W.corpus():
        name, a, seg, dither, mode = case
        f, offs = _core_file(demo, tmp_path, a, seg, dither, mode)
        assert f == W.restated(case), name
        assert offs == W.segment_offsets(a, seg, dither, mode), name


def test_core_equals_restatement_rows(demo, tmp_path):
    for m in (2, 3, 8):
        for a in W.row_cases(m)[::3] + W.row_cases(m)[-40:]:
            for seg in (-1, 64):
                assert _core_file(demo, tmp_path, a, seg, 0, W.AUTO)[0] == W.write_gif(a, seg), (m, a.shape[1], seg)


# (w, h, d, segment_pixels, dither, palette_mode)
REFUSED = [
    (4, 4, 2, 0, 0, 0), (4, 4, 0, 0, 0, 0), (4, 4, 5, 0, 0, 0),              # d
    (0, 4, 3, 0, 0, 0), (4, 0, 3, 0, 0, 0), (-1, 4, 3, 0, 0, 0), (65536, 1, 3, 0, 0, 0), (1, 65536, 1, 0, 0, 0),  # width, height
    (4, 4, 3, 0, 2, 0), (4, 4, 3, 0, -1, 0),                                 # dither
    (4, 4, 3, 0, 0, 2), (4, 4, 3, 0, 0, -1),                                 # palette mode
    (4, 4, 3, 1, 0, 0), (4, 4, 3, 63, 0, 0), (4, 4, 3, -2, 0, 0), (300, 300, 1, 63, 0, 0),  # segment_pixels
    (32769, 32768, 1, 0, 0, 0), (65535, 65535, 3, -1, 0, 0),                 # more than 2^30 pixels
]
ACCEPTED = [(1, 1, 1, 0, 0, 0), (4, 4, 4, 64, 1, 1), (65535, 1, 3, -1, 0, 0), (1, 65535, 1, 1 << 30, 0, 1), (32768, 32768, 3, 0, 0, 0)]


def test_core_refuses(demo):
    for args in REFUSED + ACCEPTED:
        r = subprocess.run([demo, "args", *map(str, args)], capture_output=True, text=True, check=True)
        assert (r.stdout.strip() == "invalid") == (args in REFUSED), (args, r.stdout)
        w, h, _, seg, _, _ = args
        b = int(subprocess.run([demo, "bound", str(w), str(h), str(seg)], capture_output=True, text=True, check=True).stdout)
        assert b == W.bound(w, h, seg), args


def test_library_bound_refuses_and_bounds():
    """icx_gif_encode_bound (host only): 0 for every refused size or segment size, the contract's
    formula otherwise, and at least the size of every file of the corpus."""
    import imagecodecs_amd as icx
    for w, h, _, seg, _, _ in REFUSED + ACCEPTED:
        assert icx.gif_encode_bound(w, h, seg) == W.bound(w, h, seg), (w, h, seg)
    assert icx.gif_encode_bound(4, 4, 63) == 0 and icx.gif_encode_bound(0, 4, 0) == 0 and icx.gif_encode_bound(4, 4, 64) > 0
    worst = 0.0
    for case in W.corpus():
        name, a, seg, _, _ = case
        b = icx.gif_encode_bound(a.shape[1], a.shape[0], seg)
        assert b >= len(W.restated(case)), name
        if a.shape[0] * a.shape[1] > 4000:
            worst = max(worst, len(W.restated(case)) / b)
    assert worst > 0.5  # (the bound is not idle: noise of 256 colours comes close to it)
    assert icx.GIF_INVALID_ARGUMENT == 7 == W.INVALID_ARGUMENT
