"""CPU tests of the inflate on crafted deflate streams (deflate_craft / inflate_corpus): what RFC
1951 allows and zlib's compressor never writes. The writer is checked against zlib's decoder; the
portable inflate (icx_exr_core.h exr_inflate, run by tests/emu in both window forms) must agree
with zlib on acceptance and on bytes, except for the leniencies of inf_build's miniz rule, each
asserted as such; and the wave inflate's parallel Adler-32 (adler_wave_lane / adler_wave_combine,
the functions the kernel calls) must equal zlib.adler32 up to the sizes where the sum of the lanes
no longer fits 64 bits."""
import ctypes as C
import zlib

import numpy as np
import pytest

import inflate_corpus as K
from test_exr_oracle import emu, emu_inflate


def zlib_inflate(z):
    try:
        return zlib.decompress(z)
    except zlib.error:
        return None


@pytest.mark.parametrize("name", sorted(K.GROUPS))
def test_writer_against_zlib(name):
    """zlib gives apply(tokens) for every stream built as valid, and refuses every other one (the
    lenient ones included: that is what makes them leniencies)."""
    for c in K.group(name):
        got = zlib_inflate(c.z)
        assert got == (None if c.lenient else c.full), c.name


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("name", sorted(K.GROUPS))
def test_portable_inflate(name, ring):
    """exr_inflate: the bytes of the construction with a capacity of exactly the size and of 100
    more, a refusal with one byte less, and a refusal of every invalid stream."""
    for c in K.group(name):
        if c.full is None:
            assert emu_inflate(c.z, 70000, ring) is None, c.name
            assert emu_inflate(c.z, c.need, ring) is None, c.name
            continue
        n = len(c.full)
        assert emu_inflate(c.z, n, ring) == c.full, c.name
        assert emu_inflate(c.z, n + 100, ring) == c.full, c.name
        if n:
            assert emu_inflate(c.z, n - 1, ring) is None, c.name
        if c.need < n:  # (a stream longer than the image: the capacity the reads pass)
            assert emu_inflate(c.z, c.need, ring) is None, c.name


@pytest.mark.parametrize("ring", [False, True])
def test_leniencies(ring):
    """zlib refuses, exr_inflate accepts with exactly these bytes: a literal/length or a distance
    code with one used symbol of two or more bits (zlib allows an incomplete code only as one
    symbol of one bit; inf_build, as miniz, with any single symbol), and a zlib header whose
    window size is above 32 KiB (only the method's bits are read). A change of either decoder in
    either direction fails here."""
    kinds = set()
    for c in K.group("leniencies"):
        assert c.lenient and zlib_inflate(c.z) is None, c.name
        assert emu_inflate(c.z, len(c.full), ring) == c.full, c.name
        kinds.add(next(k for k in ("one literal/length code", "one distance code", "CMF") if k in c.name))
    assert len(kinds) == 3
    # and the neighbours zlib accepts: one symbol of one bit, the largest legal window
    ok = [c for g in ("header_forms", "invalid_symbols", "zlib_headers") for c in K.group(g)
          if c.name in ("header: only EOB, 1 bit, no distance code", "symbol: the present code of a one-code distance table",
                        "zlib: CMF 0x78 FLG 0x9c")]
    assert len(ok) == 3
    for c in ok:
        assert zlib_inflate(c.z) == c.full and emu_inflate(c.z, len(c.full), ring) == c.full, c.name


# ------------------------------------------------------------------------------------ Adler-32
def adler_wave(buf: np.ndarray) -> int:
    L = emu()
    L.emu_adler_wave.restype = C.c_uint32
    L.emu_adler_wave.argtypes = [C.c_void_p, C.c_uint32]
    assert buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.ctypes.data % 4 == 0
    return L.emu_adler_wave(buf.ctypes.data, len(buf))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257, 4099, 70001])
def test_adler_wave_random(n):
    buf = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    assert adler_wave(buf) == zlib.adler32(buf.tobytes())


def test_adler_wave_large():
    """0xFF bytes: sum (out - p) b_p over all lanes is 255 out (out + 1) / 2, below 2^64 up to
    out = 380,368,696 and above it from the next byte on (the 64-bit sum of the lanes wrapped there
    and a valid stream of that size failed its check). 400,010,000 is a 10000 x 10000 RGBA PNG's
    filtered size; 2^30 - 1 is the largest output the wave inflate takes."""
    first_wrapped = 380_368_697
    assert 255 * (first_wrapped - 1) * first_wrapped // 2 < 1 << 64 <= 255 * first_wrapped * (first_wrapped + 1) // 2
    buf = np.full((1 << 30) - 1, 0xFF, np.uint8)
    for n in (first_wrapped, 400_010_000, (1 << 30) - 1):
        assert adler_wave(buf[:n]) == zlib.adler32(memoryview(buf)[:n]), n


def test_png_size_limit_is_below_the_adler_bound():
    """Why no PNG reaches that length: the read refuses more than 0x1000000 pixels (a 10000 x 10000
    file is TOO_LARGE at the chunk walk, before any inflate), and the most filtered bytes that limit
    allows, 2^24 rows of one 16-bit RGBA pixel, is 9 * 2^24."""
    import imagecodecs_amd as icx
    import pngread_util as R
    assert icx.png_probe(R.wrap(10000, 10000, 8, 6, zlib.compress(b"\0")))[0] == icx.PNGR_TOO_LARGE
    assert icx.png_probe(R.wrap(1, 1 << 24, 16, 6, zlib.compress(b"\0")))[0] == icx.PNGR_OK
    assert (1 << 24) * (1 + 8) < 380_368_697
