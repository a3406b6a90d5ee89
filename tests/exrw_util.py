"""TEST INFRASTRUCTURE for the OpenEXR write: the seeded inputs, a numpy restatement of what
tinyexr's SaveEXR puts in a file (tinyexr.h:9333-9480, :7800-8024, :7184-7232, :1316-1422,
:989-1026), and the chunk-by-chunk comparison the GPU tests run.

The goldens under tests/golden/exrw (tools/make_exr_write_goldens.py) are tinyexr's own files for
the small cases; the restatement is pinned to them by tests/test_exr_write_core.py, and stands in
for tinyexr where a golden would be too large to commit.
"""
import json
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "exrw")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libref_exr.so")

# float bit patterns for float_to_half_full's branches: +-0, float denormals, results below /
# at / around the smallest half subnormal (2^-24) incl. the 2^-25 tie, the largest subnormal and
# the carry into the smallest normal half (2^-14), ties in the normal range (dropped bit 0x1000
# alone, with lower bits, and just under), the mantissa carry into the exponent, 65504, 65520
# (rounds to Inf), just under it, 1e6, +-Inf, NaNs (quiet, signalling with low bits only, negative)
HALF_EDGES = np.array([
    0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,
    0x33800000, 0x33000000, 0x32800000, 0x33000001, 0x337FFFFF, 0x33C00000, 0xB3800000,
    0x387FC000, 0x387FE000, 0x387FF000, 0x387FFFFF, 0x38800000, 0xB8800000, 0x38000000, 0x38001000,
    0x3F800000, 0x3F801000, 0x3F800FFF, 0x3F801001, 0x3F803000, 0x3F802000, 0xBF801000,
    0x3FFFF000, 0x3FFFEFFF, 0x40490FDB, 0x3E800000,
    0x477FE000, 0x477FF000, 0x477FEFFF, 0x47800000, 0xC77FF000, 0x49742400, 0xC9742400,
    0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00001, 0x7FFFFFFF,
], np.uint32)


def smooth(w, h, c, seed):
    """Seeded smooth data with a little noise: gradients and a slow wave per component."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.empty((h, w, c), np.float32)
    for k in range(c):
        a[:, :, k] = (0.25 * (k + 1) + x / max(1, w) + 0.5 * y / max(1, h)
                      + 0.125 * np.sin(0.05 * x * (k + 1) + 0.07 * y)).astype(np.float32)
    a += (rng.integers(0, 2, a.shape) * np.float32(2.0 ** -7)).astype(np.float32)
    return (np.round(a * 128) / 128).astype(np.float32)  # few mantissa bits: zlib gains on it


def random_bits(w, h, c, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (h, w, c), dtype=np.uint64).astype(np.uint32).view(np.float32)


def half_edge_image():
    return np.resize(HALF_EDGES, 64 * 16 * 4).reshape(16, 64, 4).view(np.float32)


# name -> (array builder, fp16): the cases with a committed tinyexr file
def golden_cases():
    return {
        "none_9x8_rgba": (lambda: smooth(9, 8, 4, 1), False),
        "none_15x15_rgb": (lambda: smooth(15, 15, 3, 2), False),
        "none_1x1_a": (lambda: smooth(1, 1, 1, 3), False),
        "zip_16x1_rgba": (lambda: smooth(16, 1, 4, 4), False),
        "zip_1x16_rgba": (lambda: smooth(1, 16, 4, 5), False),
        "zip_33x20_rgba": (lambda: smooth(33, 20, 4, 6), False),
        "zip_33x17_rgb_half": (lambda: smooth(33, 17, 3, 7), True),
        "zip_16x17_a": (lambda: smooth(16, 17, 1, 8), False),
        "raw_33x40_rgba": (lambda: random_bits(33, 40, 4, 9), False),
        "half_edges_64x16_rgba": (half_edge_image, True),
    }


def load_manifest():
    return json.load(open(os.path.join(GOLD, "manifest.json")))


def load_golden(name):
    """(float32 (h, w, c) input, fp16, tinyexr's file)."""
    m = load_manifest()[name]
    a = np.load(os.path.join(GOLD, m["input"]))
    return a, bool(m["fp16"]), open(os.path.join(GOLD, m["file"]), "rb").read()


# ---------------------------------------------------------------- the restatement
def half_full(bits):
    """float_to_half_full on uint32 bit patterns -> uint16."""
    f = np.asarray(bits, np.uint32).astype(np.int64)
    sign = (f >> 16) & 0x8000
    fe = (f >> 23) & 255
    fm = f & 0x7FFFFF
    newexp = fe - 127 + 15
    o = np.zeros_like(f)
    # normal
    n = (fe != 0) & (fe != 255) & (newexp > 0) & (newexp < 31)
    o = np.where(n, ((newexp << 10) | (fm >> 13)) + ((fm >> 12) & 1), o)
    # overflow
    o = np.where((fe != 0) & (fe != 255) & (newexp >= 31), 31 << 10, o)
    # underflow with a mantissa left
    u = (fe != 0) & (fe != 255) & (newexp <= 0) & (14 - newexp <= 24)
    sh = np.clip(14 - newexp, 14, 24)
    mant = fm | 0x800000
    o = np.where(u, ((mant >> sh) & 0x3FF) + ((mant >> (sh - 1)) & 1), o)
    # Inf / NaN
    o = np.where(fe == 255, (31 << 10) | np.where(fm != 0, 0x200, 0), o)
    return ((o & 0x7FFF) | sign).astype(np.uint16)


def half_to_float_bits(h):
    """The float bits a reader gets back from HALF samples (exact: numpy's float16 -> float32)."""
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float32).view(np.uint32)


def geometry(a, fp16):
    h, w, c = a.shape
    zipc = not (w < 16 and h < 16)
    return w, h, c, (2 if fp16 else 4), (16 if zipc else 1), zipc


def chunk_raw(a, fp16, k):
    """The sample bytes of chunk k: per line, per file channel (components reversed), w samples."""
    w, h, c, s, lines, _ = geometry(a, fp16)
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32)
    out = []
    for y in range(k * lines, min(h, (k + 1) * lines)):
        for ch in range(c):
            row = bits[y, :, c - 1 - ch]
            out.append(half_full(row).astype("<u2").tobytes() if fp16 else row.astype("<u4").tobytes())
    return b"".join(out)


def predict(raw):
    """CompressZip's reorder and predictor."""
    r = np.frombuffer(raw, np.uint8)
    t = np.concatenate([r[0::2], r[1::2]]).astype(np.int32)
    p = t.copy()
    p[1:] = (t[1:] - t[:-1] + 384) & 255
    return p.astype(np.uint8).tobytes()


def _attr(name, typ, data):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data


def header(a, fp16):
    w, h, c, s, _, zipc = geometry(a, fp16)
    names = {1: "A", 3: "BGR", 4: "ABGR"}[c]
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", 1 if fp16 else 2, 0, 1, 1) for n in names) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (b"\x76\x2f\x31\x01\x02\0\0\0" + _attr("channels", "chlist", chl)
            + _attr("compression", "compression", bytes([3 if zipc else 0]))
            + _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
            + _attr("lineOrder", "lineOrder", b"\0") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def nchunks(a, fp16):
    _, h, _, _, lines, _ = geometry(a, fp16)
    return (h + lines - 1) // lines


def split(a, fp16, data):
    """A file for input `a` -> (header bytes, [offsets], [(y, size, payload)]), walking the chunks
    where the container says they are: each follows the previous one, the first follows the table."""
    hdr = header(a, fp16)
    n = nchunks(a, fp16)
    got_hdr = data[: len(hdr)]
    offs = list(struct.unpack_from(f"<{n}Q", data, len(hdr)))
    at = len(hdr) + 8 * n
    chunks = []
    for k in range(n):
        y, size = struct.unpack_from("<ii", data, at)
        chunks.append((y, size, data[at + 8: at + 8 + size], at))
        at += 8 + size
    assert at == len(data), ("file length", at, len(data))
    return got_hdr, offs, chunks


def check_file(a, fp16, data, golden=None):
    """The parity contract on one file of ours: container bytes exact; each payload raw with
    size == S or a zlib stream shorter than S that inflates to the predictor bytes. With a golden,
    its container and inflated chunks must be the same. -> number of raw chunks."""
    w, h, c, s, lines, zipc = geometry(a, fp16)
    hdr = header(a, fp16)
    got_hdr, offs, chunks = split(a, fp16, data)
    assert got_hdr == hdr, "header bytes"
    nraw = 0
    gch = None
    if golden is not None:
        ghdr, goffs, gch = split(a, fp16, golden)
        assert ghdr == hdr, "golden header bytes"
    for k, (y, size, payload, at) in enumerate(chunks):
        assert offs[k] == at, ("offset table", k)
        assert y == k * lines, ("chunk y", k)
        raw = chunk_raw(a, fp16, k)
        S = len(raw)
        if not zipc or size == S:
            assert payload == raw, ("raw payload", k)
            nraw += 1
        else:
            assert size < S, ("stream not smaller than raw", k, size, S)
            assert payload[0] == 0x78 and (payload[0] * 256 + payload[1]) % 31 == 0, ("zlib header", k)
            d = zlib.decompressobj()
            inf = d.decompress(payload)
            assert d.eof and d.unused_data == b"", ("stream ends with the payload", k)
            assert inf == predict(raw), ("inflated bytes", k)
        if gch is not None:
            gy, gsize, gpay, _ = gch[k]
            assert gy == y
            graw = not zipc or gsize == S
            assert (gpay if graw else zlib.decompress(gpay)) == (raw if graw else predict(raw)), ("golden chunk", k)
    return nraw


def expected_readback(a, fp16):
    """The RGBA float bits LoadEXRFromMemory gives for the file of `a`: R, G, B, A by name (A = 1.0
    where the file has none); a one-channel file fills all four with its channel."""
    h, w, c = a.shape
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32)
    if fp16:
        bits = half_to_float_bits(half_full(bits))
    out = np.zeros((h, w, 4), np.uint32)
    one = np.float32(1.0).view(np.uint32)
    if c == 1:
        for k in range(4):
            out[:, :, k] = bits[:, :, 0]
    elif c == 3:
        out[:, :, :3] = bits
        out[:, :, 3] = one
    else:
        out[:] = bits
    return out
