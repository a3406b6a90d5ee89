"""The TIFF write's contract (include/icx.h, "TIFF write") restated in Python, independently of the
C++ core: write_tiff builds the whole file from the pixels; for Deflate it takes the strips'
payloads as given, so that everything around them is checked byte for byte. The LZW and PackBits
streams are tiffutil's (lzw_encode reproduces libtiff's bytes), the reader is tiffutil.decode."""
import struct
import zlib

import numpy as np

from tiffutil import lzw_encode, packbits_encode, decode, parse  # noqa: F401 (decode, parse: for the tests)

NONE, LZW, DEFLATE, PACKBITS = 1, 5, 8, 32773
COMPS = (NONE, LZW, DEFLATE, PACKBITS)
INVALID_ARGUMENT, TOO_LARGE = 8, 7
MAX_STRIPS = 4096


def legal(comp, pred):
    return comp in COMPS and (pred == 1 or (pred == 2 and comp in (LZW, DEFLATE)))


def combos():
    """Every compression x legal predictor."""
    return [(c, p) for c in COMPS for p in (1, 2) if legal(c, p)]


def rps_set(h):
    return sorted({r for r in (0, 1, 2, h - 1, h, h + 5) if r >= 0})


def geometry(w, h, d, comp, pred, rps):
    """(rps clamped, strips) or None for arguments the contract refuses (the 2^32 bound aside)."""
    if d not in (1, 3, 4) or w < 1 or h < 1 or rps < 0 or not legal(comp, pred) or w * h > 1 << 30:
        return None
    r = h if rps == 0 or rps > h else rps
    n = -(-h // r)
    if n > MAX_STRIPS or w * d * r >= 1 << 31:
        return None
    return r, n


def strips_raw(arr, pred, r):
    """The (differenced) bytes of each strip."""
    a = np.asarray(arr, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    if pred == 2:
        a = np.concatenate([a[:, :1], (a[:, 1:].astype(np.int16) - a[:, :-1]).astype(np.uint8)], axis=1)
    return [a[y:y + r].tobytes() for y in range(0, a.shape[0], r)]


def payload(raw, comp, row_bytes, zlevel=6):
    if comp == NONE:
        return raw
    if comp == LZW:
        return lzw_encode(raw)
    if comp == PACKBITS:
        return packbits_encode(raw, row_bytes)
    return zlib.compress(raw, zlevel)


def write_tiff(arr, comp, pred=1, rps=0, payloads=None, zlevel=6):
    """The file of the contract. payloads: the strips' data as given (Deflate: the writer's own)."""
    a = np.asarray(arr, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, d = a.shape
    r, n = geometry(w, h, d, comp, pred, rps)
    if payloads is None:
        payloads = [payload(s, comp, w * d, zlevel) for s in strips_raw(a, pred, r)]
    assert len(payloads) == n
    body = bytearray()
    offsets = []
    for p in payloads:
        offsets.append(8 + len(body))
        body += p
        if len(body) & 1:
            body += b"\0"
    counts = [len(p) for p in payloads]

    def array(fmt, values):
        at = 8 + len(body)
        assert at % 2 == 0
        body.extend(struct.pack("<%d%s" % (len(values), fmt), *values))
        return at

    S, L = 3, 4
    ent = [(256, L, 1, w), (257, L, 1, h),
           (258, S, d, 8 if d == 1 else array("H", [8] * d)),
           (259, S, 1, comp), (262, S, 1, 1 if d == 1 else 2),
           (273, L, n, offsets[0] if n == 1 else array("I", offsets)),
           (277, S, 1, d), (278, L, 1, r),
           (279, L, n, counts[0] if n == 1 else array("I", counts)),
           (284, S, 1, 1)]
    if pred == 2:
        ent.append((317, S, 1, 2))
    if d == 4:
        ent.append((338, S, 1, 2))
    ifd = 8 + len(body)
    assert ifd % 2 == 0 and [e[0] for e in ent] == sorted(e[0] for e in ent)
    out = b"II*\0" + struct.pack("<I", ifd) + bytes(body) + struct.pack("<H", len(ent))
    for tag, typ, count, value in ent:
        out += struct.pack("<HHII", tag, typ, count, value)
    return out + struct.pack("<I", 0)


def file_strips(f):
    """(head, [payload bytes of each strip]) of a file of ours, from its own arrays."""
    code, H = parse(f)
    assert code == 0, code
    return H, [f[o:o + c] for o, c in zip(H["offsets"], H["counts"])]


def pil_pixels(f):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    a = np.asarray(im)
    return a if a.ndim == 3 else a[:, :, None]


def _kernel_constant(name):
    """A constexpr int of imagecodecs_amd/csrc/icx_tiffw.hip, read from the source."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "imagecodecs_amd", "csrc", "icx_tiffw.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


PB_TILE = _kernel_constant("kPbTile")  # positions a wave of k_tiffw_pb takes per step
PB_LONG_ROW = 16 * PB_TILE - 24        # a row of many tiles, not a multiple of the tile

LZW_EDGE_LENGTHS = (253, 254, 255, 256, 765, 766, 767, 768, 1789, 1790, 1791, 1792, 3835, 3836, 3837, 3838, 3839, 3840,
                    7676)


def lzw_edge_images():
    """(name, (h, w) uint8): one-strip grey images whose streams put the strip's end and the EOI on
    each width step and on both sides of the forced Clear; 17 Clears; long strings with a full
    table; string lengths 1, 2, 3 ..."""
    ab = np.frombuffer(ab_sequence(), np.uint8)
    out = [("ab_%d" % n, ab[:n].reshape(1, n).copy()) for n in LZW_EDGE_LENGTHS]
    out.append(("ab_all", ab.reshape(255, 256).copy()))
    out.append(("two_level", (np.random.default_rng(5).integers(0, 2, (256, 256)) * 200).astype(np.uint8)))
    out.append(("all_equal", np.full((256, 256), 77, np.uint8)))
    return out


def _lits(n, seed=0):
    """n bytes, no two neighbours equal, none equal to 250..255 (the runs' values)."""
    return [(seed + 3 * i) % 250 for i in range(n)]


def packbits_edge_images():
    """(name, (h, w) uint8) grey images for the packer's edges: runs of each critical length at a
    row's start, middle and end, the same byte continuing over a row end, literal stretches around
    128 and 256, a 2-run between literals, rows of 1 and 2 bytes, rows of 16 PB_TILE less 24 bytes and more."""
    out = []
    for L in (1, 2, 3, 127, 128, 129, 130, 131, 256, 257, 258):
        for where in ("start", "middle", "end"):
            a, b = {"start": (0, 7), "middle": (5, 6), "end": (9, 0)}[where]
            row0 = _lits(a) + [255] * L + _lits(b, 1)
            # the second row starts with the byte the first ends with, and ends in a run of its own
            row1 = [row0[-1]] * 2 + _lits(len(row0) - 5, 2) + [251] * 3
            out.append(("run%d_%s" % (L, where), np.array([row0, row1, row0], np.uint8)))
    for L in (127, 128, 129, 257):
        row = [254] * 3 + _lits(L) + [253] * 4
        out.append(("lit%d" % L, np.array([row, row[::-1]], np.uint8)))
        out.append(("lit%d_whole_row" % L, np.array([_lits(L), _lits(L, 9)], np.uint8)))
    out.append(("two_run_between_literals", np.array([[1, 2, 3, 9, 9, 4, 5, 6], [9, 9, 1, 2, 3, 4, 8, 8]], np.uint8)))
    out.append(("rows_of_1", np.array([[5], [5], [6], [6], [6]], np.uint8)))
    out.append(("rows_of_2", np.array([[5, 5], [5, 6], [6, 6], [7, 8]], np.uint8)))
    n = PB_LONG_ROW
    rng = np.random.default_rng(11)
    out.append(("long_rows_mixed", np.repeat(rng.integers(0, 4, (3, n)), rng.integers(1, 4, n), axis=1).astype(np.uint8)))
    out.append(("long_row_one_run", np.full((2, n), 9, np.uint8)))
    return out


def ab_sequence():
    """a, b over all a < b <= 255: 65,280 bytes that repeat no byte pair, so greedy LZW emits one
    code per byte."""
    return bytes(v for a in range(256) for b in range(a + 1, 256) for v in (a, b))
