"""Test helpers for the PNG read: crafted files (any colour type / bit depth, a chosen filter type
per row, a chosen deflate level, IDAT split every k bytes) and the 16-bit oracle. Plain numpy +
zlib; nothing here uses the library under test. The forward filter is parallel (every predictor
reads original bytes), unlike the un-filter the decoder has to run."""
import struct
import zlib

import numpy as np

import pngutil as P

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(t: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xFFFFFFFF)


def ihdr(w, h, bd, ct, comp=0, flt=0, il=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bd, ct, comp, flt, il))


def geometry(w, bd, ct):
    """(row bytes lb, filter unit bw)"""
    bpp = CHANNELS[ct] * bd
    return (w * bpp + 7) // 8, max(1, bpp // 8)


def pack_rows(samples: np.ndarray, bd: int) -> np.ndarray:
    """(h, w, ch) integer samples -> (h, lb) uint8 row bytes as the file stores them."""
    h, w, ch = samples.shape
    if bd == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, w * ch * 2)
    if bd == 8:
        return samples.astype(np.uint8).reshape(h, w * ch)
    bits = ((samples.reshape(h, w, 1).astype(np.uint8) >> np.arange(bd - 1, -1, -1, dtype=np.uint8)) & 1).reshape(h, w * bd)
    return np.packbits(bits, axis=1)  # (the last byte's spare low bits are zero)


def forward_filter(rows: np.ndarray, bw: int, types) -> bytes:
    """rows (h, lb) -> the filtered stream: per row its type byte and lb filtered bytes."""
    h, lb = rows.shape
    x = rows.astype(np.int32)
    b = np.vstack([np.zeros((1, lb), np.int32), x[:-1]])
    a = np.hstack([np.zeros((h, bw), np.int32), x[:, :-bw]]) if lb > bw else np.zeros((h, lb), np.int32)
    c = np.hstack([np.zeros((h, bw), np.int32), b[:, :-bw]]) if lb > bw else np.zeros((h, lb), np.int32)
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    out = np.zeros((h, lb + 1), np.uint8)
    for y in range(h):
        t = int(types[y])
        out[y, 0] = t
        out[y, 1:] = (x[y] - pred[t][y] if t <= 4 else x[y]) & 255  # (t > 4: an illegal type byte, bytes as they are)
    return out.tobytes()


def wrap(w, h, bd, ct, z: bytes, plte=None, trns=None, split=0, iend=True, pre=b"") -> bytes:
    """The file around a zlib stream; split > 0: one IDAT per `split` bytes of it."""
    out = SIG + ihdr(w, h, bd, ct) + pre
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    step = split if split > 0 else max(1, len(z))
    for k in range(0, len(z), step):
        out += chunk(b"IDAT", z[k:k + step])
    return out + (chunk(b"IEND", b"") if iend else b"")


def make_png(samples: np.ndarray, bd: int, ct: int, types=None, level=6, **kw) -> bytes:
    h, w, _ = samples.shape
    lb, bw = geometry(w, bd, ct)
    rows = pack_rows(samples, bd)
    assert rows.shape == (h, lb)
    if types is None:
        types = [0] * h
    return wrap(w, h, bd, ct, zlib.compress(forward_filter(rows, bw, types), level), **kw)


def random_samples(rng, w, h, bd, ct, top=None) -> np.ndarray:
    return rng.integers(0, top if top is not None else 1 << bd, (h, w, CHANNELS[ct]), dtype=np.int64)


def filter_types(kind, h):
    """kind 0..4: that type on every row; "cycle": (3 + 7y) mod 5."""
    return [(3 + 7 * y) % 5 for y in range(h)] if kind == "cycle" else [int(kind)] * h


def decode_rgba16(data: bytes) -> np.ndarray:
    """16-bit files -> (h, w, 4) uint8 RGBA by the PNG specification's rules: the high byte of every
    sample; the tRNS key compared at 16 bits (PIL clips 16-bit grey to 255: the wrong yardstick)."""
    I = P.info(data)
    w, h, ct = I["w"], I["h"], I["colortype"]
    assert I["bitdepth"] == 16
    ch = CHANNELS[ct]
    rows = P.unfilter(zlib.decompress(I["idat"]), h, w * ch * 2, ch * 2)
    v = np.ascontiguousarray(rows).view(">u2").astype(np.int32).reshape(h, w, ch)
    out = np.zeros((h, w, 4), np.uint8)
    hi = (v >> 8).astype(np.uint8)
    if ct in (0, 4):
        out[..., 0] = out[..., 1] = out[..., 2] = hi[..., 0]
        out[..., 3] = hi[..., 1] if ct == 4 else 255
    else:
        out[..., :3] = hi[..., :3]
        out[..., 3] = hi[..., 3] if ct == 6 else 255
    if I["trns"] and ct in (0, 2):
        key = struct.unpack(">" + "H" * (len(I["trns"]) // 2), I["trns"])
        m = np.ones((h, w), bool)
        for k in range(ch):
            m &= v[..., k] == key[k]
        out[..., 3][m] = 0
    return out


def oracle(data: bytes) -> np.ndarray:
    return decode_rgba16(data) if P.info(data)["bitdepth"] == 16 else P.decode_rgba(data)
