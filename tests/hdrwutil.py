"""The Radiance .hdr write restated in Python (include/icx.h "Radiance .hdr write"), shared by the
CPU core test and the GPU tests. Nothing here is a port of icx_hdrw_core.h:

  * the mantissas come from math.frexp and integer shifts of the float's exact 53-bit significand,
  * the row packer works on maximal stretches of equal bytes (cut into 127s, short rests joined into
    literals of 128), not on the serial rule; `pack_plane_rule` is the rule as icx.h prints it, and
    the core test holds the two against each other,
  * `decode` restates decrunchHDR / oldDecrunchHDR (codecs.cpp:630-703) and gives the RGBE bytes.
"""
import itertools
import math

import numpy as np

OK, TOO_LARGE, INVALID_ARGUMENT, INTERNAL_ERR = 0, 5, 6, -1
FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.float32(1e-32))


def header(w: int, h: int) -> bytes:
    return b"#?RADIANCE\nSOFTWARE=GEGL\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)


def packed_width(w: int) -> bool:
    return 8 <= w <= 32767


def encode_bound(w: int, h: int, d: int, rle: bool) -> int:
    if d not in (3, 4) or w < 1 or h < 1 or w * h > 1 << 30:
        return 0
    if rle and packed_width(w):
        return len(header(w, h)) + h * (4 + 4 * (w + -(-w // 128)))
    return len(header(w, h)) + 4 * w * h


def mantissa(v: float, E: int) -> int:
    """min(255, floor(v * 2^(136 - E))) for finite v > 0; 255 for +inf; 0 for NaN, negatives, +-0."""
    if v != v or v <= 0:
        return 0
    if math.isinf(v):
        return 255
    f, e = math.frexp(v)          # v = f * 2^e, f in [0.5, 1)
    sig = int(f * (1 << 53))      # exact: f has at most 53 bits
    sh = e - 53 + 136 - E         # v * 2^(136 - E) = sig * 2^sh
    return min(255, sig << sh if sh >= 0 else sig >> -sh)


def exponent4(ef: float) -> int:
    if ef != ef:
        return 0
    if math.isinf(ef):
        return 255 if ef > 0 else 0
    return min(255, max(0, math.trunc(ef)))


def rgbe4(r, g, b, ef):
    E = exponent4(ef)
    return mantissa(r, E), mantissa(g, E), mantissa(b, E), E


def rgbe3(r, g, b):
    c = [0.0 if (v != v or v < 0) else FLT_MAX if math.isinf(v) else v for v in (r, g, b)]
    mx = max(c)
    if mx < TINY:
        return 0, 0, 0, 0
    _, e = math.frexp(mx)
    E = min(255, e + 128)
    return mantissa(c[0], E), mantissa(c[1], E), mantissa(c[2], E), E


def quantise_scalar(px: np.ndarray) -> np.ndarray:
    """float32 (h, w, d) -> the RGBE bytes (h, w, 4), pixel by pixel through rgbe4 / rgbe3."""
    px = np.asarray(px, np.float32)
    h, w, d = px.shape
    flat = px.reshape(-1, d).astype(np.float64).tolist()  # (binary32 values, exactly)
    fn = rgbe4 if d == 4 else rgbe3
    return np.array([fn(*p) for p in flat], np.uint8).reshape(h, w, 4)


def _mantissas(v: np.ndarray, E: np.ndarray) -> np.ndarray:
    """`mantissa` over arrays (v float64 holding binary32 values, E int64): the same frexp and shifts.
    sig >= 2^52 for every finite v > 0, so a left shift always passes 255."""
    pos = np.isfinite(v) & (v > 0)
    f, e = np.frexp(np.where(pos, v, 1.0))
    sig = (f * float(1 << 53)).astype(np.int64)
    sh = e.astype(np.int64) - 53 + 136 - E
    m = np.where(sh >= 0, 255, np.minimum(255, sig >> np.minimum(np.maximum(-sh, 0), 63)))
    return np.where(pos, m, np.where(v == np.inf, 255, 0))


def quantise(px: np.ndarray) -> np.ndarray:
    """float32 (h, w, d) -> the RGBE bytes (h, w, 4) the write must give (numpy form of rgbe4 /
    rgbe3; the core test holds it against quantise_scalar on the value lists)."""
    v = np.asarray(px, np.float32).astype(np.float64)
    d = v.shape[2]
    rgb = v[..., :3]
    if d == 4:
        ef = v[..., 3]
        E = np.where(np.isnan(ef), 0.0, np.clip(np.trunc(np.nan_to_num(ef, nan=0.0, posinf=255.0, neginf=0.0)), 0, 255)).astype(np.int64)
        dark = np.zeros(E.shape, bool)
    else:
        rgb = np.where(np.isnan(rgb) | (rgb < 0), 0.0, np.where(np.isinf(rgb), FLT_MAX, rgb))
        mx = rgb.max(axis=-1)
        dark = mx < TINY
        E = np.minimum(255, np.frexp(np.where(dark, 1.0, mx))[1].astype(np.int64) + 128)
    out = np.empty(v.shape[:2] + (4,), np.int64)
    out[..., :3] = _mantissas(rgb, E[..., None])
    out[..., 3] = E
    out[dark] = 0
    return out.astype(np.uint8)


def pack_plane(p: bytes) -> bytes:
    toks = []  # (repeat count, value) for runs, bytes for literal pieces
    for v, g in itertools.groupby(p):
        full, rest = divmod(sum(1 for _ in g), 127)
        toks += [(127, v)] * full
        if rest >= 4:
            toks.append((rest, v))
        elif rest:
            toks.append(bytes([v]) * rest)
    out, lit = bytearray(), bytearray()

    def flush():
        for o in range(0, len(lit), 128):
            out.append(len(lit[o:o + 128]))
            out.extend(lit[o:o + 128])
        lit.clear()

    for t in toks:
        if isinstance(t, bytes):
            lit.extend(t)
        else:
            flush()
            out.extend((128 + t[0], t[1]))
    flush()
    return bytes(out)


def pack_plane_rule(p: bytes) -> bytes:
    """The rule of include/icx.h, serial as printed."""
    w, i, out = len(p), 0, bytearray()
    while i < w:
        r = 1
        while r < min(127, w - i) and p[i + r] == p[i]:
            r += 1
        if r >= 4:
            out.extend((128 + r, p[i]))
            i += r
        else:
            k = i
            while k < w and k - i < 128 and not (k > i and k + 3 < w and p[k] == p[k + 1] == p[k + 2] == p[k + 3]):
                k += 1
            out.append(k - i)
            out.extend(p[i:k])
            i = k
    return bytes(out)


def encode_rgbe(q: np.ndarray, rle: bool) -> bytes:
    """The file of already quantised pixels (h, w, 4)."""
    h, w, _ = q.shape
    parts = [header(w, h)]
    for row in q:
        if rle and packed_width(w):
            parts.append(bytes((2, 2, w >> 8, w & 255)))
            parts += [pack_plane(row[:, c].tobytes()) for c in range(4)]
        else:
            parts.append(row.tobytes())
    return b"".join(parts)


def encode(px: np.ndarray, rle: bool) -> bytes:
    return encode_rgbe(quantise(px), rle)


def decode(data: bytes) -> np.ndarray:
    """readHdr's scanline loop over a well-formed file -> RGBE bytes (h, w, 4)."""
    assert data[:10] == b"#?RADIANCE"
    at = data.index(b"\n\n", 10) + 2
    end = data.index(b"\n", at)
    words = data[at:end].split()
    assert words[0] == b"-Y" and words[2] == b"+X"
    h, w = int(words[1]), int(words[3])
    pos = end + 1
    out = np.zeros((h, w, 4), np.uint8)

    def old(y, x0, pos):  # oldDecrunchHDR (:630-660)
        x, shift = x0, 0
        while x < w:
            px = data[pos:pos + 4]
            assert len(px) == 4
            pos += 4
            if px[0] == 1 and px[1] == 1 and px[2] == 1:
                n = px[3] << shift
                assert 0 < x and x + n <= w
                out[y, x:x + n] = out[y, x - 1]
                x += n
                shift += 8
            else:
                out[y, x] = list(px)
                x += 1
                shift = 0
        return pos

    for y in range(h):
        if not packed_width(w) or data[pos] != 2:
            pos = old(y, 0, pos)
            continue
        px = data[pos:pos + 4]
        if px[1] != 2 or px[2] & 128:  # (2, G, B, E) is pixel 0 (:679-683)
            out[y, 0] = list(px)
            pos = old(y, 1, pos + 4)
            continue
        pos += 4
        for c in range(4):  # :686-700
            x = 0
            while x < w:
                code = data[pos]
                pos += 1
                if code > 128:
                    n = code & 127
                    assert n and x + n <= w
                    out[y, x:x + n, c] = data[pos]
                    pos += 1
                else:
                    assert code and x + code <= w
                    out[y, x:x + code, c] = list(data[pos:pos + code])
                    pos += code
                    n = code
                x += n
    assert pos == len(data)
    return out


def ambiguous(q: np.ndarray) -> bool:
    """A flat file of these RGBE bytes is not read back as written (the property icx.h documents)."""
    w = q.shape[1]
    rep = ((q[..., 0] == 1) & (q[..., 1] == 1) & (q[..., 2] == 1)).any()
    first = packed_width(w) and ((q[:, 0, 0] == 2) & (q[:, 0, 1] == 2) & (q[:, 0, 2] < 128)).any()
    return bool(rep or first)


# ----------------------------------------------------------------------------------- inputs
def floats_of(rgbe: np.ndarray) -> np.ndarray:
    """The read's formula: v = m * 2^(E - 136), E as a float (exact in binary32)."""
    rgbe = np.asarray(rgbe, np.uint8)
    out = np.empty(rgbe.shape, np.float32)
    e = rgbe[..., 3].astype(np.int32) - 136
    for c in range(3):
        out[..., c] = np.ldexp(rgbe[..., c].astype(np.float64), e).astype(np.float32)
    out[..., 3] = rgbe[..., 3]
    return out


def rgbe_noise(seed: int, w: int, h: int) -> np.ndarray:
    """Seeded RGBE pixels with stretches of equal bytes per component and no ambiguous pixel: largest
    mantissa >= 128, as a real encoder writes them."""
    rng = np.random.default_rng(seed)
    q = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        for c in range(4):
            row = []
            while len(row) < w:
                n = int(rng.choice([1, 1, 2, 3, 4, 5, 9, 40, 127, 128, 131, 260]))
                v = int(rng.integers(100, 140)) if c == 3 else int(rng.integers(0, 256))
                row += [v] * n if rng.random() < 0.5 else [int(x) for x in rng.integers(0, 256, n)]
            q[y, :, c] = row[:w]
    q[..., 3] = np.clip(q[..., 3], 100, 140)
    q[..., 0] |= 128
    return q


WIDTHS = (1, 7, 8, 9, 127, 128, 129, 130, 131, 255, 256, 300)
KNOWN_PLANES = {4: "84 v", 127: "ff v", 128: "ff v 01 v", 130: "ff v 03 v v v", 131: "ff v 84 v", 258: "ff v ff v 84 v"}


def known_plane(w: int, v: int) -> bytes:
    return bytes(v if t == "v" else int(t, 16) for t in KNOWN_PLANES[w].split())


def stretch_planes():
    """Planes with a stretch of 3, 4, 126..131, 254..258 equal bytes at the row start, middle and end."""
    rng = np.random.default_rng(77)
    out = []
    for L in (3, 4, 126, 127, 128, 129, 130, 131, 254, 255, 256, 257, 258):
        for where in ("start", "middle", "end"):
            w = L + 140
            p = rng.integers(0, 256, w, dtype=np.uint8)
            p[0::2] &= 0xFE  # (no stretch in the noise: neighbours differ in bit 0)
            p[1::2] |= 1
            a = {"start": 0, "middle": 71, "end": w - L}[where]
            p[a:a + L] = 6  # (even: differs from the odd byte before, if any)
            if a + L < w:
                p[a + L] = 9
            if a > 0:
                p[a - 1] = 9
            out.append((f"L{L}_{where}", p.tobytes()))
    return out


def _ulp(v: np.float32, up: bool) -> np.float32:
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf), dtype=np.float32)


SPECIALS = [0.0, -0.0, -1.5, float("nan"), float("inf"), float("-inf"), FLT_MAX, 1e-45, 1e-40, float(np.float32(1.17549421e-38)),
            float(np.float32(2 ** -126)), 1.0, 0.5, 255.0, 256.0]


def d4_inverse_pixels() -> np.ndarray:
    """Every E in 0..255 against mantissas 0, 1, 127, 128, 255 as the read's floats -> (256, 5, 4) RGBE."""
    q = np.zeros((256, 5, 4), np.uint8)
    m = (0, 1, 127, 128, 255)
    for E in range(256):
        for k in range(5):
            q[E, k] = (m[k], m[(k + 1) % 5], m[(k + 2) % 5], E)
    return q


def d4_value_pixels() -> np.ndarray:
    """(1, n, 4) floats: odd Ef values, special components, and values one ulp around mantissa steps."""
    px = []
    for ef in (-1.0, 0.9, 255.5, 256.0, 1e9, float("nan"), 128.0, 0.0, 9.0, 3.0):
        px.append((1.0, 0.75, 1e-3, ef))
        px.append((2.0 ** -140, 2.0 ** -135, 2.0 ** -128, ef))  # subnormals against small E
    for E in (0, 1, 8, 9, 100, 128, 136, 200, 255):
        for v in SPECIALS:
            px.append((v, 1.0, v, float(E)))
        for m in (1, 2, 128, 255, 256):
            step = np.ldexp(np.float64(m), E - 136).astype(np.float32)  # exact step, if representable
            px.append((float(_ulp(step, False)), float(step), float(_ulp(step, True)), float(E)))
    return np.array(px, np.float32).reshape(1, -1, 4)


def d3_value_pixels() -> np.ndarray:
    px = []
    for v in SPECIALS:
        px += [(v, 0.25, 0.5), (0.25, v, v), (v, v, v)]
    t = np.float32(1e-32)
    for mx in (_ulp(t, False), t, _ulp(t, True), np.float32(2.0 ** 127), _ulp(np.float32(2.0 ** 127), True),
               np.float32(FLT_MAX), np.float32(2.0 ** 126), _ulp(np.float32(2.0 ** 127), False)):
        mx = float(mx)
        px += [(mx, mx / 2, mx / 300), (mx / 3, mx, 0.0), (0.0, mx / 1e3, mx)]
    rng = np.random.default_rng(5)
    for _ in range(60):
        px.append(tuple(float(np.float32(10.0 ** rng.uniform(-20, 20))) for _ in range(3)))
    return np.array(px, np.float32).reshape(1, -1, 3)


_SHAPES = None


def shape_cases():
    """(name, float pixels (h, w, d)) over the width list at h = 1, 2, 3, both d; computed once."""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = []
        for w in WIDTHS:
            for h in (1, 2, 3):
                px = floats_of(rgbe_noise(300 + 7 * w + h, w, h))
                _SHAPES.append((f"d4_{w}x{h}", px))
                _SHAPES.append((f"d3_{w}x{h}", np.ascontiguousarray(px[..., :3])))
    return _SHAPES


_WIDE = None


def wide_cases(heights=(1, 2, 3)):
    """32767 (the widest run-length coded row) and 32768 (flat whatever rle says) at the given
    heights, both d; computed once."""
    global _WIDE
    if _WIDE is None:
        _WIDE = []
        for w in (32767, 32768):
            for h in (1, 2, 3):
                px = floats_of(rgbe_noise(w + h - 1, w, h))
                _WIDE += [(f"d4_{w}x{h}", px), (f"d3_{w}x{h}", np.ascontiguousarray(px[..., :3]))]
    return [c for c in _WIDE if c[1].shape[0] in heights]


_QUANTISED = {}


def quantised(name: str, px: np.ndarray) -> np.ndarray:
    """quantise(px), kept by the case's name: the reference is computed once and shared."""
    if name not in _QUANTISED:
        q = quantise(px)
        q.setflags(write=False)
        _QUANTISED[name] = q
    return _QUANTISED[name]
