"""BMP as include/icx.h states it, restated in numpy and Python for the tests: a decoder written from
the contract's text (struct for the headers, a serial walk for the run-length streams), writers for
every form -- the crafted RLE4 / RLE8 streams the library itself never writes included -- and the
case lists the CPU and GPU tests share. Nothing here calls the library."""
import struct

import numpy as np

OK, NOT_BMP, BAD_HEADER, UNSUPPORTED, TRUNCATED, TOO_LARGE, INVALID_ARGUMENT = range(7)
FIXTURE_SHA256 = "197f6b862531f4b81f313584cae00ba3ab2cdafe8ddccefb67ead15189d38b78"  # of the 499 x 289 x 3 pixels
HEADER_SIZES = (12, 40, 52, 56, 64, 108, 124)
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 127, 128, 129, 395, 499)
HEIGHTS = (1, 2, 3, 17)
DEPTHS = (1, 4, 8, 16, 24, 32)
M555 = (0x7C00, 0x03E0, 0x001F)
M565 = (0xF800, 0x07E0, 0x001F)
M4444 = (0x0F00, 0x00F0, 0x000F, 0xF000)
M8888 = (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000)
M101010 = (0x3FF00000, 0x000FFC00, 0x000003FF)
M5551 = (0x7C00, 0x03E0, 0x001F, 0x8000)


# ------------------------------------------------------------------------------------ decode
def _field(m):
    """(shift, width) of a mask, or None when its set bits are not contiguous."""
    if m == 0:
        return 0, 0
    shift = (m & -m).bit_length() - 1
    v = m >> shift
    if v & (v + 1):
        return None
    return shift, v.bit_length()


def _scale(v, width):
    """Field values (numpy, uint64) -> 8 bits."""
    if width == 0:
        return np.zeros_like(v)
    if width > 8:
        return v >> np.uint64(width - 8)
    m = np.uint64((1 << width) - 1)
    return (v * np.uint64(510) + m) // (np.uint64(2) * m)


class Head:
    pass


def parse(data: bytes):
    """-> (code, Head or None), the checks in the contract's order."""
    n = len(data)
    if n < 18 or data[:2] != b"BM":
        return NOT_BMP, None
    offbits, hs = struct.unpack_from("<II", data, 10)
    if hs not in HEADER_SIZES or 14 + hs > n:
        return BAD_HEADER, None
    comp = used = 0
    if hs == 12:
        w, h, _, bits = struct.unpack_from("<HHHH", data, 18)
    else:
        w, h, _, bits, comp = struct.unpack_from("<iiHHI", data, 18)
        used, = struct.unpack_from("<I", data, 46)
    if w <= 0 or h == 0 or h == -2 ** 31 or bits not in DEPTHS:
        return BAD_HEADER, None
    if (comp == 1 and bits != 8) or (comp == 2 and bits != 4) or (comp in (3, 6) and bits not in (16, 32)):
        return BAD_HEADER, None
    if used > 2 ** bits:
        return BAD_HEADER, None
    extra = {3: 12, 6: 16}.get(comp, 0) if hs == 40 else 0
    if 14 + hs + extra > n:
        return BAD_HEADER, None
    H = Head()
    H.pal_at = 14 + hs + extra
    H.pal_es = 3 if hs == 12 else 4
    H.pal_n = (used or 2 ** bits) if bits <= 8 else 0
    pal_end = H.pal_at + (H.pal_n if bits <= 8 else used) * H.pal_es
    if offbits < pal_end:
        return BAD_HEADER, None
    if comp not in (0, 1, 2, 3, 6) or (hs == 64 and comp != 0) or (comp in (1, 2) and h < 0):
        return UNSUPPORTED, None
    H.w, H.h, H.flip, H.bits, H.ds = w, abs(h), h > 0, bits, offbits
    H.rle = {1: 8, 2: 4}.get(comp, 0)
    H.stride = (w * bits + 31) // 32 * 4
    masks = [0, 0, 0, 0]
    if bits in (16, 32):
        if comp in (3, 6):
            k = 4 if (hs >= 56 or (hs == 40 and comp == 6)) else 3  # a 52-byte header holds three
            masks[:k] = struct.unpack_from("<%dI" % k, data, 54)
        else:
            masks[:3] = M555 if bits == 16 else M8888[:3]
    H.fields = []
    seen = 0
    for m in masks:
        f = _field(m)
        if f is None or seen & m:
            return UNSUPPORTED, None
        seen |= m
        H.fields.append((m,) + f)
    H.d = 4 if masks[3] else 3
    if w * H.h > 2 ** 30:
        return TOO_LARGE, None
    if pal_end > n or offbits > n:
        return TRUNCATED, None
    if not H.rle and offbits + H.stride * H.h > n:
        return TRUNCATED, None
    H.pal = np.zeros((256, 3), np.uint8)  # R,G,B; zero at and past pal_n
    if bits <= 8:
        e = np.frombuffer(data, np.uint8, H.pal_n * H.pal_es, H.pal_at).reshape(H.pal_n, H.pal_es)
        H.pal[:H.pal_n] = e[:, 2::-1]
        if bits == 8 and (H.pal[:H.pal_n] == np.arange(H.pal_n, dtype=np.uint8)[:, None]).all():
            H.d = 1
    return OK, H


def probe(data: bytes):
    code, H = parse(data)
    return (code, H.w, H.h, H.d) if code == OK else (code, 0, 0, 0)


def _walk(data, H):
    """The packets of a run-length stream in walk order: (kind, pos, count) with kind 'run', 'lit',
    'eol', 'delta'; None when a packet is cut short."""
    n, pos, out = len(data), H.ds, []
    while pos + 2 <= n:
        a, b = data[pos], data[pos + 1]
        if a:
            out.append(("run", pos, a))
            pos += 2
        elif b == 0:
            out.append(("eol", pos, 0))
            pos += 2
        elif b == 1:
            break
        elif b == 2:
            if pos + 4 > n:
                return None
            out.append(("delta", pos, 0))
            pos += 4
        else:
            nb = b if H.rle == 8 else (b + 1) // 2
            nb += nb & 1
            if pos + 2 + nb > n:
                return None
            out.append(("lit", pos, b))
            pos += 2 + nb
    return out


def decode(data: bytes):
    """-> (code, w, h, d, uint8 (h, w, d) or None)."""
    code, H = parse(data)
    if code != OK:
        return code, 0, 0, 0, None
    w, h, d = H.w, H.h, H.d
    buf = np.frombuffer(data, np.uint8)
    if H.rle:
        packets = _walk(data, H)
        if packets is None:
            return TRUNCATED, 0, 0, 0, None
        idx = np.zeros((h, w), np.int64)  # bottom row first
        x = y = 0
        for kind, pos, count in packets:
            if kind == "eol":
                x, y = 0, y + 1
            elif kind == "delta":
                x, y = x + data[pos + 2], y + data[pos + 3]
            else:
                if kind == "run":
                    v = data[pos + 1]
                    vals = np.full(count, v) if H.rle == 8 else np.where(np.arange(count) & 1, v & 15, v >> 4)
                elif H.rle == 8:
                    vals = buf[pos + 2:pos + 2 + count].astype(np.int64)
                else:
                    b = buf[pos + 2:pos + 2 + (count + 1) // 2]
                    vals = np.stack([b >> 4, b & 15], 1).reshape(-1)[:count].astype(np.int64)
                if y < h and x < w:
                    k = min(count, w - x)
                    idx[y, x:x + k] = vals[:k]
                x += count
        px = H.pal[idx[::-1]]
        return OK, w, h, d, np.ascontiguousarray(px[:, :, :1] if d == 1 else px)
    rows = np.lib.stride_tricks.as_strided(buf[H.ds:], (h, H.stride), (H.stride, 1))
    if H.bits <= 8:
        per = 8 // H.bits
        sh = (per - 1 - np.arange(per)) * H.bits
        idx = ((rows[:, :, None] >> sh) & (2 ** H.bits - 1)).reshape(h, -1)[:, :w]
        px = H.pal[idx]
        if d == 1:
            px = px[:, :, :1]
    elif H.bits == 24:
        px = rows[:, :3 * w].reshape(h, w, 3)[:, :, ::-1]
    else:
        nb = H.bits // 8
        b = rows[:, :nb * w].reshape(h, w, nb).astype(np.uint64)
        v = sum(b[:, :, k] << np.uint64(8 * k) for k in range(nb))
        px = np.stack([_scale((v & np.uint64(m)) >> np.uint64(s), wd) for m, s, wd in H.fields[:d]], 2)
    px = px.astype(np.uint8)
    return OK, w, h, d, np.ascontiguousarray(px[::-1] if H.flip else px)


# ------------------------------------------------------------------------------------ writers
def dib(hs, w, h, bits, comp=0, used=0, masks=(), size_image=0):
    if hs == 12:
        return struct.pack("<IHHHH", 12, w & 0xFFFF, h & 0xFFFF, 1, bits)
    out = struct.pack("<IiiHHIIiiII", hs, w, h, 1, bits, comp, size_image, 0, 0, used, 0)
    if hs >= 52:
        m = (tuple(masks) + (0, 0, 0, 0))[:4 if hs >= 56 else 3]
        out += struct.pack("<%dI" % len(m), *m)
    return out + bytes(hs - len(out))


def bmp_file(hs, w, h, bits, body, comp=0, used=0, masks=(), palette=b"", gap=0, offbits=None, bf_size=None):
    """A whole file: file header, DIB header, the masks after a 40-byte header, palette bytes, `gap`
    unused bytes, then `body` (raster or packet stream)."""
    head = dib(hs, w, h, bits, comp, used, masks)
    if hs == 40 and comp in (3, 6):
        head += struct.pack("<%dI" % len(masks), *masks)
    off = 14 + len(head) + len(palette) + gap if offbits is None else offbits
    total = 14 + len(head) + len(palette) + gap + len(body)
    return b"BM" + struct.pack("<IHHI", total if bf_size is None else bf_size, 0, 0, off) + head + palette + bytes(gap) + body


def random_palette(seed, n, es=4):
    e = np.random.default_rng(seed).integers(0, 256, (n, es), dtype=np.uint8)
    return e.tobytes()


def grey_palette(n=256, es=4):
    e = np.zeros((n, es), np.uint8)
    e[:, :3] = np.arange(n, dtype=np.uint8)[:, None]
    return e.tobytes()


def raw_file(seed, bits, w, h, topdown=False, hs=40, gap=0, used=None, palette=None, comp=0, masks=()):
    """Random raster bytes (pad bytes included: they are ignored) under the given form."""
    rng = np.random.default_rng(seed)
    stride = (w * bits + 31) // 32 * 4
    body = rng.integers(0, 256, stride * h, dtype=np.uint8).tobytes()
    es = 3 if hs == 12 else 4
    if bits <= 8 and palette is None:
        palette = random_palette(seed + 1, used or 2 ** bits, es)
    return bmp_file(hs, w, -h if topdown else h, bits, body, comp, used or 0, masks, palette or b"", gap)


def run(n, v):
    return bytes([n, v])


def lit(vals, rle):
    """An absolute packet of len(vals) >= 3 palette indices."""
    n = len(vals)
    assert 3 <= n <= 255
    if rle == 8:
        p = bytes(vals)
    else:
        v = list(vals) + [0]
        p = bytes(v[2 * k] << 4 | v[2 * k + 1] for k in range((n + 1) // 2))
    return bytes([0, n]) + p + bytes(len(p) & 1)


EOL, EOB = b"\0\0", b"\0\1"


def delta(dx, dy):
    return bytes([0, 2, dx, dy])


def rle_file(rle, w, h, stream, seed=7, hs=40, gap=0, used=None, palette=None, height=None):
    bits = rle
    if palette is None:
        palette = random_palette(seed, used or 2 ** bits)
    return bmp_file(hs, w, h if height is None else height, bits, stream, 1 if rle == 8 else 2, used or 0, (), palette, gap)


def encode_bound(w, h, d):
    if d not in (1, 3, 4) or not (1 <= w <= 65535 and 1 <= h <= 65535):
        return 0
    return {1: 1078, 3: 54, 4: 122}[d] + (w * d + 3) // 4 * 4 * h


def encode(px):
    """The write's bytes for (h, w, d) pixels, d in 1, 3, 4."""
    h, w, d = px.shape
    stride = (w * d + 3) // 4 * 4
    rows = np.zeros((h, stride), np.uint8)
    file_px = px[::-1] if d == 1 else px[::-1, :, [2, 1, 0] + [3] * (d == 4)]
    rows[:, :w * d] = file_px.reshape(h, w * d)
    off = {1: 1078, 3: 54, 4: 122}[d]
    image = stride * h
    head = b"BM" + struct.pack("<IHHI", off + image, 0, 0, off)
    if d == 4:
        head += struct.pack("<IiiHHIIiiII", 108, w, h, 1, 32, 3, image, 0, 0, 0, 0) + struct.pack("<4I", *M8888) + b"BGRs" + bytes(48)
    else:
        head += struct.pack("<IiiHHIIiiII", 40, w, h, 1, 8 * d, 0, image, 0, 0, 256 if d == 1 else 0, 0)
    if d == 1:
        head += grey_palette()
    assert len(head) == off
    return head + rows.tobytes()


def synth(seed, w, h, d):
    return np.random.default_rng(seed).integers(0, 256, (h, w, d), dtype=np.uint8)


# ------------------------------------------------------------------------------------ case lists
def raw_cases():
    """Every raw depth x WIDTHS x HEIGHTS, bottom-up and top-down."""
    out, seed = [], 1000
    for bits in DEPTHS:
        for w in WIDTHS:
            for h in HEIGHTS:
                for td in (False, True):
                    seed += 1
                    out.append((f"raw{bits}_{w}x{h}_{'td' if td else 'bu'}", raw_file(seed, bits, w, h, td)))
    return out


def offbits_cases():
    """The raster at every residue of bfOffBits mod 16."""
    out = []
    for gap in range(16):
        out.append((f"off24_{gap}", raw_file(2000 + gap, 24, 33, 3, gap=gap)))
        out.append((f"off8_{gap}", raw_file(2100 + gap, 8, 37, 2, gap=gap)))
        out.append((f"off1_{gap}", raw_file(2200 + gap, 1, 129, 2, gap=gap)))
        out.append((f"off16_{gap}", raw_file(2220 + gap, 16, 35, 2, gap=gap, comp=3, masks=M565)))
        out.append((f"off32_{gap}", raw_file(2240 + gap, 32, 35, 2, gap=gap, comp=6, masks=M8888)))
    return out


def header_cases():
    out = []
    for hs in HEADER_SIZES:
        for bits in (1, 4, 8, 24):
            out.append((f"hs{hs}_{bits}", raw_file(2300 + hs + bits, bits, 13, 3, hs=hs)))
        if hs not in (12, 64):
            for bits in (16, 32):  # with compression 0 the masks of a large header are ignored
                out.append((f"hs{hs}_{bits}_rgb", raw_file(2400 + hs + bits, bits, 13, 3, hs=hs, masks=M4444)))
        if hs in (52, 56, 108, 124):
            out.append((f"hs{hs}_fields16", raw_file(2500 + hs, 16, 13, 3, hs=hs, comp=3, masks=M4444)))
            out.append((f"hs{hs}_fields32", raw_file(2600 + hs, 32, 13, 3, hs=hs, comp=3, masks=M8888)))
    return out


def palette_cases():
    out = []
    for used in (1, 2, 16, 255, 256):
        out.append((f"pal8_{used}", raw_file(2700 + used, 8, 67, 3, used=used)))
    for used in (1, 2, 16):
        out.append((f"pal4_{used}", raw_file(2800 + used, 4, 67, 3, used=used)))
    for used in (1, 2):
        out.append((f"pal1_{used}", raw_file(2900 + used, 1, 67, 3, used=used)))
    out.append(("pal8_core3", raw_file(2950, 8, 67, 3, hs=12)))
    out.append(("grey256", raw_file(3000, 8, 67, 3, palette=grey_palette())))
    out.append(("grey255", raw_file(3001, 8, 67, 3, used=255, palette=grey_palette(255))))
    out.append(("grey_core", raw_file(3002, 8, 67, 3, hs=12, palette=grey_palette(256, 3))))
    off = bytearray(grey_palette())
    off[4 * 200 + 1] ^= 1  # one entry off the identity
    out.append(("grey_one_off", raw_file(3003, 8, 67, 3, palette=bytes(off))))
    return out


def mask_cases():
    out = []
    for name, bits, comp, hs, masks in (
            ("555", 16, 3, 40, M555), ("565", 16, 3, 40, M565), ("4444_v3", 16, 3, 56, M4444), ("4444_alpha", 16, 6, 40, M4444),
            ("8888", 32, 6, 40, M8888), ("8888_v4", 32, 3, 108, M8888), ("8888_no_alpha", 32, 3, 40, M8888[:3]),
            ("101010", 32, 3, 40, M101010), ("5551", 16, 6, 40, M5551), ("zero_red", 16, 3, 40, (0, 0x03E0, 0x001F)),
            ("zero_all", 32, 3, 40, (0, 0, 0)), ("zero_alpha", 32, 6, 40, M8888[:3] + (0,)),
            ("wide32", 32, 3, 40, (0xFFFF0000, 0x0000FF00, 0x000000FF)), ("past16", 16, 3, 40, (0x1FC00, 0x03E0, 0x1F)),
            ("one_bit_each", 16, 6, 40, (1, 2, 4, 8)), ("hs52_comp6", 32, 6, 52, M8888), ("hs52_comp6_16", 16, 6, 52, M4444), ("332", 16, 3, 52, (0xE0, 0x1C, 0x03))):
        for w in (5, 130):
            out.append((f"mask_{name}_{w}", raw_file(3100 + len(out), bits, w, 3, hs=hs, comp=comp, masks=masks)))
    return out


def rle_shape_cases(rle):
    """Crafted streams, one property each."""
    L = lambda n, s=0: lit([(s + 3 * k) % (256 if rle == 8 else 16) for k in range(n)], rle)
    c = []
    for n in (1, 2, 254, 255):
        c.append((f"run{n}", 300, 3, run(n, 0x5A) + EOL + run(n, 0xC3) + EOB))
        c.append((f"run{n}_clipped", 20, 3, run(n, 0x5A) + EOL + run(3, 1) + run(n, 0xC3) + EOB))
    for n in (3, 4, 5, 255):
        c.append((f"lit{n}", 300, 3, L(n) + EOL + L(n, 5) + run(2, 7) + EOB))
        c.append((f"lit{n}_clipped", 20, 3, run(18, 9) + L(n) + EOL + L(n, 5) + EOB))
    c.append(("nibble_phase", 40, 2, L(3) + run(3, 0x12) + L(5, 2) + run(5, 0x34) + run(1, 0x56) + L(4, 1) + EOB))
    c.append(("eol_mid_row", 20, 4, run(5, 1) + EOL + run(6, 2) + EOL + EOL + EOL + run(7, 3) + EOB))
    c.append(("eol_first", 20, 4, EOL + EOL + run(7, 3) + EOB))
    for dx in (0, 1, 255):
        for dy in (0, 1, 255):
            c.append((f"delta_{dx}_{dy}", 300, 300 if dy == 255 else 5, run(3, 1) + delta(dx, dy) + run(4, 2) + EOL + run(2, 3) + EOB))
    c.append(("delta_chain", 30, 30, b"".join(delta(3, 2) + run(2, 9) for _ in range(12)) + EOB))
    c.append(("x_keeps_counting", 20, 3, run(255, 1) + run(255, 2) + delta(255, 0) + L(255) + EOL + run(3, 4) + EOB))
    c.append(("y_past_h", 20, 3, run(3, 1) + EOL + EOL + EOL + run(5, 2) + L(4) + delta(1, 1) + run(5, 3) + EOB))
    c.append(("y_far_past_h", 20, 3, run(3, 1) + b"".join(delta(0, 255) for _ in range(40)) + run(5, 2) + EOB))
    c.append(("early_eob", 20, 3, run(4, 1) + EOB + run(9, 2) + EOL + L(5) + EOB))
    c.append(("no_eob", 20, 3, run(4, 1) + EOL + L(5)))
    c.append(("no_eob_odd_byte", 20, 3, run(4, 1) + EOL + L(5) + b"\7"))
    c.append(("empty_stream", 20, 3, b""))
    c.append(("only_eob", 20, 3, EOB))
    c.append(("full_rows", 7, 3, (run(7, 0x21) + EOL) * 3 + EOB))
    return [(f"rle{rle}_{n}", rle_file(rle, w, h, s, seed=len(n))) for n, w, h, s in c]


def random_stream(seed, rle, nbytes, w):
    """A seeded mix of every packet kind, about nbytes long, without an end-of-bitmap."""
    rng = np.random.default_rng(seed)
    out, top = [], 256 if rle == 8 else 16
    size = 0
    while size < nbytes:
        r = rng.integers(0, 100)
        if r < 45:
            p = run(int(rng.integers(1, 40 if r < 40 else 256)), int(rng.integers(0, 256)))
        elif r < 80:
            p = lit([int(v) for v in rng.integers(0, top, int(rng.integers(3, 30 if r < 75 else 256)))], rle)
        elif r < 95:
            p = EOL
        else:
            p = delta(int(rng.integers(0, 6)), int(rng.integers(0, 2)))
        out.append(p)
        size += len(p)
    return b"".join(out)


def tiled_case(rle, tile, seed=5):
    """A stream over more than three tiles of `tile` bytes."""
    return rle_file(rle, 211, 400, random_stream(seed, rle, 3 * tile + 700, 211) + EOB, seed=seed)


def edge_cases(rle, tile):
    """A 4-byte delta packet and a 255-pixel absolute packet at every even offset across the first
    two tile edges: from ending exactly at the edge to starting exactly at it."""
    out = []
    top = 256 if rle == 8 else 16
    big = lit([(7 * k + 1) % top for k in range(255)], rle)
    unit = lit([(5 * k + 2) % top for k in range(254)], rle) + EOL  # filler: a row of 254 pixels
    for edge in (tile, 2 * tile):
        for name, p in (("delta", delta(2, 1)), ("lit255", big)):
            for o in range(edge - len(p), edge + 2, 2):
                k, m = divmod(o, len(unit))
                m //= 2
                s = unit * k + b"".join(run(1, j & 255) for j in range(m)) + p + run(5, 3) + EOL + lit([1, 2, 3], rle) + EOB
                assert s.index(p, o) == o and len(unit * k) + 2 * m == o
                out.append((f"rle{rle}_{name}_at_{o}", rle_file(rle, 300, 80, s, seed=o)))
    return out


INT_MIN = -2 ** 31


def error_cases():
    """(name, file, code): every read status and the order of the checks."""
    ok24 = raw_file(1, 24, 5, 3)
    ok8 = raw_file(2, 8, 5, 3)
    pal = random_palette(3, 256)

    def patched(data, at, fmt, *v):
        b = bytearray(data)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    c = [("exact", ok24, OK), ("trailing_bytes", ok24 + b"xyz", OK),
         ("empty", b"", NOT_BMP), ("short_17", ok24[:17], NOT_BMP), ("magic", b"BN" + ok24[2:], NOT_BMP),
         ("magic_wins_over_header", b"MB" + patched(ok24, 14, "<I", 41)[2:], NOT_BMP),
         ("hs_41", patched(ok24, 14, "<I", 41), BAD_HEADER), ("hs_0", patched(ok24, 14, "<I", 0), BAD_HEADER),
         ("hs_16", patched(ok24, 14, "<I", 16), BAD_HEADER),
         ("header_past_file", ok24[:53], BAD_HEADER), ("core_past_file", raw_file(4, 24, 5, 3, hs=12)[:25], BAD_HEADER),
         ("w_0", patched(ok24, 18, "<i", 0), BAD_HEADER), ("w_neg", patched(ok24, 18, "<i", -5), BAD_HEADER),
         ("h_0", patched(ok24, 22, "<i", 0), BAD_HEADER), ("h_int_min", patched(ok24, 22, "<i", INT_MIN), BAD_HEADER),
         ("bits_2", patched(ok24, 28, "<H", 2), BAD_HEADER), ("bits_0", patched(ok24, 28, "<H", 0), BAD_HEADER),
         ("bits_48", patched(ok24, 28, "<H", 48), BAD_HEADER),
         ("clr_used_257", patched(ok8, 46, "<I", 257), BAD_HEADER),
         ("clr_used_3_of_1bit", patched(raw_file(5, 1, 5, 3), 46, "<I", 3), BAD_HEADER),
         ("clr_used_huge_24", patched(ok24, 46, "<I", 2 ** 24 + 1), BAD_HEADER),
         ("offbits_in_palette", patched(ok8, 10, "<I", 54 + 1020), BAD_HEADER),
         ("offbits_in_header", patched(ok24, 10, "<I", 50), BAD_HEADER),
         ("offbits_in_masks", patched(raw_file(6, 16, 5, 3, comp=3, masks=M565), 10, "<I", 62), BAD_HEADER),
         ("offbits_in_unused_palette_24", patched(patched(ok24, 46, "<I", 2), 10, "<I", 58), BAD_HEADER),
         ("rle8_on_4", patched(raw_file(7, 4, 5, 3), 30, "<I", 1), BAD_HEADER),
         ("rle4_on_8", patched(ok8, 30, "<I", 2), BAD_HEADER),
         ("fields_on_24", patched(ok24, 30, "<I", 3), BAD_HEADER), ("alphafields_on_8", patched(ok8, 30, "<I", 6), BAD_HEADER),
         ("masks_past_file", raw_file(8, 16, 5, 3, comp=3, masks=M565)[:60], BAD_HEADER),
         ("bad_header_wins_over_unsupported", patched(patched(ok24, 30, "<I", 4), 18, "<i", 0), BAD_HEADER),
         ("jpeg", patched(ok24, 30, "<I", 4), UNSUPPORTED), ("png", patched(ok24, 30, "<I", 5), UNSUPPORTED),
         ("comp_7", patched(ok24, 30, "<I", 7), UNSUPPORTED), ("comp_11", patched(ok24, 30, "<I", 11), UNSUPPORTED),
         ("os2_rle", rle_file(8, 5, 3, run(5, 1) + EOB, hs=64), UNSUPPORTED),
         ("os2_fields", raw_file(9, 16, 5, 3, hs=64, comp=3), UNSUPPORTED),
         ("rle8_topdown", rle_file(8, 5, 3, run(5, 1) + EOB, height=-3), UNSUPPORTED),
         ("rle4_topdown", rle_file(4, 5, 3, run(5, 1) + EOB, height=-3), UNSUPPORTED),
         ("mask_gap", raw_file(10, 16, 5, 3, comp=3, masks=(0x5000, 0x03E0, 0x1F)), UNSUPPORTED),
         ("mask_overlap", raw_file(11, 16, 5, 3, comp=3, masks=(0x7C00, 0x07E0, 0x1F)), UNSUPPORTED),
         ("alpha_overlap", raw_file(12, 32, 5, 3, comp=6, masks=M8888[:3] + (0xFF800000,)), UNSUPPORTED),
         ("unsupported_wins_over_too_large", patched(patched(patched(ok24, 30, "<I", 4), 18, "<i", 65536), 22, "<i", 16385), UNSUPPORTED),
         ("too_large", patched(patched(ok24, 18, "<i", 65536), 22, "<i", 16385), TOO_LARGE),
         ("too_large_topdown", patched(patched(ok24, 18, "<i", 65536), 22, "<i", -16385), TOO_LARGE),
         ("pixels_2_30", patched(patched(ok24, 18, "<i", 65536), 22, "<i", 16384), TRUNCATED),
         ("hs52_comp6_66_bytes", raw_file(13, 32, 5, 3, hs=52, comp=6, masks=M8888)[:66], TRUNCATED),
         ("hs52_comp6_palette_is_no_mask", raw_file(14, 32, 5, 3, hs=52, comp=6, masks=M8888, used=1, palette=b"\xff\0\0\0"), OK),
         ("hs56_comp3_70_bytes", raw_file(15, 32, 5, 3, hs=56, comp=3, masks=M8888)[:70], TRUNCATED),
         ("hs40_comp6_70_bytes", raw_file(16, 32, 5, 3, comp=6, masks=M8888)[:70], TRUNCATED),
         ("hs40_comp6_69_bytes", raw_file(16, 32, 5, 3, comp=6, masks=M8888)[:69], BAD_HEADER),
         ("hs40_comp3_66_bytes", raw_file(17, 16, 5, 3, comp=3, masks=M565)[:66], TRUNCATED),
         ("raster_short_1", ok24[:-1], TRUNCATED), ("raster_missing", ok24[:54], TRUNCATED),
         ("palette_cut", ok8[:54 + 1000], TRUNCATED), ("offbits_past_file", patched(ok24, 10, "<I", len(ok24) + 1), TRUNCATED),
         ("raw_offbits_at_end", patched(ok24, 10, "<I", len(ok24)), TRUNCATED)]
    for rle in (8, 4):
        full = rle_file(rle, 9, 3, run(4, 1) + lit([1, 2, 3, 4, 5, 6, 7], rle) + delta(1, 1) + run(2, 3) + EOB)
        nl = len(lit([1, 2, 3, 4, 5, 6, 7], rle))
        start = len(full) - (2 + 2 + 4 + nl)  # of the literal packet
        c += [(f"rle{rle}_whole", full, OK),
              (f"rle{rle}_offbits_at_end", rle_file(rle, 9, 3, b""), OK),
              (f"rle{rle}_cut_in_literal", full[:start + 4], TRUNCATED),
              (f"rle{rle}_cut_pad_byte", full[:start + nl - 1], TRUNCATED),
              (f"rle{rle}_cut_literal_header_only", full[:start + 2], TRUNCATED),
              (f"rle{rle}_cut_in_delta", full[:start + nl + 3], TRUNCATED),
              (f"rle{rle}_cut_delta_header_only", full[:start + nl + 2], TRUNCATED),
              (f"rle{rle}_cut_between_packets", full[:start + nl], OK),
              (f"rle{rle}_cut_one_byte_into_packet", full[:start + nl + 1], OK),
              (f"rle{rle}_cut_after_eob", rle_file(rle, 9, 3, run(4, 1) + EOB + bytes([0, 200, 1])), OK)]
    assert {code for _, _, code in c} == {OK, NOT_BMP, BAD_HEADER, UNSUPPORTED, TRUNCATED, TOO_LARGE}
    return c


def fuzz_sources():
    """One 24-bit and one RLE8 file, small enough for every prefix."""
    raw = raw_file(41, 24, 5, 3)
    rle = rle_file(8, 9, 4, run(4, 1) + lit([1, 2, 3, 0, 2], 8) + EOL + delta(2, 1) + run(3, 2) + EOL + lit([3, 2, 1], 8) + EOB,
                   used=4)
    return raw, rle


def prefixes(data):
    return [data[:k] for k in range(len(data) + 1)]


def bit_flips(data, seed, count=200):
    """Seeded single-bit flips anywhere in the file but the three upper bytes of biWidth and
    biHeight: those ask for images of up to 2^30 pixels, which try the allocator and nothing else.
    Every flipped file is at most 255 x 255."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        b = bytearray(data)
        k = int(rng.integers(0, 8 * len(data)))
        if k >> 3 in (19, 20, 21, 23, 24, 25):
            continue
        b[k >> 3] ^= 1 << (k & 7)
        out.append(bytes(b))
    return out


def pil_raw_cases():
    """Raw files PIL reads as the contract does: 1, 4, 8, 24 and 32 bits, 40-byte header."""
    return [(n, f) for n, f in raw_cases() if not n.startswith("raw16_") and ("x3_" in n or "x17_" in n)]


def pil_rle_cases():
    """Run-length streams in which no packet crosses a row end and no delta occurs. RLE4 absolute
    packets have even counts: PIL reads n // 2 bytes for n pixels, one too few when n is odd."""
    out = []
    for rle in (8, 4):
        top = 256 if rle == 8 else 16
        for w in (1, 2, 3, 7, 31, 254, 255, 300):
            rng = np.random.default_rng(w + rle)
            s = b""
            for y in range(4):
                x = 0
                while x < w:
                    n = int(min(w - x, rng.integers(1, 60)))
                    if n >= 3 and (rle == 8 or n % 2 == 0) and rng.integers(0, 2):
                        s += lit([int(v) for v in rng.integers(0, top, n)], rle)
                    else:
                        s += run(n, int(rng.integers(0, 256)))
                    x += n
                s += EOL
            out.append((f"pil_rle{rle}_{w}", rle_file(rle, w, 4, s + EOB, seed=w)))
    return out
