"""The DDS contract of include/icx.h restated with struct and numpy only: decode(file) and
encode(px, fmt), file builders for every form, and the case lists the CPU and GPU tests share.
Nothing here is shared with imagecodecs_amd/csrc/icx_dds_core.h."""
import struct

import numpy as np

OK, NOT_DDS, BAD_HEADER, UNSUPPORTED, TRUNCATED, TOO_LARGE, INVALID_ARGUMENT = range(7)
UBYTE, USHORT, FLOAT = range(3)
RAW, BC = 0, 1
DTYPES = (np.uint8, np.dtype("<u2"), np.dtype("<f4"))

# (block bytes, channels) of BC1 .. BC5
BLOCK = {1: (8, 3), 2: (16, 4), 3: (16, 4), 4: (8, 1), 5: (16, 2)}
FOURCC_BC = {b"DXT1": 1, b"DXT2": 2, b"DXT3": 2, b"DXT4": 3, b"DXT5": 3, b"BC3U": 3, b"ATI1": 4, b"BC4U": 4, b"ATI2": 5,
             b"BC5U": 5}
DXGI_BC = {71: 1, 72: 1, 74: 2, 75: 2, 77: 3, 78: 3, 80: 4, 83: 5}
# (type, channels) of the copied forms, by DXGI format and by legacy FourCC number
DXGI_COPY = {2: (FLOAT, 4), 6: (FLOAT, 3), 16: (FLOAT, 2), 41: (FLOAT, 1), 11: (USHORT, 4), 35: (USHORT, 2), 56: (USHORT, 1)}
LEGACY_COPY = {116: (FLOAT, 4), 115: (FLOAT, 2), 114: (FLOAT, 1), 36: (USHORT, 4)}
# (bit count, R, G, B, A masks) of the DX10 8-bit forms
DXGI_BYTES = {28: (32, 0xFF, 0xFF00, 0xFF0000, 0xFF000000), 29: (32, 0xFF, 0xFF00, 0xFF0000, 0xFF000000),
              87: (32, 0xFF0000, 0xFF00, 0xFF, 0xFF000000), 91: (32, 0xFF0000, 0xFF00, 0xFF, 0xFF000000),
              88: (32, 0xFF0000, 0xFF00, 0xFF, 0), 93: (32, 0xFF0000, 0xFF00, 0xFF, 0), 61: (8, 0xFF, 0, 0, 0),
              49: (16, 0xFF, 0xFF00, 0, 0)}


# ------------------------------------------------------------------------------------ read
def _field(m):
    """(shift, width) of a mask, or None when its set bits are not contiguous."""
    if m == 0:
        return 0, 0
    s = (m & -m).bit_length() - 1
    v = m >> s
    return (s, v.bit_length()) if v & (v + 1) == 0 else None


def _channels(bits, masks, lum):
    """The masks of the output channels, in order; None for what the contract refuses."""
    seen = 0
    for m in masks:
        if _field(m) is None or m >> bits or seen & m:
            return None
        seen |= m
    r, g, b, a = masks
    if lum:
        return None if not r else [r] + ([a] if a else [])
    if not (r or g or b):
        return [a] if a else None
    if r and not g and not b and not a:
        return [r]
    if r and g and not b and not a:
        return [r, g]
    if r and g and b:
        return [r, g, b] + ([a] if a else [])
    return None


def _scale(v, width):
    """A field's values -> 8 bits."""
    v = v.astype(np.uint64)
    if width > 8:
        return (v >> np.uint64(width - 8)).astype(np.uint8)
    m = (1 << width) - 1
    return ((v * np.uint64(510) + np.uint64(m)) // np.uint64(2 * m)).astype(np.uint8)


def _expand565(c):
    c = c.astype(np.uint32)
    r, g, b = c >> 11 & 31, c >> 5 & 63, c & 31
    return np.stack([r << 3 | r >> 2, g << 2 | g >> 4, b << 3 | b >> 2], -1)  # (N, 3)


def color_palette(c0, c1, four):
    """(N,) 5-6-5 endpoints -> (N, 4, 3) palette; four: always the 4-colour form."""
    p0, p1 = _expand565(c0), _expand565(c1)
    a = np.stack([p0, p1, (2 * p0 + p1) // 3, (p0 + 2 * p1) // 3], 1)
    if four:
        return a
    b = np.stack([p0, p1, (p0 + p1) // 2, np.zeros_like(p0)], 1)
    return np.where((c0 > c1)[:, None, None], a, b)


def alpha_palette(a0, a1):
    """(N,) endpoints -> (N, 8) palette."""
    a0, a1 = a0.astype(np.uint32), a1.astype(np.uint32)
    e8 = np.stack([a0, a1] + [((7 - k) * a0 + k * a1) // 7 for k in range(1, 7)], 1)
    e6 = np.stack([a0, a1] + [((5 - k) * a0 + k * a1) // 5 for k in range(1, 5)] + [np.zeros_like(a0), np.full_like(a0, 255)], 1)
    return np.where((a0 > a1)[:, None], e8, e6)


def _color_block(b, four):
    """(N, 8) bytes -> (N, 16, 3)."""
    c = b[:, :4].copy().view("<u2")
    idx = b[:, 4:8].copy().view("<u4")[:, 0]
    pal = color_palette(c[:, 0], c[:, 1], four)
    sel = (idx[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3
    return np.take_along_axis(pal, sel[:, :, None].astype(np.int64), 1)


def _alpha_block(b):
    """(N, 8) bytes -> (N, 16)."""
    pal = alpha_palette(b[:, 0], b[:, 1])
    bits = np.zeros(len(b), np.uint64)
    for k in range(6):
        bits |= b[:, 2 + k].astype(np.uint64) << np.uint64(8 * k)
    sel = (bits[:, None] >> (3 * np.arange(16, dtype=np.uint64))[None, :]) & np.uint64(7)
    return np.take_along_axis(pal, sel.astype(np.int64), 1)


def _explicit_alpha(b):
    """(N, 8) bytes of 4-bit alpha -> (N, 16)."""
    lo, hi = b & 15, b >> 4
    return (np.stack([lo, hi], -1).reshape(len(b), 16).astype(np.uint32)) * 17


def decode_blocks(kind, blocks):
    """(N, block bytes) -> (N, 16, channels) uint8."""
    if kind == 1:
        px = _color_block(blocks, False)
    elif kind == 2:
        px = np.concatenate([_color_block(blocks[:, 8:], True), _explicit_alpha(blocks[:, :8])[:, :, None]], 2)
    elif kind == 3:
        px = np.concatenate([_color_block(blocks[:, 8:], True), _alpha_block(blocks[:, :8])[:, :, None]], 2)
    elif kind == 4:
        px = _alpha_block(blocks)[:, :, None]
    else:
        px = np.stack([_alpha_block(blocks[:, :8]), _alpha_block(blocks[:, 8:])], 2)
    return px.astype(np.uint8)


def _walk(f):
    """The header walk -> (code, dict)."""
    n = len(f)
    if n < 4 or f[:4] != b"DDS ":
        return NOT_DDS, None
    if n < 128:
        return BAD_HEADER, None
    size, flags, h, w = struct.unpack_from("<4I", f, 4)
    pfsize, pff, cc, bits, mr, mg, mb, ma = struct.unpack_from("<8I", f, 76)
    caps2, = struct.unpack_from("<I", f, 112)
    if size != 124 or pfsize != 32 or w == 0 or h == 0:
        return BAD_HEADER, None
    fourcc = bool(pff & 4)
    dx10 = fourcc and f[84:88] == b"DX10"
    if dx10 and n < 148:
        return BAD_HEADER, None
    if not fourcc and bits not in (8, 16, 24, 32):
        return BAD_HEADER, None
    if caps2 & (0x200 | 0x200000):
        return UNSUPPORTED, None
    H = dict(w=w, h=h, at=148 if dx10 else 128)
    if dx10:
        fmt, dim, misc, arr = struct.unpack_from("<4I", f, 128)
        if arr != 1 or misc & 4 or dim != 3:
            return UNSUPPORTED, None
        if fmt in DXGI_BC:
            H.update(kind=DXGI_BC[fmt])
        elif fmt in DXGI_COPY:
            H.update(copy=DXGI_COPY[fmt])
        elif fmt in DXGI_BYTES:
            H.update(bits=DXGI_BYTES[fmt][0], chans=_channels(DXGI_BYTES[fmt][0], DXGI_BYTES[fmt][1:], False))
        else:
            return UNSUPPORTED, None
    elif fourcc:
        if f[84:88] in FOURCC_BC:
            H.update(kind=FOURCC_BC[f[84:88]])
        elif cc in LEGACY_COPY:
            H.update(copy=LEGACY_COPY[cc])
        else:
            return UNSUPPORTED, None
    else:
        chans = _channels(bits, (mr, mg, mb, ma), bool(pff & 0x20000))
        if chans is None:
            return UNSUPPORTED, None
        H.update(bits=bits, chans=chans)
    if w * h > 1 << 30:
        return TOO_LARGE, None
    if "kind" in H:
        H.update(d=BLOCK[H["kind"]][1], type=UBYTE, nbytes=((w + 3) // 4) * ((h + 3) // 4) * BLOCK[H["kind"]][0])
    elif "copy" in H:
        t, d = H["copy"]
        H.update(d=d, type=t, nbytes=w * h * d * (4 if t == FLOAT else 2))
    else:
        H.update(d=len(H["chans"]), type=UBYTE, nbytes=w * h * H["bits"] // 8)
    if H["at"] + H["nbytes"] > n:
        return TRUNCATED, None
    return OK, H


def probe(f):
    code, H = _walk(f)
    return (code, H["w"], H["h"], H["d"], H["type"]) if code == OK else (code, 0, 0, 0, 0)


def decode(f):
    """-> (code, w, h, d, type, array (h, w, d) or None)."""
    f = bytes(f)
    code, H = _walk(f)
    if code != OK:
        return code, 0, 0, 0, 0, None
    w, h, d, t = H["w"], H["h"], H["d"], H["type"]
    top = np.frombuffer(f, np.uint8, H["nbytes"], H["at"])
    if "kind" in H:
        bs = BLOCK[H["kind"]][0]
        bw, bh = (w + 3) // 4, (h + 3) // 4
        px = decode_blocks(H["kind"], top.reshape(-1, bs)).reshape(bh, bw, 4, 4, d)
        px = px.transpose(0, 2, 1, 3, 4).reshape(4 * bh, 4 * bw, d)[:h, :w].copy()
    elif "copy" in H:
        px = top.view(DTYPES[t]).reshape(h, w, d).copy()
    else:
        nb = H["bits"] // 8
        v = np.zeros(w * h, np.uint32)
        raw = top.reshape(w * h, nb)
        for k in range(nb):
            v |= raw[:, k].astype(np.uint32) << np.uint32(8 * k)
        px = np.stack([_scale((v & np.uint32(m)) >> np.uint32(_field(m)[0]), _field(m)[1]) for m in H["chans"]], -1).reshape(h, w, d)
    return OK, w, h, d, t, px


# ------------------------------------------------------------------------------------ write
def encode_bound(w, h, d, fmt):
    if not (1 <= d <= 4 and 1 <= w <= 65535 and 1 <= h <= 65535 and fmt in (RAW, BC)):
        return 0
    if fmt == RAW:
        return 128 + w * h * d
    return 128 + ((w + 3) // 4) * ((h + 3) // 4) * (8 if d in (1, 3) else 16)


def encode_color_blocks(px):
    """(N, 16, 3) uint8 -> (N, 8) bytes."""
    p = px.astype(np.int64)
    hi, lo = p.max(1), p.min(1)

    def q565(v):
        return ((31 * v[:, 0] + 127) // 255) << 11 | ((63 * v[:, 1] + 127) // 255) << 5 | (31 * v[:, 2] + 127) // 255

    c0, c1 = q565(hi), q565(lo)
    pal = color_palette(c0, c1, True).astype(np.int64)
    dist = ((p[:, :, None, :] - pal[:, None, :, :]) ** 2).sum(3)  # (N, 16, 4)
    sel = dist.argmin(2)  # (the first of equal minima)
    sel[c0 == c1] = 0
    idx = (sel.astype(np.uint64) << (2 * np.arange(16, dtype=np.uint64))[None, :]).sum(1).astype("<u4")
    out = np.zeros((len(px), 8), np.uint8)
    out[:, 0:2] = c0.astype("<u2")[:, None].view(np.uint8)
    out[:, 2:4] = c1.astype("<u2")[:, None].view(np.uint8)
    out[:, 4:8] = idx[:, None].view(np.uint8)
    return out


def encode_alpha_blocks(v):
    """(N, 16) uint8 -> (N, 8) bytes."""
    a = v.astype(np.int64)
    a0, a1 = a.max(1), a.min(1)
    pal = alpha_palette(a0, a1).astype(np.int64)
    sel = np.abs(a[:, :, None] - pal[:, None, :]).argmin(2)
    sel[a0 == a1] = 0
    bits = (sel.astype(np.uint64) << (3 * np.arange(16, dtype=np.uint64))[None, :]).sum(1)
    out = np.zeros((len(v), 8), np.uint8)
    out[:, 0], out[:, 1] = a0, a1
    for k in range(6):
        out[:, 2 + k] = (bits >> np.uint64(8 * k)) & np.uint64(255)
    return out


def encode_blocks(px):
    """(N, 16, d) uint8 -> (N, 8 or 16) bytes: DXT1, DXT5, BC4, BC5 by d."""
    d = px.shape[2]
    if d == 3:
        return encode_color_blocks(px)
    if d == 4:
        return np.concatenate([encode_alpha_blocks(px[:, :, 3]), encode_color_blocks(px[:, :, :3])], 1)
    if d == 1:
        return encode_alpha_blocks(px[:, :, 0])
    return np.concatenate([encode_alpha_blocks(px[:, :, 0]), encode_alpha_blocks(px[:, :, 1])], 1)


def write_header(w, h, d, fmt):
    raw = fmt == RAW
    head = bytearray(128)
    head[:4] = b"DDS "
    struct.pack_into("<5I", head, 4, 124, 0x1007 | (0x8 if raw else 0x80000), h, w, w * d if raw else encode_bound(w, h, d, fmt) - 128)
    struct.pack_into("<I", head, 76, 32)
    struct.pack_into("<I", head, 108, 0x1000)
    if raw:
        pf = {3: (0x40, 24, 0xFF0000, 0xFF00, 0xFF, 0), 4: (0x41, 32, 0xFF0000, 0xFF00, 0xFF, 0xFF000000),
              1: (0x20000, 8, 0xFF, 0, 0, 0), 2: (0x20001, 16, 0xFF, 0, 0, 0xFF00)}[d]
        struct.pack_into("<I", head, 80, pf[0])
        struct.pack_into("<5I", head, 88, *pf[1:])
    else:
        struct.pack_into("<I", head, 80, 4)
        head[84:88] = {3: b"DXT1", 4: b"DXT5", 1: b"BC4U", 2: b"BC5U"}[d]
    return bytes(head)


def encode(px, fmt=RAW):
    """uint8 (h, w, d) -> the file."""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, d = px.shape
    assert encode_bound(w, h, d, fmt)
    if fmt == RAW:
        body = px[:, :, [2, 1, 0] + [3] * (d == 4)] if d >= 3 else px
        return write_header(w, h, d, fmt) + body.tobytes()
    bw, bh = (w + 3) // 4, (h + 3) // 4
    pad = np.pad(px, ((0, 4 * bh - h), (0, 4 * bw - w), (0, 0)), mode="edge")
    blocks = pad.reshape(bh, 4, bw, 4, d).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, d)
    return write_header(w, h, d, fmt) + encode_blocks(blocks).tobytes()


# ------------------------------------------------------------------------------------ builders
def header(w, h, pff=0, fourcc=b"\0\0\0\0", bits=0, masks=(0, 0, 0, 0), flags=0x1007, pitch=0, depth=0, mips=0, caps=0x1000,
           caps2=0, size=124, pfsize=32, magic=b"DDS ", dx10=None):
    """The 128 header bytes; dx10 = (format, dimension, misc, array size, misc2) appends the DX10 header."""
    if isinstance(fourcc, int):
        fourcc = struct.pack("<I", fourcc)
    head = magic + struct.pack("<7I", size, flags, h, w, pitch, depth, mips) + bytes(44)
    head += struct.pack("<2I", pfsize, pff) + fourcc + struct.pack("<5I", bits, *masks) + struct.pack("<5I", caps, caps2, 0, 0, 0)
    assert len(head) == 128
    if dx10 is not None:
        head += struct.pack("<5I", *dx10)
    return head


def dx10_header(w, h, fmt, dim=3, misc=0, arr=1, **kw):
    return header(w, h, pff=4, fourcc=b"DX10", dx10=(fmt, dim, misc, arr, 0), **kw)


def rng(seed):
    return np.random.default_rng(seed)


def block_file(seed, fourcc, w, h, tail=0, dxgi=None):
    """A file of random blocks of the FourCC's (or the DXGI format's) kind."""
    kind = DXGI_BC[dxgi] if dxgi is not None else FOURCC_BC[fourcc]
    n = ((w + 3) // 4) * ((h + 3) // 4) * BLOCK[kind][0]
    body = rng(seed).integers(0, 256, n + tail, dtype=np.uint8).tobytes()
    head = dx10_header(w, h, dxgi) if dxgi is not None else header(w, h, pff=4, fourcc=fourcc)
    return head + body


def masked_file(seed, w, h, bits, masks, pff=None, tail=0):
    if pff is None:
        pff = 0x40 | (1 if masks[3] else 0)
    body = rng(seed).integers(0, 256, w * h * bits // 8 + tail, dtype=np.uint8).tobytes()
    return header(w, h, pff=pff, bits=bits, masks=masks) + body


def copy_file(seed, w, h, dxgi=None, legacy=None, nan=False):
    t, d = DXGI_COPY[dxgi] if dxgi is not None else LEGACY_COPY[legacy]
    if t == FLOAT:
        a = rng(seed).standard_normal(w * h * d).astype("<f4")
        if nan:  # quiet and signalling NaNs with payloads, infinities, a negative zero, a subnormal
            a.view("<u4")[:7] = [0x7FC12345, 0xFF812345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001][:a.size]
        body = a.tobytes()
    else:
        body = rng(seed).integers(0, 65536, w * h * d, dtype=np.uint16).astype("<u2").tobytes()
    head = dx10_header(w, h, dxgi) if dxgi is not None else header(w, h, pff=4, fourcc=legacy)
    return head + body


# ------------------------------------------------------------------------------------ case lists
BLOCK_FOURCCS = (b"DXT1", b"DXT3", b"DXT5", b"ATI1", b"ATI2")  # one FourCC per block format
# name, bit count, (R, G, B, A), ddspf flags
MASK_SETS = [
    ("r8g8b8", 24, (0xFF0000, 0xFF00, 0xFF, 0), 0x40), ("b8g8r8", 24, (0xFF, 0xFF00, 0xFF0000, 0), 0x40),
    ("a8r8g8b8", 32, (0xFF0000, 0xFF00, 0xFF, 0xFF000000), 0x41), ("a8b8g8r8", 32, (0xFF, 0xFF00, 0xFF0000, 0xFF000000), 0x41),
    ("x8r8g8b8", 32, (0xFF0000, 0xFF00, 0xFF, 0), 0x40), ("x8b8g8r8", 32, (0xFF, 0xFF00, 0xFF0000, 0), 0x40),
    ("a2r10g10b10", 32, (0x3FF00000, 0xFFC00, 0x3FF, 0xC0000000), 0x41), ("a2b10g10r10", 32, (0x3FF, 0xFFC00, 0x3FF00000, 0xC0000000), 0x41),
    ("g16r16", 32, (0xFFFF, 0xFFFF0000, 0, 0), 0x40), ("r32", 32, (0xFFFFFFFF, 0, 0, 0), 0x40),
    ("r5g6b5", 16, (0xF800, 0x7E0, 0x1F, 0), 0x40), ("a1r5g5b5", 16, (0x7C00, 0x3E0, 0x1F, 0x8000), 0x41),
    ("x1r5g5b5", 16, (0x7C00, 0x3E0, 0x1F, 0), 0x40), ("a4r4g4b4", 16, (0xF00, 0xF0, 0xF, 0xF000), 0x41),
    ("x4r4g4b4", 16, (0xF00, 0xF0, 0xF, 0), 0x40), ("a8r3g3b2", 16, (0xE0, 0x1C, 0x3, 0xFF00), 0x41),
    ("r8g8", 16, (0xFF, 0xFF00, 0, 0), 0x40), ("r16", 16, (0xFFFF, 0, 0, 0), 0x40),
    ("r3g3b2", 8, (0xE0, 0x1C, 0x3, 0), 0x40), ("r8", 8, (0xFF, 0, 0, 0), 0x40), ("r1_in_8", 8, (0x10, 0, 0, 0), 0x40),
    ("a8", 8, (0, 0, 0, 0xFF), 0x2), ("a8_in_16", 16, (0, 0, 0, 0xFF00), 0x2), ("a4_in_32", 32, (0, 0, 0, 0xF0000), 0x2),
    ("l8", 8, (0xFF, 0, 0, 0), 0x20000), ("a8l8", 16, (0xFF, 0, 0, 0xFF00), 0x20001), ("l16", 16, (0xFFFF, 0, 0, 0), 0x20000),
    ("a4l4", 8, (0x0F, 0, 0, 0xF0), 0x20001), ("l8_rgb_masks", 24, (0xFF, 0xFF00, 0xFF0000, 0), 0x20000),
    ("no_flags_rgb", 24, (0xFF0000, 0xFF00, 0xFF, 0), 0),
]
BAD_MASKS = [
    ("gap", 32, (0xFF00FF, 0xFF00, 0, 0)), ("overlap", 16, (0xFF, 0x1F0, 0, 0)), ("past_bits", 16, (0xFF0000, 0xFF00, 0xFF, 0)),
    ("past_bits8", 8, (0x1FF, 0, 0, 0)), ("r_b_only", 24, (0xFF0000, 0, 0xFF, 0)), ("all_zero", 24, (0, 0, 0, 0)),
    ("r_a_no_lum", 16, (0xFF, 0, 0, 0xFF00)), ("rg_a", 32, (0xFF, 0xFF00, 0, 0xFF000000)), ("g_only", 8, (0, 0xFF, 0, 0)),
    ("gb_only", 16, (0, 0xFF00, 0xFF, 0)),
]


def block_cases():
    """Every block format at widths 1-21 x heights 1-9."""
    return [(f"{cc.decode()}_{w}x{h}", block_file(1000 * k + 32 * h + w, cc, w, h))
            for k, cc in enumerate(BLOCK_FOURCCS) for h in range(1, 10) for w in range(1, 22)]


def alias_cases():
    """Every FourCC and DXGI alias of the block formats, the copied forms and the DX10 8-bit forms."""
    out = [(f"cc_{cc.decode()}", block_file(50 + k, cc, 13, 6, tail=k)) for k, cc in enumerate(FOURCC_BC)]
    out += [(f"dxgi_{v}", block_file(70 + v, None, 9, 7, dxgi=v)) for v in DXGI_BC]
    out += [(f"copy_dxgi_{v}", copy_file(90 + v, 7, 5, dxgi=v, nan=True)) for v in DXGI_COPY]
    out += [(f"copy_cc_{v}", copy_file(110 + v, 5, 7, legacy=v, nan=True)) for v in LEGACY_COPY]
    out += [(f"bytes_dxgi_{v}", dx10_header(11, 3, v) + rng(130 + v).integers(0, 256, 11 * 3 * DXGI_BYTES[v][0] // 8,
                                                                               dtype=np.uint8).tobytes()) for v in DXGI_BYTES]
    return out


def mask_cases():
    """Every listed mask set, at a width that is no multiple of 4 and one of 16."""
    out = []
    for k, (name, bits, masks, pff) in enumerate(MASK_SETS):
        out.append((f"mask_{name}_7x3", masked_file(200 + k, 7, 3, bits, masks, pff, tail=k % 3)))
        out.append((f"mask_{name}_16x2", masked_file(300 + k, 16, 2, bits, masks, pff)))
    return out


def field_sweep_cases():
    """Every value of every field of the narrow mask sets once: 2^bits pixels in stored order (16 bits and fewer)."""
    out = []
    for name, bits, masks, pff in MASK_SETS:
        if bits <= 16:
            v = np.arange(1 << bits, dtype="<u4").view(np.uint8).reshape(-1, 4)[:, :bits // 8]
            out.append((f"sweep_{name}", header(1 << (bits // 2), 1 << (bits // 2), pff=pff, bits=bits, masks=masks) + v.tobytes()))
    return out


def error_cases():
    """(name, file, code): every status, in the probe's order of checks."""
    good = block_file(7, b"DXT5", 9, 6)
    raw = masked_file(8, 5, 3, 24, (0xFF0000, 0xFF00, 0xFF, 0))

    def patch(f, at, fmt, *v):
        b = bytearray(f)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    out = [("empty", b"", NOT_DDS), ("three_bytes", b"DDS", NOT_DDS), ("magic", b"DDX " + good[4:], NOT_DDS),
           ("jpeg", b"\xff\xd8\xff\xe0" + bytes(200), NOT_DDS),
           ("magic_only", b"DDS ", BAD_HEADER), ("short_header", good[:127], BAD_HEADER), ("size_123", patch(good, 4, "<I", 123), BAD_HEADER),
           ("pfsize_0", patch(good, 76, "<I", 0), BAD_HEADER), ("width_0", patch(good, 16, "<I", 0), BAD_HEADER),
           ("height_0", patch(good, 12, "<I", 0), BAD_HEADER), ("dx10_short", dx10_header(4, 4, 71)[:147], BAD_HEADER),
           ("bits_0", patch(raw, 88, "<I", 0), BAD_HEADER), ("bits_12", patch(raw, 88, "<I", 12), BAD_HEADER),
           ("bits_64", patch(raw, 88, "<I", 64), BAD_HEADER),
           # BAD_HEADER before UNSUPPORTED, UNSUPPORTED before TOO_LARGE and TRUNCATED
           ("cubemap_width_0", patch(patch(good, 112, "<I", 0x200), 16, "<I", 0), BAD_HEADER),
           ("cubemap", patch(good, 112, "<I", 0x200), UNSUPPORTED), ("cubemap_faces", patch(good, 112, "<I", 0xFE00), UNSUPPORTED),
           ("volume", patch(good, 112, "<I", 0x200000), UNSUPPORTED), ("volume_cut", patch(good, 112, "<I", 0x200000)[:128], UNSUPPORTED),
           ("array_2", dx10_header(4, 4, 71, arr=2) + bytes(16), UNSUPPORTED), ("array_0", dx10_header(4, 4, 71, arr=0) + bytes(8), UNSUPPORTED),
           ("dx10_cube", dx10_header(4, 4, 71, misc=4) + bytes(8), UNSUPPORTED), ("dx10_1d", dx10_header(4, 4, 71, dim=2) + bytes(8), UNSUPPORTED),
           ("dx10_3d", dx10_header(4, 4, 71, dim=4) + bytes(8), UNSUPPORTED), ("huge_unknown", header(1 << 20, 1 << 20, pff=4, fourcc=b"XYZW"), UNSUPPORTED)]
    for cc in (b"BC4S", b"BC5S", b"RGBG", b"GRGB", b"UYVY", b"YUY2", b"XYZW", b"\0\0\0\0", b"dxt1"):
        out.append((f"fourcc_{cc.hex()}", header(4, 4, pff=4, fourcc=cc) + bytes(16), UNSUPPORTED))
    for v in (111, 112, 113, 117, 34, 0, 1, 81, 84, 95, 96, 98, 99, 10, 54, 24, 132):  # halfs, signed, BC6H, BC7, others
        out.append((f"legacy_{v}", header(4, 4, pff=4, fourcc=v) + bytes(64), UNSUPPORTED))
    for v in (0, 1, 3, 10, 13, 24, 34, 54, 70, 73, 76, 79, 81, 82, 84, 85, 86, 95, 96, 98, 99, 115, 132):
        out.append((f"dxgi_{v}", dx10_header(4, 4, v) + bytes(256), UNSUPPORTED))
    out += [(f"mask_{n}", header(4, 4, pff=0x40, bits=b, masks=m) + bytes(64), UNSUPPORTED) for n, b, m in BAD_MASKS]
    out += [("lum_no_r", header(4, 4, pff=0x20000, bits=8, masks=(0, 0, 0, 0xFF)) + bytes(16), UNSUPPORTED),
            ("too_large", header(1 << 15, (1 << 15) + 1, pff=4, fourcc=b"DXT1"), TOO_LARGE),
            ("too_large_wide", header(0xFFFFFFFF, 1, pff=0x40, bits=24, masks=(0xFF0000, 0xFF00, 0xFF, 0)), TOO_LARGE),
            ("too_large_sq", header(0xFFFFFFFF, 0xFFFFFFFF, pff=4, fourcc=b"ATI2"), TOO_LARGE),
            ("just_fits_pixels", header(1 << 15, 1 << 15, pff=4, fourcc=b"DXT1"), TRUNCATED),
            ("header_only", good[:128], TRUNCATED), ("one_short", good[:-1], TRUNCATED), ("raw_one_short", raw[:-1], TRUNCATED),
            ("dx10_one_short", block_file(3, None, 5, 5, dxgi=83)[:-1], TRUNCATED), ("float_one_short", copy_file(4, 3, 3, dxgi=6)[:-1], TRUNCATED),
            ("exact", good, OK), ("mip_tail", good + bytes(range(200)), OK), ("raw_exact", raw, OK), ("raw_tail", raw + b"\xEE" * 40, OK),
            ("flags_0_mips_9", patch(patch(good, 8, "<I", 0), 28, "<I", 9), OK), ("pitch_wrong", patch(raw, 20, "<I", 1), OK)]
    return out


def fuzz_sources(fixture):
    return [block_file(21, b"DXT5", 10, 7), fixture]


def prefixes(src, most=300):
    """Proper prefixes of src: all of them, or for a long file every length through the header and a
    little past it, the last 40, and lengths spread evenly between -- `most` at the most."""
    n = len(src)
    if n <= most:
        return [src[:k] for k in range(n)]
    lens = set(range(160)) | set(range(n - 40, n))
    lens |= set(int(x) for x in np.linspace(160, n - 41, most - len(lens)))
    return [src[:k] for k in sorted(lens)]


def bit_flips(src, seed, count=200):
    """`count` copies of src with one bit of its first 160 bytes flipped (the header and a little of the data)."""
    r = rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(src)
        at = int(r.integers(0, min(len(b), 160)))
        b[at] ^= 1 << int(r.integers(0, 8))
        out.append(bytes(b))
    return out


def synth(seed, w, h, d):
    """Noise over a gradient: an image every encoder path sees something of."""
    r = rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 5 + y * 3)[:, :, None] + 40 * np.arange(d)[None, None, :]) % 256
    return ((base + r.integers(0, 48, (h, w, d))) % 256).astype(np.uint8)


def waves(w=256, h=192):
    """Waves plus noise (seed fixed), d = 3."""
    y, x = np.mgrid[0:h, 0:w]
    r = rng(5)
    img = np.stack([128 + 90 * np.sin(x / 9.0) * np.cos(y / 13.0), 128 + 90 * np.sin((x + y) / 17.0), 128 + 90 * np.cos(x / 5.0 - y / 7.0)], -1)
    return np.clip(img + r.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def encoder_images(d):
    """(name, uint8 (h, w, d)): noise, flat blocks, two-colour blocks, gradients, ties, clamped edges."""
    r = rng(40 + d)
    out = [("noise", r.integers(0, 256, (12, 20, d), dtype=np.uint8)), ("synth", synth(3 + d, 37, 11, d))]
    flat = np.repeat(np.repeat(r.integers(0, 256, (3, 5, d), dtype=np.uint8), 4, 0), 4, 1)
    out.append(("flat", flat))
    two = r.integers(0, 256, (3, 5, 2, d), dtype=np.uint8)
    pick = r.integers(0, 2, (12, 20))
    out.append(("two_colour", two[np.arange(12)[:, None] // 4, np.arange(20)[None, :] // 4, pick]))
    y, x = np.mgrid[0:16, 0:64]
    out.append(("gradient", np.stack([(4 * x + (c + 1) * y) % 256 for c in range(d)], -1).astype(np.uint8)))
    out.append(("gradient_smooth", np.stack([(x + c * y) // (c + 1) for c in range(d)], -1).astype(np.uint8)))
    out.append(("extremes", r.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (8, 16, d))))
    out.append(("ties", tie_image(d)))
    out += [(f"edge_{w}x{h}", synth(100 * w + h, w, h, d)) for h in range(1, 10) for w in range(1, 10)]
    return out


# Values of one channel of a block whose pixels sit exactly between two palette entries.
# Alpha: the endpoints 252 and 0 give 252, 0, 216, 180, 144, 108, 72, 36; each midpoint 234, 198, 162,
# 126, 90, 54, 18 is as far from one entry as from the next (18: entries 7 and 1).
TIE_ALPHA = (252, 0, 234, 198, 162, 126, 90, 54, 18, 216, 180, 144, 108, 72, 36, 235)
# A 5-bit channel: 206 and 8 survive q5 and the expansion, the palette is 206, 8, 140, 74 with gaps of
# 66, so 173, 107 and 41 are midpoints. A 6-bit channel: 190 and 4, palette 190, 4, 128, 66, gaps of 62,
# midpoints 159, 97 and 35. With the other channels constant the squared distance is this channel's.
TIE_5 = (206, 8, 173, 107, 41, 140, 74, 172, 174, 106, 108, 40, 42, 173, 107, 41)
TIE_6 = (190, 4, 159, 97, 35, 128, 66, 158, 160, 96, 98, 34, 36, 159, 97, 35)


def tie_image(d):
    """Blocks with pixels equidistant from two palette entries, in alpha and in each colour channel."""
    def blk(vals):
        return np.array(vals, np.uint8).reshape(4, 4)

    if d <= 2:
        img = np.zeros((4, 8, d), np.uint8)
        for c in range(d):
            img[:, :4, c] = blk(TIE_ALPHA) if c == 0 else blk(TIE_ALPHA).T
            img[:, 4:, c] = blk(TIE_ALPHA)[::-1]
        return img
    img = np.zeros((4, 12, d), np.uint8)
    for c, vals in enumerate((TIE_5, TIE_6, TIE_5)):
        img[:, 4 * c:4 * c + 4, :3] = (90, 60, 30)  # (constant in the block, so of no weight in the distance)
        img[:, 4 * c:4 * c + 4, c] = blk(vals)
    if d == 4:
        img[:, :, 3] = np.tile(blk(TIE_ALPHA), (1, 3))
    return img


def alpha_exhaustive():
    """Every pair a1 < a0 with every value strictly between them, 14 probes to a block (the other
    two pixels are a0 and a1; a last block of a pair repeats its last probe): (N, 16) uint8, about
    195 000 blocks."""
    rows = []
    for gap in range(2, 256):
        a1 = np.arange(0, 256 - gap)
        a0 = a1 + gap
        for j in range(0, gap - 1, 14):
            probes = np.minimum(a1[:, None] + 1 + j + np.arange(14)[None, :], a0[:, None] - 1)
            rows.append(np.concatenate([a0[:, None], a1[:, None], probes], 1))
    return np.concatenate(rows).astype(np.uint8)


def alpha_exhaustive_image():
    """The exhaustive set as one image of d = 1: 512 blocks to a block row."""
    b = alpha_exhaustive()
    n = -(-len(b) // 512) * 512
    b = np.concatenate([b, np.repeat(b[-1:], n - len(b), 0)])
    return b.reshape(n // 512, 512, 4, 4).transpose(0, 2, 1, 3).reshape(n // 512 * 4, 2048, 1)


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / mse)
