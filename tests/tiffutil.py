"""The TIFF read's contract (include/icx.h, "TIFF read") restated serially in Python, and a writer
that crafts the files the tests need.

parse / decode follow the contract's order of checks: the header, the IFD's entries in file order,
then what the tags say together, then the chunks (an image's code is its lowest failing chunk's).
The LZW reader keeps a dictionary of strings; zlib chunks go through Python's zlib as a raw deflate
stream with the two header checks and the Adler-32 of the contract around it.

make_tiff writes II or MM files in strips or tiles, under each compression, with predictor 2,
SHORT or LONG tag forms, sorted or shuffled entries and the chunk data at a chosen offset;
lzw_encode is a writer whose plain output equals libtiff's (tests/test_tiff_core.py) and which can
leave out the EOI or the leading Clear, clear early, or never clear."""
import struct
import zlib

import numpy as np

OK, NOT_TIFF, BAD_HEADER, UNSUPPORTED, MALFORMED, BAD_DATA, TRUNCATED, TOO_LARGE = range(8)
INTERNAL_ERR = -1
MAX_CHUNKS = 4096
LZW_LAST_T = 3837  # the last code number after a Clear (from 0) that may add an entry: 257 + t = 4094

SCALAR = {256, 257, 259, 262, 266, 274, 277, 278, 284, 317, 322, 323}
ARRAY = {273, 279, 324, 325}
SHORT_ARRAY = {258, 320, 339}


# ------------------------------------------------------------------------------ restatement
def parse(f):
    """(code, head): head is a dict when code is OK."""
    n = len(f)
    if n < 8:
        return NOT_TIFF, None
    if f[:2] == b"II":
        E = "<"
    elif f[:2] == b"MM":
        E = ">"
    else:
        return NOT_TIFF, None
    magic = struct.unpack(E + "H", f[2:4])[0]
    if magic == 43:
        return UNSUPPORTED, None
    if magic != 42:
        return NOT_TIFF, None
    ifd = struct.unpack(E + "I", f[4:8])[0]
    if ifd + 2 > n:
        return BAD_HEADER, None
    ne = struct.unpack(E + "H", f[ifd:ifd + 2])[0]
    if ifd + 2 + 12 * ne > n:
        return BAD_HEADER, None
    T = {}
    for e in range(ne):
        p = ifd + 2 + 12 * e
        tag, typ, count = struct.unpack(E + "HHI", f[p:p + 8])
        if tag not in SCALAR and tag not in ARRAY and tag not in SHORT_ARRAY:
            continue
        if not (typ == 3 or (typ == 4 and tag not in SHORT_ARRAY)):
            return MALFORMED, None
        if (count != 1) if tag in SCALAR else (count == 0):
            return MALFORMED, None
        if tag == 320 and count != 768:
            return MALFORMED, None
        size = 2 if typ == 3 else 4
        at = p + 8
        if count * size > 4:
            at = struct.unpack(E + "I", f[p + 8:p + 12])[0]
            if at + count * size > n:
                return TRUNCATED, None
        T[tag] = (typ, count, at)

    def vals(tag, limit=None):
        typ, count, at = T[tag]
        k = count if limit is None else min(count, limit)
        return list(struct.unpack(E + ("H" if typ == 3 else "I") * k, f[at:at + k * (2 if typ == 3 else 4)]))

    def val(tag, default):
        return vals(tag, 1)[0] if tag in T else default

    w, h = val(256, 0), val(257, 0)
    if w == 0 or h == 0:
        return BAD_HEADER, None
    if 273 not in T and 324 not in T:
        return BAD_HEADER, None
    spp, comp, photo = val(277, 1), val(259, 1), val(262, None)
    if 258 not in T or spp not in (1, 3, 4) or T[258][1] != spp or any(v != 8 for v in vals(258, 4)):
        return UNSUPPORTED, None
    if comp not in (1, 5, 8, 32946, 32773):
        return UNSUPPORTED, None
    if not ((photo in (0, 1, 3) and spp == 1) or (photo == 2 and spp >= 3)):
        return UNSUPPORTED, None
    planar = val(284, 1)
    if not (planar == 1 or (planar == 2 and spp == 1)):
        return UNSUPPORTED, None
    pred = val(317, 1)
    if val(274, 1) != 1 or val(266, 1) != 1 or (339 in T and any(v != 1 for v in vals(339, 4))) or pred not in (1, 2):
        return UNSUPPORTED, None
    strips = 273 in T or 279 in T
    tiles = any(t in T for t in (322, 323, 324, 325))
    if strips and tiles:
        return MALFORMED, None
    if tiles:
        if not all(t in T for t in (322, 323, 324, 325)) or val(322, 0) == 0 or val(323, 0) == 0:
            return MALFORMED, None
        cw, ch = val(322, 0), val(323, 0)
        ot, ct = 324, 325
    else:
        rps = val(278, 0xFFFFFFFF)
        if 279 not in T or rps == 0:
            return MALFORMED, None
        cw, ch = w, min(rps, h)
        ot, ct = 273, 279
    across, down = -(-w // cw), -(-h // ch)
    nchunks = across * down
    if T[ot][1] != nchunks or T[ct][1] != nchunks:
        return MALFORMED, None
    if photo == 3 and 320 not in T:
        return MALFORMED, None
    if cw > 1 << 30 or ch > 1 << 30 or w * h > 1 << 30 or nchunks > MAX_CHUNKS:
        return TOO_LARGE, None
    if across * cw * down * ch > 1 << 30 or cw * ch * spp >= 1 << 31:
        return TOO_LARGE, None
    H = dict(w=w, h=h, spp=spp, d=3 if photo == 3 else spp, photo=photo, comp=comp,
             pred=2 if pred == 2 and comp in (5, 8, 32946) else 1, tiled=tiles, cw=cw, ch=ch, across=across, down=down,
             nchunks=nchunks, offsets=vals(ot), counts=vals(ct), E=E)
    if photo == 3:
        cm = np.array(vals(320), np.uint32).reshape(3, 256)
        H["pal"] = (cm >> 8).astype(np.uint8).T.copy()  # (256, 3)
    return OK, H


def chunk_room(H):
    return (H["cw"] * H["ch"] * H["spp"] + 15) & ~15


def scratch_slot(max_w, max_h):
    px = max_w * max_h
    return ((4 * px + 15) & ~15) + 16 * min(px, MAX_CHUNKS)


def code_width(t):
    return 9 + (t >= 254) + (t >= 766) + (t >= 1790)


def lzw_decode(s, want):
    """(code, bytes): exactly `want` bytes or why not."""
    if len(s) >= 2 and s[0] == 0 and s[1] & 1:
        return UNSUPPORTED, None
    nbits = len(s) * 8
    big = int.from_bytes(s, "big")
    bit = t = 0
    started = False
    out = bytearray()
    table = {}
    prev = None
    while len(out) < want:
        width = code_width(t)
        if bit + width > nbits:
            return BAD_DATA, None
        code = (big >> (nbits - bit - width)) & ((1 << width) - 1)
        bit += width
        if not started:
            if code != 256:
                return BAD_DATA, None
            started = True
            continue
        if code == 256:
            t, table = 0, {}
            continue
        if code == 257:
            return BAD_DATA, None
        if t == 0:
            if code >= 256:
                return BAD_DATA, None
            prev = bytes([code])
            out += prev
            t = 1
            continue
        entry = 257 + t
        if t > LZW_LAST_T or code > entry:
            return BAD_DATA, None
        cur = bytes([code]) if code < 256 else prev + prev[:1] if code == entry else table[code]
        table[entry] = prev + cur[:1]
        out += cur
        prev = cur
        t += 1
    return OK, bytes(out[:want])


def packbits_decode(s, want):
    p, out = 0, bytearray()
    while len(out) < want:
        if p >= len(s):
            return BAD_DATA, None
        hb = s[p]
        if hb == 128:
            p += 1
            continue
        m, need = (hb + 1, hb + 2) if hb < 128 else (257 - hb, 2)
        if p + need > len(s):
            return BAD_DATA, None
        out += s[p + 1:p + 1 + m] if hb < 128 else s[p + 1:p + 2] * m
        p += need
    return OK, bytes(out[:want])


def zlib_decode(s, want):
    """Exactly `want` bytes, no more; the header checks and the Adler-32 of the shared inflate."""
    if len(s) < 2 or (s[0] * 256 + s[1]) % 31 or s[1] & 32 or (s[0] & 15) != 8:
        return BAD_DATA, None
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(s[2:], want + 1)
    except zlib.error:
        return BAD_DATA, None
    if not d.eof or len(out) != want:
        return BAD_DATA, None
    tail = d.unused_data[:4]
    if len(tail) < 4 or int.from_bytes(tail, "big") != zlib.adler32(out):
        return BAD_DATA, None
    return OK, out


def decode(f, max_w=None, max_h=None):
    """(code, w, h, d, uint8 (h, w, d) or None). max_w / max_h: the batch workspace's limits."""
    code, H = parse(f)
    if code != OK:
        return code, 0, 0, 0, None
    w, h, spp, d = H["w"], H["h"], H["spp"], H["d"]
    if max_w is not None and (w > max_w or h > max_h or H["nchunks"] * chunk_room(H) > scratch_slot(max_w, max_h)):
        return TOO_LARGE, 0, 0, 0, None
    img = np.zeros((h, w, d), np.uint8)
    for k in range(H["nchunks"]):
        cx, cy = k % H["across"], k // H["across"]
        x0, y0 = cx * H["cw"], cy * H["ch"]
        cols, rows = min(H["cw"], w - x0), min(H["ch"], h - y0)
        row_bytes = H["cw"] * spp
        want = (H["ch"] if H["tiled"] else rows) * row_bytes
        off, cnt = H["offsets"][k], H["counts"][k]
        if off + cnt > len(f):
            return TRUNCATED, 0, 0, 0, None
        s = f[off:off + cnt]
        if H["comp"] == 1:
            rc, raw = (OK, s[:want]) if cnt >= want else (BAD_DATA, None)
        elif H["comp"] == 5:
            rc, raw = lzw_decode(s, want)
        elif H["comp"] == 32773:
            rc, raw = packbits_decode(s, want)
        else:
            rc, raw = zlib_decode(s, want)
        if rc != OK:
            return rc, 0, 0, 0, None
        a = np.frombuffer(raw, np.uint8).reshape(-1, H["cw"], spp)[:rows]
        if H["pred"] == 2:
            a = np.cumsum(a, axis=1, dtype=np.uint32).astype(np.uint8)
        a = a[:, :cols]
        if H["photo"] == 0:
            a = 255 - a
        elif H["photo"] == 3:
            a = H["pal"][a[:, :, 0]]
        img[y0:y0 + rows, x0:x0 + cols] = a
    return OK, w, h, d, img


# ------------------------------------------------------------------------------ writers
class _Bits:
    def __init__(self):
        self.acc = self.n = 0

    def put(self, code, width):
        self.acc = self.acc << width | code
        self.n += width

    def bytes(self):
        pad = -self.n % 8
        return (self.acc << pad).to_bytes((self.n + pad) // 8, "big")


def lzw_encode(data, eoi=True, clear_every=None, lead_clear=True, never_clear=False):
    """libtiff's stream for `data` (MSB first, early change, a Clear once 3836 codes have followed
    the last one: the next free entry is then 4094). eoi=False leaves the EOI out; clear_every=N
    clears after every N codes; lead_clear=False leaves the first Clear out; never_clear goes on
    past the table's end with 12-bit codes."""
    B = _Bits()
    if lead_clear:
        B.put(256, 9)
    t, table, nxt = 0, {}, 258
    cur = None

    def emit(code):
        nonlocal t, table, nxt
        B.put(code, code_width(t))
        t += 1
        if (clear_every and t == clear_every) or (not never_clear and not clear_every and t == LZW_LAST_T - 1):
            B.put(256, code_width(t))
            t, table, nxt = 0, {}, 258
            return True
        return False

    for b in bytes(data):
        if cur is None:
            cur = b
        elif (cur, b) in table:
            cur = table[(cur, b)]
        else:
            cleared = emit(cur)
            if not cleared and nxt < 4096:
                table[(cur, b)] = nxt
                nxt += 1
            cur = b
    if cur is not None:
        emit(cur)
    if eoi:
        B.put(257, code_width(t))
    return B.bytes()


def lzw_from_codes(codes):
    """A stream from explicit codes, each at the width its place after the last Clear gives it (the
    very first code counts as t = 0)."""
    B = _Bits()
    t, started = 0, False
    for c in codes:
        B.put(c, code_width(t))
        if not started:
            started = True
            if c == 256:
                continue
        if c == 256:
            t = 0
        else:
            t += 1
    return B.bytes()


def packbits_encode(data, row_bytes):
    """Row by row: runs of three or more as repeat packets, the rest as literals."""
    out = bytearray()
    data = bytes(data)
    for r0 in range(0, len(data), row_bytes):
        row = data[r0:r0 + row_bytes]
        i, lit = 0, bytearray()

        def flush():
            for q in range(0, len(lit), 128):
                part = lit[q:q + 128]
                out.append(len(part) - 1)
                out.extend(part)
            lit.clear()

        while i < len(row):
            j = i
            while j < len(row) and row[j] == row[i] and j - i < 128:
                j += 1
            if j - i >= 3:
                flush()
                out.append(257 - (j - i))
                out.append(row[i])
            else:
                lit += row[i:j]
            i = j
        flush()
    return bytes(out)


def packbits_packets(packets):
    """('lit', bytes) | ('rep', n, byte) | ('nop',) -> stream and what it decodes to."""
    s, out = bytearray(), bytearray()
    for p in packets:
        if p[0] == "lit":
            s.append(len(p[1]) - 1)
            s += p[1]
            out += p[1]
        elif p[0] == "rep":
            s.append(257 - p[1])
            s.append(p[2])
            out += bytes([p[2]]) * p[1]
        else:
            s.append(128)
    return bytes(s), bytes(out)


def compress(raw, comp, row_bytes, zlevel=6, lzw=None):
    if comp == 1:
        return bytes(raw)
    if comp == 5:
        return lzw_encode(raw, **(lzw or {}))
    if comp == 32773:
        return packbits_encode(raw, row_bytes)
    c = zlib.compressobj(zlevel)
    return c.compress(bytes(raw)) + c.flush()


def make_tiff(arr, be=False, comp=1, pred=1, rps=None, tile=None, photo=None, cmap=None, long_tags=False, shuffle=None,
              data_at=8, zlevel=6, lzw=None, chunks=None, override=None, drop=(), honour_pred=None, trailer=b""):
    """arr: the stored samples, (h, w) or (h, w, spp). tile=(tw, tl) or strips of rps rows (None: one
    strip). chunks: {k: bytes} replaces chunk k's data. override: {tag: (type, [values])} replaces or
    adds an entry (None values drop nothing); drop: tags left out. shuffle: a seed for the entry
    order. data_at: file offset of the first chunk. honour_pred: difference the samples (default:
    when pred == 2 and the compression honours it)."""
    a = np.asarray(arr, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, spp = a.shape
    if photo is None:
        photo = 1 if spp == 1 else 2
    E = ">" if be else "<"
    if tile:
        cw, ch = tile
    else:
        cw, ch = w, min(rps or h, h)
    across, down = -(-w // cw), -(-h // ch)
    if honour_pred is None:
        honour_pred = pred == 2 and comp in (5, 8, 32946)
    datas = []
    for k in range(across * down):
        cx, cy = k % across, k // across
        rows_store = ch if tile else min(ch, h - cy * ch)
        blk = np.zeros((rows_store, cw, spp), np.uint8)
        part = a[cy * ch:cy * ch + ch, cx * cw:cx * cw + cw]
        blk[:part.shape[0], :part.shape[1]] = part
        if honour_pred:
            blk = np.concatenate([blk[:, :1], (blk[:, 1:].astype(np.int16) - blk[:, :-1]).astype(np.uint8)], axis=1)
        datas.append(compress(blk.tobytes(), comp, cw * spp, zlevel, lzw))
    for k, v in (chunks or {}).items():
        datas[k] = bytes(v)
    body = bytearray(b"\0" * (data_at - 8))
    offsets = []
    for dta in datas:
        offsets.append(8 + len(body))
        body += dta
    S, L = 3, 4
    big = L if long_tags else S
    tags = {256: (big, [w]), 257: (big, [h]), 258: (S, [8] * spp), 259: (S, [comp]), 262: (S, [photo]), 277: (S, [spp]),
            284: (S, [1])}
    fits = lambda v: L if long_tags or max(v) > 65535 else S
    if tile:
        tags.update({322: (big, [cw]), 323: (big, [ch]), 324: (L, offsets), 325: (fits([len(x) for x in datas]), [len(x) for x in datas])})
    else:
        tags.update({273: (fits(offsets), offsets), 279: (fits([len(x) for x in datas]), [len(x) for x in datas])})
        if rps is not None:
            tags[278] = (big, [rps])
    if pred != 1:
        tags[317] = (S, [pred])
    if spp == 4:
        tags[338] = (S, [2])
    if photo == 3:
        cm = np.asarray(cmap if cmap is not None else palette16(), np.uint16).reshape(3, 256)
        tags[320] = (S, [int(v) for v in cm.reshape(-1)])
    for t, v in (override or {}).items():
        tags[t] = v
    for t in drop:
        tags.pop(t, None)
    order = sorted(tags)
    if shuffle is not None:
        order = [order[i] for i in np.random.default_rng(shuffle).permutation(len(order))]
    entries = []
    for t in order:
        typ, v = tags[t]
        count = len(v)
        if isinstance(typ, tuple):  # (type, count): a count that is not the number of values written
            typ, count = typ
        raw = struct.pack(E + {1: "B", 2: "B", 3: "H", 4: "I", 5: "I"}.get(typ, "H") * len(v), *v)
        if len(raw) <= 4 and count * {3: 2, 4: 4}.get(typ, 1) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            if len(body) & 1:
                body += b"\0"
            field = struct.pack(E + "I", 8 + len(body))
            body += raw
        entries.append(struct.pack(E + "HHI", t, typ, count) + field)
    if len(body) & 1:
        body += b"\0"
    ifd = 8 + len(body)
    head = (b"MM" if be else b"II") + struct.pack(E + "HI", 42, ifd)
    return head + bytes(body) + struct.pack(E + "H", len(entries)) + b"".join(entries) + struct.pack(E + "I", 0) + trailer


def palette16(seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 65536, (3, 256), dtype=np.uint16)


def noise(seed, h, w, spp=1, levels=256):
    a = np.random.default_rng(seed).integers(0, levels, (h, w, spp), dtype=np.uint8)
    return a[:, :, 0] if spp == 1 else a


def smooth(seed, h, w, spp=1):
    """A picture with runs and gradients: compressible under every scheme."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [((x * (3 + s) + y * (5 - s) + seed) // 4 % 256) for s in range(spp)]
    a = np.stack(planes, axis=2).astype(np.uint8)
    a[h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 2)] = 77
    return a[:, :, 0] if spp == 1 else a


COMPS = (("raw", 1), ("lzw", 5), ("deflate", 8), ("zip32946", 32946), ("packbits", 32773))


def corpus():
    """(name, file) of accepted files: every compression x predictor x layout over small shapes."""
    out = []
    for cname, comp in COMPS:
        for pred in (1, 2):
            for spp in (1, 3, 4):
                a = smooth(spp, 9, 21, spp)
                out.append((f"{cname}_p{pred}_s{spp}_strips3", make_tiff(a, comp=comp, pred=pred, rps=3)))
            out.append((f"{cname}_p{pred}_tiles", make_tiff(smooth(7, 33, 17, 3), comp=comp, pred=pred, tile=(16, 16))))
        out.append((f"{cname}_mm_long_shuffled", make_tiff(noise(3, 7, 22, 3), be=True, comp=comp, rps=4, long_tags=True, shuffle=5)))
        out.append((f"{cname}_miniswhite", make_tiff(noise(4, 5, 5), comp=comp, photo=0, pred=2)))
        out.append((f"{cname}_palette", make_tiff(noise(5, 6, 65), comp=comp, photo=3, rps=4)))
        out.append((f"{cname}_palette_mm_tiles", make_tiff(noise(6, 20, 20), be=True, comp=comp, photo=3, tile=(7, 9))))
    out.append(("one_strip_no_rps", make_tiff(noise(8, 4, 4, 3))))
    out.append(("rps_above_height", make_tiff(noise(9, 4, 4), rps=1000)))
    out.append(("planar2_spp1", make_tiff(noise(10, 4, 4), override={284: (3, [2])})))
    out.append(("extra_unknown_tags", make_tiff(noise(11, 4, 4), override={305: (2, list(b"crafted\0")), 700: (1, [1, 2, 3])})))
    out.append(("raw_pred2_ignored", make_tiff(noise(12, 4, 9, 3), pred=2)))
    out.append(("packbits_pred2_ignored", make_tiff(smooth(13, 4, 9, 3), comp=32773, pred=2)))
    out.append(("raw_longer_chunk", make_tiff(noise(14, 3, 3), chunks={0: bytes(range(20))})))
    out.append(("lzw_no_eoi", make_tiff(smooth(15, 9, 33), comp=5, lzw={"eoi": False})))
    out.append(("lzw_clear_every_10", make_tiff(smooth(16, 9, 33), comp=5, lzw={"clear_every": 10})))
    out.append(("lzw_kwkwk", make_tiff(np.full((8, 200), 9, np.uint8), comp=5)))
    out.append(("lzw_trailing_bytes", make_tiff(noise(17, 3, 5), comp=5, chunks={0: lzw_encode(noise(17, 3, 5).tobytes()) + b"\xff\x00\xff"})))
    out.append(("zlib_trailing_bytes", make_tiff(noise(18, 3, 5), comp=8, chunks={0: zlib.compress(noise(18, 3, 5).tobytes()) + b"junk"})))
    return out


def status_cases():
    """(name, file, code)."""
    a = noise(20, 6, 10, 3)
    good = make_tiff(a, comp=5, rps=2)
    ifd = struct.unpack("<I", good[4:8])[0]
    big = bytearray(good)
    big[2:4] = struct.pack("<H", 43)
    lz = lzw_encode(a[:2].tobytes())
    n2 = a[:2].size
    cases = [
        ("ok", good, OK),
        ("empty", b"", NOT_TIFF),
        ("seven_bytes", good[:7], NOT_TIFF),
        ("bad_order", b"IM" + good[2:], NOT_TIFF),
        ("bad_magic", good[:2] + b"\x2b\x2a" + good[4:], NOT_TIFF),
        ("bigtiff", bytes(big), UNSUPPORTED),
        ("ifd_outside", good[:4] + struct.pack("<I", len(good)) + good[8:], BAD_HEADER),
        ("entries_outside", good[:ifd + 20], BAD_HEADER),
        ("no_width", make_tiff(a, drop=(256,)), BAD_HEADER),
        ("zero_height", make_tiff(a, override={257: (3, [0])}), BAD_HEADER),
        ("no_offsets", make_tiff(a, drop=(273,)), BAD_HEADER),
        ("no_bps", make_tiff(a, drop=(258,)), UNSUPPORTED),
        ("bps_16", make_tiff(a, override={258: (3, [16, 16, 16])}), UNSUPPORTED),
        ("bps_one_for_three", make_tiff(a, override={258: (3, [8])}), UNSUPPORTED),
        ("spp_2", make_tiff(noise(1, 4, 4, 3)[:, :, :2], photo=1), UNSUPPORTED),
        ("jpeg_compression", make_tiff(a, override={259: (3, [7])}), UNSUPPORTED),
        ("ycbcr", make_tiff(a, photo=6), UNSUPPORTED),
        ("no_photometric", make_tiff(a, drop=(262,)), UNSUPPORTED),
        ("rgb_with_one_sample", make_tiff(noise(1, 4, 4), photo=2), UNSUPPORTED),
        ("planar2_rgb", make_tiff(a, override={284: (3, [2])}), UNSUPPORTED),
        ("orientation_3", make_tiff(a, override={274: (3, [3])}), UNSUPPORTED),
        ("fill_order_2", make_tiff(a, override={266: (3, [2])}), UNSUPPORTED),
        ("float_samples", make_tiff(a, override={339: (3, [3, 3, 3])}), UNSUPPORTED),
        ("predictor_3", make_tiff(a, comp=5, override={317: (3, [3])}), UNSUPPORTED),
        ("width_as_byte", make_tiff(a, override={256: (1, [10])}), MALFORMED),
        ("bps_as_long", make_tiff(a, override={258: (4, [8, 8, 8])}), MALFORMED),
        ("compression_count_2", make_tiff(a, override={259: (3, [1, 1])}), MALFORMED),
        ("offsets_count_0", make_tiff(a, override={273: ((4, 0), [8])}), MALFORMED),
        ("one_count_short", make_tiff(a, rps=2, override={279: (3, [60, 60])}), MALFORMED),
        ("offsets_not_chunk_count", make_tiff(a, rps=2, override={273: (3, [8, 68]), 279: (3, [60, 60])}), MALFORMED),
        ("no_byte_counts", make_tiff(a, drop=(279,)), MALFORMED),
        ("rps_zero", make_tiff(a, override={278: (3, [0])}), MALFORMED),
        ("strips_and_tiles", make_tiff(a, override={322: (3, [16])}), MALFORMED),
        ("tile_width_zero", make_tiff(a, tile=(16, 16), override={322: (3, [0])}), MALFORMED),
        ("tiles_without_length", make_tiff(a, tile=(16, 16), drop=(323,)), MALFORMED),
        ("palette_without_map", make_tiff(noise(1, 4, 4), photo=3, drop=(320,)), MALFORMED),
        ("colormap_of_48", make_tiff(noise(1, 4, 4), photo=3, override={320: (3, [0] * 48)}), MALFORMED),
        ("array_past_file", make_tiff(noise(1, 4, 4), photo=3, override={320: ((3, 768), [0] * 700)})[:-4], TRUNCATED),
        ("chunk_past_file", make_tiff(a, rps=2, override={279: (3, [60, 60, 6000])}), TRUNCATED),
        ("too_many_chunks", make_tiff(np.zeros((4097, 1), np.uint8), rps=1), TOO_LARGE),
        ("too_many_pixels", make_tiff(noise(1, 2, 2), override={256: (4, [40000]), 257: (4, [40000])}), TOO_LARGE),
        ("huge_tile", make_tiff(noise(1, 2, 2), tile=(2, 2), override={322: (4, [1 << 31])}), TOO_LARGE),
        ("raw_short_chunk", make_tiff(a, rps=2, chunks={1: b"\0" * 59}), BAD_DATA),
        ("lzw_no_leading_clear", make_tiff(a, comp=5, rps=2, chunks={1: lzw_encode(a[2:4].tobytes(), lead_clear=False)}), BAD_DATA),
        ("lzw_first_not_literal", make_tiff(a, comp=5, rps=2, chunks={0: lzw_from_codes([256, 258, 1, 2])}), BAD_DATA),
        ("lzw_code_above_next", make_tiff(a, comp=5, rps=2, chunks={0: lzw_from_codes([256, 1, 2, 261, 3])}), BAD_DATA),
        ("lzw_eoi_early", make_tiff(a, comp=5, rps=2, chunks={2: lzw_from_codes([256, 1, 2, 257])}), BAD_DATA),
        ("lzw_cut", make_tiff(a, comp=5, rps=2, chunks={2: lz[:len(lz) // 2]}), BAD_DATA),
        ("lzw_empty_chunk", make_tiff(a, comp=5, rps=2, chunks={2: b""}), BAD_DATA),
        ("lzw_old_style", make_tiff(a, comp=5, rps=2, chunks={1: b"\x00\x01" + lz}), UNSUPPORTED),
        ("packbits_packet_past_input", make_tiff(a, comp=32773, rps=2, chunks={1: bytes([n2 - 1]) + bytes(n2 - 1)}), BAD_DATA),
        ("packbits_short", make_tiff(a, comp=32773, rps=2, chunks={1: bytes([257 - 59, 7])}), BAD_DATA),
        ("zlib_longer_stream", make_tiff(a, comp=8, rps=2, chunks={1: zlib.compress(bytes(n2 + 1))}), BAD_DATA),
        ("zlib_shorter_stream", make_tiff(a, comp=8, rps=2, chunks={1: zlib.compress(bytes(n2 - 1))}), BAD_DATA),
        ("zlib_bad_adler", make_tiff(a, comp=8, rps=2, chunks={1: zlib.compress(bytes(n2))[:-1] + b"\x55"}), BAD_DATA),
        ("zlib_cut", make_tiff(a, comp=8, rps=2, chunks={1: zlib.compress(a[2:4].tobytes())[:20]}), BAD_DATA),
        ("lowest_failing_chunk_wins", make_tiff(a, comp=5, rps=2, chunks={1: b"\x00\x01" + lz, 2: b""}), UNSUPPORTED),
    ]
    return cases


def lzw_never_clear_file():
    """97 x 131 noise in one strip whose LZW stream never clears: BAD_DATA at the 3839th code."""
    a = noise(30, 131, 97)
    return make_tiff(a, comp=5, lzw={"never_clear": True})


def base_file():
    """A small file with every kind of field the walk reads: the base of prefixes and mutants."""
    return make_tiff(smooth(40, 5, 6), comp=5, pred=2, photo=3, rps=2, shuffle=3)


def mutants(base, count=200, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(base)
        # (the ColorMap's 1536 bytes would take most hits: two thirds of the mutants go outside it)
        pos = int(rng.integers(0, len(b)))
        if k % 3 and len(b) > 1700:
            pos = int(rng.choice(np.r_[0:80, len(b) - 160:len(b)]))
        b[pos] ^= 1 << int(rng.integers(0, 8))
        out.append((f"mutant{k}", bytes(b)))
    return out
