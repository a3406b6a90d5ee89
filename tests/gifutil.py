"""GIF test tools: a container writer, an LZW crafter (an explicit code list -> bits under the
GIF width rule -> sub-blocks of given sizes), a plain LZW coder that yields such code lists, and
a serial restatement of the read contract of include/icx.h in classic dictionary form (a table of
strings; nothing of the kernel's offsets, substrings or lanes)."""
import itertools

import numpy as np

OK, NOT_GIF, BAD_HEADER, MALFORMED, BAD_DATA, TRUNCATED, TOO_LARGE = range(7)
INTERNAL_ERR = -1


# ------------------------------------------------------------------------------------ writer
def u16(v):
    return bytes([v & 255, v >> 8])


def table_bytes(pal):
    """pal: (k, 3) uint8 with k a power of two in 2..256 -> (the 3 size bits, the bytes)."""
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    k = len(pal)
    assert k in (2, 4, 8, 16, 32, 64, 128, 256)
    return k.bit_length() - 2, pal.tobytes()


def screen(w, h, gct=None, bg=0, version=b"89a"):
    flags, body = 0, b""
    if gct is not None:
        bits, body = table_bytes(gct)
        flags = 0x80 | 0x70 | bits
    return b"GIF" + version + u16(w) + u16(h) + bytes([flags, bg, 0]) + body


def extension(label, *blocks):
    return bytes([0x21, label]) + b"".join(bytes([len(b)]) + bytes(b) for b in blocks) + b"\0"


def gce(transparent=None, index=0, disposal=0):
    return extension(0xF9, bytes([(disposal << 2) | (1 if transparent else 0), 0, 0, index]))


def descriptor(fx, fy, fw, fh, lct=None, interlace=False):
    flags, body = 0x40 if interlace else 0, b""
    if lct is not None:
        bits, body = table_bytes(lct)
        flags |= 0x80 | bits
    return b"," + u16(fx) + u16(fy) + u16(fw) + u16(fh) + bytes([flags]) + body


def pack_codes(codes, mcs):
    """The crafter: the codes as bits, each as wide as a reader following the width rule expects
    it (whatever the codes are: clear, stop and invalid codes included)."""
    clear, stop = 1 << mcs, (1 << mcs) + 1
    width, nxt, prev = mcs + 1, clear + 2, False
    acc = nbits = 0
    out = bytearray()
    for c in codes:
        assert 0 <= c < (1 << width), (c, width)
        acc |= c << nbits
        nbits += width
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8
        if c == clear:
            width, nxt, prev = mcs + 1, clear + 2, False
        elif c != stop:
            if prev and nxt < 4096:
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
            prev = True
    if nbits:
        out.append(acc & 255)
    return bytes(out)


def sub_blocks(payload, plan=(255,), terminator=True):
    """payload cut into sub-blocks whose sizes cycle through `plan` (1..255 each)."""
    out, p = bytearray(), 0
    for sz in itertools.cycle(plan):
        if p >= len(payload):
            break
        assert 1 <= sz <= 255
        chunk = payload[p:p + sz]
        out.append(len(chunk))
        out += chunk
        p += len(chunk)
    if terminator:
        out.append(0)
    return bytes(out)


def lzw_codes(indices, mcs, lead_clear=True, stop=True, clear_at=None, use_table=True):
    """A greedy LZW coder -> code list. clear_at(next_free_entry, codes_so_far) -> True emits a
    clear code after the current code; by default none is ever emitted, so a long input fills the
    table and goes on with 12-bit codes (the deferred clear)."""
    clear = 1 << mcs
    codes = [clear] if lead_clear else []
    idx = [int(v) for v in np.asarray(indices).reshape(-1)]
    assert all(v < clear for v in idx)
    table, nxt = {}, clear + 2
    if idx:
        w = idx[0]
        for k in idx[1:]:
            if use_table and (w, k) in table:
                w = table[(w, k)]
                continue
            codes.append(w)
            if nxt < 4096:
                table[(w, k)] = nxt
                nxt += 1
            if clear_at is not None and clear_at(nxt, codes):
                codes.append(clear)
                table, nxt = {}, clear + 2
            w = k
        codes.append(w)
    if stop:
        codes.append(clear + 1)
    return codes


def image_data(codes, mcs, plan=(255,), terminator=True):
    return bytes([mcs]) + sub_blocks(pack_codes(codes, mcs), plan, terminator)


def simple_gif(idx, pal, mcs=None, interlace=False, plan=(255,), bg=0, version=b"89a", pre=b"", post=b";", **kw):
    """A full-canvas file of the index image `idx` (h, w); rows are put in interlace order when asked."""
    idx = np.asarray(idx, np.uint8)
    h, w = idx.shape
    if mcs is None:
        mcs = max(2, (len(np.asarray(pal).reshape(-1, 3)) - 1).bit_length())
    rows = idx[interlace_order(h)] if interlace else idx
    return (screen(w, h, pal, bg, version) + pre + descriptor(0, 0, w, h, interlace=interlace) +
            image_data(lzw_codes(rows, mcs, **kw), mcs, plan) + post)


def interlace_order(h):
    """Frame rows in stream order."""
    return [y for a, b in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(a, h, b)]


def palette(k, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (k, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------ restatement
def parse(d):
    """-> (code, fields). The container walk of the contract, in file order."""
    n = len(d)
    F = dict(has_image=False, transparent=None)
    if n >= 6 and (d[:4] != b"GIF8" or d[4:5] not in (b"7", b"9") or d[5:6] != b"a"):
        return NOT_GIF, F
    if n < 13:
        return BAD_HEADER, F
    W, H = d[6] | d[7] << 8, d[8] | d[9] << 8
    if W == 0 or H == 0:
        return BAD_HEADER, F
    F.update(W=W, H=H, bg=d[11], gct=None)
    p = 13
    if d[10] & 0x80:
        k = 1 << ((d[10] & 7) + 1)
        if p + 3 * k > n:
            return TRUNCATED, F
        F["gct"] = np.frombuffer(d[p:p + 3 * k], np.uint8).reshape(k, 3)
        p += 3 * k
    while True:
        if p >= n:
            return TRUNCATED, F
        sep = d[p]
        if sep == 0x3B:
            return OK, F
        if sep == 0x21:
            if p + 1 >= n:
                return TRUNCATED, F
            label = d[p + 1]
            p += 2
            first = True
            while True:
                if p >= n:
                    return TRUNCATED, F
                sz = d[p]
                if sz == 0:
                    p += 1
                    break
                if p + 1 + sz > n:
                    return TRUNCATED, F
                if first and label == 0xF9 and sz >= 4:
                    F["transparent"] = d[p + 4] if d[p + 1] & 1 else None
                first = False
                p += 1 + sz
            continue
        if sep != 0x2C:
            return MALFORMED, F
        if p + 10 > n:
            return TRUNCATED, F
        fx, fy, fw, fh = (d[p + 1 + 2 * k] | d[p + 2 + 2 * k] << 8 for k in range(4))
        fl = d[p + 9]
        p += 10
        if fx >= W or fy >= H:
            return MALFORMED, F
        if not fl & 0x80 and F["gct"] is None:
            return MALFORMED, F
        pal = F["gct"]
        if fl & 0x80:
            k = 1 << ((fl & 7) + 1)
            if p + 3 * k > n:
                return TRUNCATED, F
            pal = np.frombuffer(d[p:p + 3 * k], np.uint8).reshape(k, 3)
            p += 3 * k
        if p >= n:
            return TRUNCATED, F
        mcs = d[p]
        if not 2 <= mcs <= 8:
            return BAD_DATA, F
        F.update(has_image=True, fx=fx, fy=fy, fw=fw, fh=fh, interlace=bool(fl & 0x40), pal=pal, mcs=mcs, data_at=p + 1)
        return OK, F


def data_stream(d, p):
    """The data sub-blocks' payload from offset p -> (bytes, 'term' | 'file': how it ends)."""
    n, out = len(d), bytearray()
    while True:
        if p >= n:
            return bytes(out), "file"
        sz = d[p]
        if sz == 0:
            return bytes(out), "term"
        chunk = d[p + 1:p + 1 + sz]
        out += chunk
        if len(chunk) < sz:
            return bytes(out), "file"
        p += 1 + sz


def lzw_decode(stream, end, mcs, npix):
    """-> (code, the index bytes produced, at most npix)."""
    clear, stop = 1 << mcs, (1 << mcs) + 1
    bits, nbits, bp = int.from_bytes(stream, "little"), 8 * len(stream), 0
    out = bytearray()
    table, width, prev = {}, mcs + 1, None
    nxt = clear + 2
    while len(out) < npix:
        if bp + width > nbits:
            return (TRUNCATED if end == "file" else OK), bytes(out)
        c = (bits >> bp) & ((1 << width) - 1)
        bp += width
        if c == clear:
            table, width, prev, nxt = {}, mcs + 1, None, clear + 2
            continue
        if c == stop:
            break
        if prev is None:
            if c >= clear:
                return BAD_DATA, bytes(out)
            s = bytes([c])
        else:
            if c < clear:
                s = bytes([c])
            elif c < nxt:
                s = table[c]
            elif c == nxt and nxt < 4096:
                s = prev + prev[:1]
            else:
                return BAD_DATA, bytes(out)
            if nxt < 4096:
                table[nxt] = prev + s[:1]
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
        out += s
        prev = s
    return OK, bytes(out[:npix])


def decode(data, max_w=None, max_h=None):
    """The whole read -> (code, w, h, uint8 (h, w, 3) or None)."""
    d = bytes(data)
    code, F = parse(d)
    if code != OK:
        return code, 0, 0, None
    W, H = F["W"], F["H"]
    if (max_w is not None and W > max_w) or (max_h is not None and H > max_h):
        return TOO_LARGE, 0, 0, None
    gct, bg = F["gct"], F["bg"]
    canvas = np.zeros((H, W, 3), np.uint8)
    if gct is not None and bg < len(gct):
        canvas[:] = gct[bg]
    if not F["has_image"]:
        return OK, W, H, canvas
    fw, fh, fx, fy = F["fw"], F["fh"], F["fx"], F["fy"]
    stream, end = data_stream(d, F["data_at"])
    code, idx = lzw_decode(stream, end, F["mcs"], fw * fh)
    if code != OK:
        return code, 0, 0, None
    plane = np.frombuffer(idx + bytes([bg]) * (fw * fh - len(idx)), np.uint8).reshape(fh, fw)
    if F["interlace"]:
        t = np.empty_like(plane)
        t[interlace_order(fh)] = plane
        plane = t
    plane = plane[:H - fy, :W - fx]
    pal = np.zeros((256, 3), np.uint8)
    pal[:len(F["pal"])] = F["pal"]
    rgb = pal[plane]
    keep = np.ones(plane.shape, bool) if F["transparent"] is None else plane != F["transparent"]
    sub = canvas[fy:fy + plane.shape[0], fx:fx + plane.shape[1]]
    sub[keep] = rgb[keep]
    return OK, W, H, canvas


# ------------------------------------------------------------------------------------ corpus
def noise(seed, h, w, k):
    return np.random.default_rng(seed).integers(0, k, (h, w), dtype=np.uint8)


def base_file():
    """A ~200-byte file with a graphic control extension, a comment, a global and a local table."""
    idx = noise(7, 13, 15, 8)
    return (screen(17, 14, palette(8, 1), 2) + gce(True, 5) + extension(0xFE, b"hello") +
            descriptor(1, 1, 15, 13, lct=palette(8, 2), interlace=True) +
            image_data(lzw_codes(idx[interlace_order(13)], 3), 3, (40,)) + b";")


def status_cases():
    """(name, file, expected code): one or more per status."""
    pal = palette(4)
    good = simple_gif(noise(1, 4, 4, 4), pal)
    body = good[13 + 12:]
    out = [
        ("ok", good, OK),
        ("not_gif_signature", b"GIX" + good[3:], NOT_GIF),
        ("not_gif_version", b"GIF88a" + good[6:], NOT_GIF),
        ("not_gif_short", b"PNG\r\n\x1a", NOT_GIF),
        ("short_5", good[:5], BAD_HEADER),
        ("short_12", good[:12], BAD_HEADER),
        ("empty", b"", BAD_HEADER),
        ("zero_width", good[:6] + u16(0) + good[8:], BAD_HEADER),
        ("zero_height", good[:8] + u16(0) + good[10:], BAD_HEADER),
        ("bad_separator", good[:25] + b"\x00" + good[26:], MALFORMED),
        ("fx_at_width", screen(4, 4, pal) + descriptor(4, 0, 1, 1) + image_data([4, 0, 5], 2) + b";", MALFORMED),
        ("fy_at_height", screen(4, 4, pal) + descriptor(0, 4, 1, 1) + image_data([4, 0, 5], 2) + b";", MALFORMED),
        ("no_palette", screen(4, 4) + body, MALFORMED),
        ("code_size_1", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + b"\x01" + sub_blocks(b"\0\0") + b";", BAD_DATA),
        ("code_size_9", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + b"\x09" + sub_blocks(b"\0\0") + b";", BAD_DATA),
        ("code_above_next", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + image_data([4, 0, 7], 2) + b";", BAD_DATA),
        ("code_two_above_next", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + image_data([4, 0, 1, 2, 9], 2) + b";", BAD_DATA),
        ("first_code_not_literal", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + image_data([4, 6], 2) + b";", BAD_DATA),
        ("not_literal_after_second_clear", screen(4, 4, pal) + descriptor(0, 0, 4, 4) + image_data([4, 0, 1, 6, 4, 6], 2) + b";", BAD_DATA),
        ("cut_in_global_table", good[:20], TRUNCATED),
        ("cut_at_separator", good[:25], TRUNCATED),
        ("cut_in_descriptor", good[:30], TRUNCATED),
        ("cut_at_code_size", good[:35], TRUNCATED),
        ("cut_at_block_size", good[:36], TRUNCATED),
        ("cut_in_data", good[:39], TRUNCATED),
        ("cut_in_extension", screen(4, 4, pal) + gce(True, 1)[:5], TRUNCATED),
        ("cut_at_extension_label", screen(4, 4, pal) + b"!", TRUNCATED),
        ("cut_in_local_table", screen(4, 4, pal) + descriptor(0, 0, 4, 4, lct=pal)[:14], TRUNCATED),
    ]
    return out


def framed(W, H, idx, gct, fx=0, fy=0, lct=None, interlace=False, mcs=None, pre=b"", post=b";", bg=0, plan=(255,),
           fw=None, fh=None, version=b"89a", **kw):
    """A file whose frame (the index image `idx`, or fw x fh if given: the data then covers idx
    only) sits at (fx, fy) on a W x H canvas."""
    idx = np.asarray(idx, np.uint8)
    h, w = idx.shape
    if mcs is None:
        mcs = max(2, int(idx.max()).bit_length())
    rows = idx[interlace_order(h)] if interlace else idx
    return (screen(W, H, gct, bg, version) + pre + descriptor(fx, fy, fw or w, fh or h, lct, interlace) +
            image_data(lzw_codes(rows, mcs, **kw), mcs, plan) + post)


def mutants(base, count=200, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(base)
        p = int(rng.integers(0, len(b)))
        b[p] ^= 1 << int(rng.integers(0, 8))
        out.append((f"mutant{k}_at{p}", bytes(b)))
    return out


def corpus():
    """(name, file) for every shape of the read that fits a 300 x 289 canvas."""
    out = []
    for mcs in range(2, 9):
        for w in (1, 2, 3, 63, 64, 65, 257):
            out.append((f"mcs{mcs}_w{w}", simple_gif(noise(mcs * 100 + w, 5, w, 1 << mcs), palette(1 << mcs, mcs), mcs=mcs)))
    for h in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17):
        out.append((f"interlaced_h{h}", simple_gif(noise(h, h, 7, 16), palette(16, h), interlace=True)))
    # width steps and the full table
    p4 = palette(4, 9)
    out.append(("literal_fill_3_to_12", simple_gif(noise(11, 70, 70, 4), p4, use_table=False)))
    out.append(("greedy_fill", simple_gif(noise(12, 289, 289, 4), p4)))
    out.append(("noise8_fill", simple_gif(noise(13, 90, 100, 256), palette(256, 3))))
    out.append(("clear_at_full", simple_gif(noise(14, 100, 100, 4), p4, use_table=False, clear_at=lambda n, c: n == 4096)))
    out.append(("clear_after_width_step", simple_gif(noise(15, 60, 60, 4), p4, clear_at=lambda n, c: n in (8, 16, 64, 512))))
    codes = lzw_codes(noise(16, 8, 8, 4), 2)
    out.append(("consecutive_clears", screen(8, 8, p4) + descriptor(0, 0, 8, 8) +
                image_data([4, 4, 4] + codes[1:20] + [4, 4] + lzw_codes(noise(16, 8, 8, 4).reshape(-1)[_reached(codes[:20], 2):], 2)[1:], 2) + b";"))
    # stream start and end
    n16, p16 = noise(17, 20, 30, 16), palette(16, 4)
    out.append(("no_leading_clear", simple_gif(n16, p16, lead_clear=False)))
    codes = lzw_codes(n16, 4)
    out.append(("early_stop", screen(30, 20, p16, 3) + descriptor(0, 0, 30, 20) + image_data(codes[:len(codes) // 2] + [17], 4) + b";"))
    out.append(("terminator_without_stop", simple_gif(n16, p16, stop=False)))
    out.append(("terminator_mid_image", screen(30, 20, p16, 5) + descriptor(0, 0, 30, 20) + image_data(codes[:40], 4) + b";"))
    out.append(("bytes_after_stop", screen(30, 20, p16) + descriptor(0, 0, 30, 20) + bytes([4]) +
                sub_blocks(pack_codes(codes, 4) + bytes(range(200, 240))) + b";"))
    out.append(("string_across_frame_end", framed(9, 6, np.full((5, 8), 2, np.uint8), p4, fw=7, fh=5)))
    out.append(("kwkwk_across_frame_end", framed(9, 6, np.full((1, 40), 1, np.uint8), p4, fw=3, fh=9)))
    # KwKwK and long strings
    out.append(("flat_300x70", simple_gif(np.full((70, 300), 3, np.uint8), p4)))
    for per in (2, 3, 63, 64, 65):
        out.append((f"period{per}", simple_gif((np.arange(40 * 200) % per % 64).reshape(40, 200).astype(np.uint8), palette(64, per))))
    # sub-block plans
    rng = np.random.default_rng(21)
    n8 = noise(18, 24, 40, 8)
    for name, plan in (("all_1", (1,)), ("3_2_1", (3, 2, 1)), ("random", tuple(int(v) for v in rng.integers(1, 256, 64))),
                       ("254_1", (254, 1))):
        out.append((f"plan_{name}", simple_gif(n8, palette(8, 5), plan=plan)))
    # container and palette
    g8, l8 = palette(8, 6), palette(8, 7)
    out.append(("local_over_global", framed(40, 24, n8, g8, lct=l8)))
    for k in (2, 4, 8, 16, 32, 64, 128, 256):
        out.append((f"table_{k}", simple_gif(noise(k, 6, 33, k), palette(k, k))))
    out.append(("index_beyond_table", framed(40, 24, n8, palette(4, 8), mcs=3)))
    out.append(("index_beyond_local_table", framed(40, 24, n8, g8, lct=palette(2, 8), mcs=3)))
    out.append(("no_global_table", framed(44, 30, n8, None, 2, 3, lct=l8, bg=1)))
    out.append(("bg_beyond_table", framed(44, 30, n8, palette(4, 2), 2, 3, lct=l8, bg=9)))
    out.append(("sub_rectangle", framed(50, 31, n8, g8, 7, 5, bg=3)))
    out.append(("sub_rectangle_interlaced", framed(50, 31, n8, g8, 7, 5, bg=3, interlace=True)))
    out.append(("clipped", framed(30, 20, n8, g8, 5, 3, bg=1)))
    out.append(("clipped_interlaced", framed(30, 20, n8, g8, 5, 3, bg=1, interlace=True)))
    out.append(("clipped_one_pixel", framed(30, 20, n8, g8, 29, 19, bg=1)))
    out.append(("transparent_on", framed(50, 31, n8, g8, 7, 5, bg=3, pre=gce(True, 2))))
    out.append(("transparent_off", framed(50, 31, n8, g8, 7, 5, bg=3, pre=gce(False, 2))))
    out.append(("transparent_is_bg_unreached", screen(30, 20, p16, 5) + gce(True, 5) + descriptor(0, 0, 30, 20) + image_data(codes[:40], 4) + b";"))
    out.append(("two_gce_last_on", framed(50, 31, n8, g8, 7, 5, pre=gce(False, 1) + gce(True, 4))))
    out.append(("two_gce_last_off", framed(50, 31, n8, g8, 7, 5, pre=gce(True, 1) + gce(False, 4))))
    out.append(("gce_short_block", framed(50, 31, n8, g8, 7, 5, pre=extension(0xF9, b"\x01\0\0"))))
    out.append(("gce_long_block", framed(50, 31, n8, g8, 7, 5, pre=extension(0xF9, b"\x01\0\0\x03\x07\x07", b"\x01\0\0\x05"))))
    ext = (extension(0xFE, b"a comment", b"x" * 255) + extension(0xFF, b"NETSCAPE2.0", b"\x01\0\0") +
           extension(0x01, bytes(12), b"plain text") + extension(0x77, b"unknown", b"\x01") + extension(0xFE))
    out.append(("extensions", framed(40, 24, n8, g8, pre=ext)))
    second = gce(True, 0) + descriptor(0, 0, 40, 24) + image_data(lzw_codes(noise(19, 24, 40, 8), 3), 3)
    out.append(("second_frame", framed(40, 24, n8, g8, post=second + b";")))
    out.append(("second_frame_broken", framed(40, 24, n8, g8, post=b",\x01\x02")))
    out.append(("no_trailer", framed(40, 24, n8, g8, post=b"")))
    out.append(("trailer_first", screen(17, 9, g8, 6) + b";"))
    out.append(("trailer_first_no_table", screen(17, 9) + extension(0xFE, b"none") + b";"))
    out.append(("gif87a", framed(40, 24, n8, g8, version=b"87a")))
    out.append(("zero_width_frame", screen(12, 7, g8, 4) + descriptor(1, 1, 0, 5) + bytes([3]) + b";"))
    return out


def _reached(codes, mcs):
    """Pixels a reader has produced after `codes`."""
    return len(lzw_decode(pack_codes(codes, mcs) + b"\0\0", "term", mcs, 1 << 30)[1])
