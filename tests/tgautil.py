"""Targa test corpus shared by the CPU tests (tests/test_tga_core.py) and the GPU parity tests
(tests/test_gpu_tga.py). numpy only; everything is seeded.

* `tga_file` builds files of every accepted type and depth: raw, or run-length coded with a chosen
  packet plan (greedy per row, greedy across row ends, literal or run packets of a fixed length),
  with an ID field, a colour-map origin, descriptor bits and the TGA 2.0 footer.
* `decode` is an independent serial statement of the read contract in include/icx.h (header
  codes, the first-failing-packet rule, palette origin, row order), written packet by packet.
* `greedy_row` / `encode` state the write: the 18 header bytes, B,G,R(,A), the greedy row packer.
"""
import numpy as np

OK, BAD_HEADER, UNSUPPORTED, NO_IMAGE, MALFORMED, TRUNCATED, TOO_LARGE, INVALID_ARGUMENT = range(8)
FOOTER = b"\0" * 8 + b"TRUEVISION-XFILE.\0"
FIXTURE_SHA256 = "197f6b862531f4b81f313584cae00ba3ab2cdafe8ddccefb67ead15189d38b78"


# ------------------------------------------------------------------------------------ pixels
def synth(seed: int, w: int, h: int, d: int, levels: int = 5) -> np.ndarray:
    """(h, w, d) pixels with real runs: stretches of 1..12 equal pixels from a few colours, some
    stretches replaced by noise."""
    rng = np.random.default_rng(seed)
    colours = rng.integers(0, 256, (levels, d), dtype=np.uint8)
    flat = np.empty((w * h, d), np.uint8)
    i = 0
    while i < w * h:
        r = int(rng.integers(1, 13))
        if rng.random() < 0.3:
            flat[i:i + r] = rng.integers(0, 256, (min(r, w * h - i), d), dtype=np.uint8)
        else:
            flat[i:i + r] = colours[rng.integers(0, levels)]
        i += r
    return flat.reshape(h, w, d)


def to_file_order(px: np.ndarray) -> np.ndarray:
    """R,G,B(,A) -> the file's B,G,R(,A)."""
    if px.shape[-1] == 1:
        return px
    out = px.copy()
    out[..., 0], out[..., 2] = px[..., 2], px[..., 0]
    return out


# ------------------------------------------------------------------------------------ packers
def pack_greedy(elems: np.ndarray) -> bytes:
    """The greedy rule of include/icx.h over one sequence of elements (n, bytes per element)."""
    n = len(elems)
    same = np.zeros(n, bool)  # same[k]: element k equals element k + 1
    if n > 1:
        same[:-1] = (elems[:-1] == elems[1:]).all(axis=1)
    out = bytearray()
    i = 0
    while i < n:
        r = 1
        while r < 128 and i + r < n and same[i + r - 1]:
            r += 1
        if r >= 2:
            out.append(0x80 | (r - 1))
            out += elems[i].tobytes()
            i += r
        else:
            k = i
            while k < n and k - i < 128 and not same[k]:
                k += 1
            out.append(k - i - 1)
            out += elems[i:k].tobytes()
            i = k
    return bytes(out)


def pack_fixed(elems: np.ndarray, length: int, run: bool) -> bytes:
    """Packets of `length` elements (the last one shorter): literal, or run packets that repeat
    each packet's first element (a decode then differs from `elems` unless they are equal)."""
    out = bytearray()
    for i in range(0, len(elems), length):
        c = min(length, len(elems) - i)
        if run:
            out.append(0x80 | (c - 1))
            out += elems[i].tobytes()
        else:
            out.append(c - 1)
            out += elems[i:i + c].tobytes()
    return bytes(out)


def greedy_row(row: np.ndarray) -> bytes:
    """One row (w, d) of R,G,B(,A) pixels -> its packets (the write's rule)."""
    return pack_greedy(to_file_order(row))


# ------------------------------------------------------------------------------------ builder
def header(typ, w, h, bits, desc=0, idlen=0, cmt=0, origin=0, mlen=0, mes=0) -> bytes:
    return bytes([idlen, cmt, typ, origin & 255, origin >> 8, mlen & 255, mlen >> 8, mes, 0, 0, 0, 0,
                  w & 255, w >> 8, h & 255, h >> 8, bits, desc])


def tga_file(px=None, *, rle=False, topdown=False, idlen=0, footer=False, plan="rows", desc=0,
             indices=None, palette=None, idx_bits=8, origin=0) -> bytes:
    """px: (h, w, d) R,G,B(,A) / grey pixels, rows top-down; or `indices` (h, w) into `palette`
    (n, d) R,G,B(,A) with the first map entry standing for index `origin`.
    plan: "rows" greedy per row, "cross" greedy over the whole image (packets cross row ends),
    ("lit", n) / ("run", n) packets of n elements."""
    if indices is not None:
        h, w = indices.shape
        d = palette.shape[1]
        bpp = idx_bits // 8
        rows = np.zeros((h, w, bpp), np.uint8)
        rows[..., 0] = indices & 255
        if bpp == 2:
            rows[..., 1] = indices >> 8
        typ, bits = 1, idx_bits
        cmap = to_file_order(palette).tobytes()
        hd = dict(cmt=1, origin=origin, mlen=len(palette), mes=8 * d)
    else:
        h, w, d = px.shape
        rows = to_file_order(px)
        bpp = d
        typ, bits = (3 if d == 1 else 2), 8 * d
        cmap = b""
        hd = {}
    if not topdown:
        rows = rows[::-1]
    rows = np.ascontiguousarray(rows)
    if not rle:
        body = rows.tobytes()
    elif plan == "rows":
        body = b"".join(pack_greedy(r) for r in rows)
    elif plan == "cross":
        body = pack_greedy(rows.reshape(-1, bpp))
    else:
        body = pack_fixed(rows.reshape(-1, bpp), plan[1], plan[0] == "run")
    ident = bytes((37 * k + 1) & 255 for k in range(idlen))
    return (header(typ + (8 if rle else 0), w, h, bits, desc | (0x20 if topdown else 0), idlen, **hd) + ident + cmap +
            body + (FOOTER if footer else b""))


# ------------------------------------------------------------------------------------ the read, restated
def decode(data: bytes):
    """-> (code, w, h, d, (h, w, d) uint8 or None)."""
    fail = lambda c: (c, 0, 0, 0, None)
    n = len(data)
    if n < 18:
        return fail(BAD_HEADER)
    u16 = lambda o: data[o] | data[o + 1] << 8
    idlen, cmt, typ, origin, mlen, mes = data[0], data[1], data[2], u16(3), u16(5), data[7]
    w, h, bits, desc = u16(12), u16(14), data[16], data[17]
    if cmt > 1 or typ not in (0, 1, 2, 3, 9, 10, 11) or w == 0 or h == 0:
        return fail(BAD_HEADER)
    pal = typ in (1, 9)
    if pal and (cmt == 0 or mlen == 0):
        return fail(BAD_HEADER)
    if typ == 0:
        return fail(NO_IMAGE)
    if desc & 0x10:
        return fail(UNSUPPORTED)
    if pal:
        if bits not in (8, 16) or mes not in (24, 32):
            return fail(UNSUPPORTED)
        d = mes // 8
    elif typ in (2, 10):
        if bits not in (24, 32):
            return fail(UNSUPPORTED)
        d = bits // 8
    else:
        if bits != 8:
            return fail(UNSUPPORTED)
        d = 1
    bpp = bits // 8
    map_at = 18 + idlen
    ds = map_at + (mlen * ((mes + 7) // 8) if cmt else 0)
    if ds > n:
        return fail(TRUNCATED)
    npix = w * h
    buf = np.frombuffer(data, np.uint8)
    if typ < 9:
        if ds + npix * bpp > n:
            return fail(TRUNCATED)
        elems = buf[ds:ds + npix * bpp].reshape(npix, bpp)
    else:
        elems = np.zeros((npix, bpp), np.uint8)
        pos, p = ds, 0
        while p < npix:
            if pos >= n:
                return fail(TRUNCATED)
            count = (data[pos] & 127) + 1
            size = bpp if data[pos] & 128 else count * bpp
            if pos + 1 + size > n:
                return fail(TRUNCATED)
            if count > npix - p:
                return fail(MALFORMED)
            elems[p:p + count] = buf[pos + 1:pos + 1 + size].reshape(-1, bpp)
            p += count
            pos += 1 + size
    if pal:
        idx = elems[:, 0].astype(np.int64) + (elems[:, 1].astype(np.int64) << 8 if bpp == 2 else 0) - origin
        table = buf[map_at:map_at + mlen * d].reshape(mlen, d)
        inside = (idx >= 0) & (idx < mlen)
        colours = np.zeros((npix, d), np.uint8)
        colours[inside] = table[idx[inside]]
    else:
        colours = elems
    out = to_file_order(colours.reshape(h, w, d))  # the exchange is its own inverse
    if not desc & 0x20:
        out = out[::-1]
    return OK, w, h, d, np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------ the write, restated
def encode(px: np.ndarray, rle: bool) -> bytes:
    h, w, d = px.shape
    head = bytes([0, 0, (3 if d == 1 else 2) + (8 if rle else 0), 0, 0, 0, 0, 0, 0, 0, 0, 0,
                  w % 256, w // 256, h % 256, h // 256, d * 8, 0x20])
    if not rle:
        return head + to_file_order(px).tobytes()
    return head + b"".join(greedy_row(r) for r in px)


def encode_bound(w, h, d):
    return 18 + w * h * (d + 1)


# ------------------------------------------------------------------------------------ corpus
def _paletted(seed, w, h, d, n, idx_bits, origin, stray=False):
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, (n, d), dtype=np.uint8)
    base = synth(seed + 1, w, h, 1, levels=4)[..., 0].astype(np.int64)
    indices = origin + base % n
    if stray:  # indices below the origin and past the map's end
        indices[0, 0] = origin + n
        indices[-1, -1] = max(0, origin - 1)
        indices[h // 2, w // 2] = origin + n + 7
    return indices, palette


def valid_cases():
    """(name, file bytes, expected (h, w, d) pixels): every type x depth, both origins, ID field,
    map origin, 16-bit indices, indices outside the map."""
    out = []
    k = 0
    for rle in (False, True):
        for d in (1, 3, 4):
            for topdown in (False, True):
                k += 1
                px = synth(100 + k, 37, 11, d)
                name = f"{'rle' if rle else 'raw'}_d{d}_{'top' if topdown else 'bot'}"
                out.append((name, tga_file(px, rle=rle, topdown=topdown, idlen=5 * (k % 3), footer=bool(k & 1)), px))
        for d in (3, 4):
            for idx_bits, n, origin in ((8, 200, 0), (8, 40, 17), (16, 300, 0), (16, 700, 1000)):
                for stray in (False, True):
                    k += 1
                    ind, pal = _paletted(200 + k, 29, 13, d, n, idx_bits, origin, stray)
                    f = tga_file(indices=ind, palette=pal, idx_bits=idx_bits, origin=origin, rle=rle,
                                 topdown=bool(k & 1), idlen=k % 4, footer=stray)
                    name = f"{'rle' if rle else 'raw'}_pal{d}_i{idx_bits}_o{origin}{'_stray' if stray else ''}"
                    out.append((name, f, decode(f)[4]))
    px = synth(31, 40, 9, 3)
    out.append(("truecolour_with_unused_map", header(2, 40, 9, 24, cmt=1, mlen=4, mes=24) + b"\1" * 12 +
                to_file_order(px[::-1]).tobytes(), px))
    return out


def rle_shape_cases():
    """(name, file bytes): the run-length shapes that can go wrong. Every file decodes OK."""
    out = []
    for w in (1, 2, 127, 128, 129, 257):
        for d in (1, 3, 4):
            px = synth(300 + w + d, w, 5, d)
            out.append((f"w{w}_d{d}_rows", tga_file(px, rle=True)))
            out.append((f"w{w}_d{d}_cross", tga_file(px, rle=True, plan="cross", topdown=True)))
    one = np.full((1, 128, 3), 9, np.uint8)
    out.append(("one_128_run", tga_file(one, rle=True)))
    noise = np.random.default_rng(5).integers(0, 256, (1, 128, 4), dtype=np.uint8)
    out.append(("one_128_literal", tga_file(noise, rle=True, plan=("lit", 128))))
    alt = np.zeros((6, 131, 3), np.uint8)
    alt.reshape(-1, 3)[1::2] = (255, 1, 2)
    out.append(("alternating", tga_file(alt, rle=True)))
    out.append(("alternating_cross", tga_file(alt, rle=True, plan="cross")))
    out.append(("all_equal", tga_file(np.full((9, 300, 4), 77, np.uint8), rle=True, plan="cross")))
    out.append(("all_equal_mono_rows", tga_file(np.full((40, 70, 1), 3, np.uint8), rle=True)))
    out.append(("runs_of_one", tga_file(synth(8, 33, 7, 3), rle=True, plan=("run", 1))))
    out.append(("literals_of_three", tga_file(synth(9, 50, 7, 1), rle=True, plan=("lit", 3))))
    return out


def tiled_case(tile: int, ntiles: int = 3):
    """A file whose packet stream spans at least `ntiles` tiles of `tile` bytes with a packet
    lying across every tile boundary -> (file bytes, the boundaries' packets as (start, end))."""
    w, h = 256, 2
    while True:
        px = synth(77, w, h, 4, levels=3)
        f = tga_file(px, rle=True, plan="cross", topdown=True)
        if len(f) - 18 >= ntiles * tile + 64:
            break
        h *= 2
    for seed in range(77, 177):  # the first seed whose stream has a packet across every boundary
        px = synth(seed, w, h, 4, levels=3)
        f = tga_file(px, rle=True, plan="cross", topdown=True)
        pos, straddle = 18, []
        npix, p = w * h, 0
        while p < npix:
            c = (f[pos] & 127) + 1
            nxt = pos + 1 + (4 if f[pos] & 128 else 4 * c)
            for b in range(1, (len(f) - 18) // tile + 1):
                if pos - 18 < b * tile < nxt - 18:
                    straddle.append((pos - 18, nxt - 18))
            p += c
            pos = nxt
        if len(straddle) == (pos - 18 - 1) // tile >= ntiles:
            return f, straddle
    raise AssertionError("no seed gives a packet across every tile boundary")


def header_cases():
    """(name, file bytes, code): crafted headers for every code the header walk gives."""
    body = b"\0" * 64
    H = header
    out = [
        ("short_17", H(2, 4, 4, 24)[:17], BAD_HEADER),
        ("empty", b"", BAD_HEADER),
        ("zero_width", H(2, 0, 4, 24) + body, BAD_HEADER),
        ("zero_height", H(10, 4, 0, 24) + body, BAD_HEADER),
        ("cmap_type_2", H(2, 4, 4, 24, cmt=2) + body, BAD_HEADER),
        ("paletted_no_map_type", H(1, 4, 4, 8, cmt=0, mlen=4, mes=24) + body, BAD_HEADER),
        ("paletted_empty_map", H(9, 4, 4, 8, cmt=1, mlen=0, mes=24) + body, BAD_HEADER),
        ("type_4", H(4, 4, 4, 24) + body, BAD_HEADER),
        ("type_8", H(8, 4, 4, 24) + body, BAD_HEADER),
        ("type_12", H(12, 4, 4, 24) + body, BAD_HEADER),
        ("type_32", H(32, 4, 4, 24) + body, BAD_HEADER),
        ("type_0", H(0, 4, 4, 24) + body, NO_IMAGE),
        ("type_0_zero_size", H(0, 0, 0, 0), BAD_HEADER),
        ("colour_15", H(2, 4, 4, 15) + body, UNSUPPORTED),
        ("colour_16", H(10, 4, 4, 16) + body, UNSUPPORTED),
        ("colour_8", H(2, 4, 4, 8) + body, UNSUPPORTED),
        ("mono_16", H(3, 4, 4, 16) + body, UNSUPPORTED),
        ("mono_24", H(11, 4, 4, 24) + body, UNSUPPORTED),
        ("map_entry_15", H(1, 4, 4, 8, cmt=1, mlen=4, mes=15) + body, UNSUPPORTED),
        ("map_entry_16", H(9, 4, 4, 8, cmt=1, mlen=4, mes=16) + body, UNSUPPORTED),
        ("index_24", H(1, 4, 4, 24, cmt=1, mlen=4, mes=24) + body, UNSUPPORTED),
        ("right_to_left", H(2, 4, 4, 24, desc=0x10) + body, UNSUPPORTED),
        ("right_to_left_top", H(10, 4, 4, 32, desc=0x38) + body, UNSUPPORTED),
        ("raw_short", H(2, 4, 4, 24) + body[:47], TRUNCATED),
        ("raw_exact", H(2, 4, 4, 24) + body[:48], OK),
        ("map_past_file", H(1, 4, 4, 8, cmt=1, mlen=30, mes=24) + body, TRUNCATED),
        ("id_past_file", H(10, 4, 4, 24, idlen=200) + body, TRUNCATED),
        ("rle_header_only", H(10, 4, 4, 24), OK),  # the packets are the decode's to judge
    ]
    return out


def edge_cases():
    """(name, file bytes): failures and fuzz; the expected result is `decode`'s."""
    out = [(n, f) for n, f, _ in header_cases()]
    px = synth(41, 23, 9, 3)
    good = tga_file(px, rle=True, plan="cross")
    # the last packet of the stream, found by a walk
    pos, p, last = 18, 0, 18
    while p < 23 * 9:
        last = pos
        c = (good[pos] & 127) + 1
        pos += 1 + (3 if good[pos] & 128 else 3 * c)
        p += c
    end = pos
    over = bytearray(good)
    over[last] = (over[last] & 128) | min(127, (over[last] & 127) + 1)
    if not over[last] & 128:
        over += b"\0\0\0"
    out.append(("overshoot_last_packet", bytes(over)))
    flat = np.full((4, 40, 4), 200, np.uint8)
    out.append(("overshoot_run_128", tga_file(flat, rle=True, plan="cross")[:18] + bytes([0x80 | 127, 1, 2, 3, 4]) * 2))
    out.append(("cut_at_header_byte", good[:last]))
    out.append(("cut_at_first_header_byte", good[:18]))
    runs = tga_file(np.full((3, 50, 3), 5, np.uint8), rle=True)
    out.append(("cut_in_run_pixel", runs[:18 + 2]))
    out.append(("cut_in_last_run_pixel", runs[:-1]))
    lits = tga_file(np.random.default_rng(3).integers(0, 256, (4, 30, 4), dtype=np.uint8), rle=True, plan=("lit", 128))
    out.append(("cut_in_literal_payload", lits[:18 + 1 + 4 * 50 + 2]))
    out.append(("cut_in_last_literal", lits[:-1]))
    out.append(("exact_end", good[:end]))
    ind, pal = _paletted(50, 16, 6, 3, 60, 8, 0)
    palf = tga_file(indices=ind, palette=pal, rle=True)
    out.append(("cut_in_colour_map", palf[:18 + 100]))
    out.append(("cut_after_colour_map", palf[:18 + 180]))
    out.append(("mono_overshoot", header(11, 10, 1, 8) + bytes([0x80 | 10, 7])))
    out.append(("mono_run_then_missing", header(11, 10, 2, 8) + bytes([0x80 | 9, 7])))
    rng = np.random.default_rng(2024)
    for name, src in (("fuzz_rle", good), ("fuzz_pal", palf)):
        for k in range(24):
            b = bytearray(src)
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, len(b)))
                b[at] ^= 1 << int(rng.integers(0, 8))
            out.append((f"{name}_{k}", bytes(b)))
    return out
