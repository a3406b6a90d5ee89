"""The GIF write's contract (include/icx.h, "GIF write") restated in Python, independently of the
C++ core and the kernels: numpy for the palette, a dictionary of tuples for LZW, gifutil's
pack_codes / sub_blocks / screen / descriptor (the reader's side) for bits and container. Also the
images the write's tests share, and PIL as a second reader."""
import io

import numpy as np

import gifutil as G

OK, TOO_LARGE, INVALID_ARGUMENT = 0, 6, 7
AUTO, CUBE = 0, 1
DEFAULT_SEG = 65536
B4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])


# ------------------------------------------------------------------------------------ arguments
def segments(n_pixels, segment_pixels):
    """-> pixels per segment, or None for a refused value."""
    if segment_pixels == 0:
        seg = DEFAULT_SEG
    elif segment_pixels == -1:
        seg = n_pixels
    elif segment_pixels >= 64:
        seg = segment_pixels
    else:
        return None
    return min(seg, n_pixels)


def accepted(w, h, d=1, segment_pixels=0, dither=0, mode=AUTO):
    return (d in (1, 3, 4) and 1 <= w <= 65535 and 1 <= h <= 65535 and w * h <= 1 << 30 and dither in (0, 1) and
            mode in (AUTO, CUBE) and (segment_pixels in (0, -1) or segment_pixels >= 64))


def bound(w, h, segment_pixels=0):
    if not accepted(w, h, 1, segment_pixels):
        return 0
    n = w * h
    seg = segments(n, segment_pixels)
    codes = n + -(-n // seg) + 1 + n // 3838
    p = -(-12 * codes // 8)
    return 13 + 768 + 10 + 1 + p + -(-p // 255) + 2


# ------------------------------------------------------------------------------------ palette
def rgb_of(a):
    """uint8 (h, w) or (h, w, d), d in 1, 3, 4 -> (h, w, 3)."""
    a = np.asarray(a, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a[:, :, :3]


def level_values(L):
    return [(255 * k + (L - 1) // 2) // (L - 1) for k in range(L)]


def cube_table():
    t = np.zeros((256, 3), np.uint8)
    r, g, b = level_values(6), level_values(7), level_values(6)
    for i in range(252):
        t[i] = (r[i // 42], g[(i // 6) % 7], b[i % 6])
    return t


def quantise(a, dither=0, mode=AUTO):
    """-> (index plane (h, w) uint8, table (2^tb, 3) uint8, tb, m)."""
    rgb = rgb_of(a).astype(np.int64)
    h, w = rgb.shape[:2]
    keys = rgb[:, :, 0] << 16 | rgb[:, :, 1] << 8 | rgb[:, :, 2]
    uniq = np.unique(keys)
    if mode == AUTO and len(uniq) <= 256:
        n = len(uniq)
        tb = max(1, (n - 1).bit_length())
        table = np.zeros((1 << tb, 3), np.uint8)
        table[:n] = np.stack([uniq >> 16, (uniq >> 8) & 255, uniq & 255], axis=1)
        return np.searchsorted(uniq, keys).astype(np.uint8), table, tb, max(2, tb)
    if dither:
        T = 2 * B4[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3] + 1
    else:
        T = np.full((h, w), 16)
    k = [(32 * rgb[:, :, c] * (L - 1) + 255 * T) // 8160 for c, L in enumerate((6, 7, 6))]
    return ((k[0] * 7 + k[1]) * 6 + k[2]).astype(np.uint8), cube_table(), 8, 8


# ------------------------------------------------------------------------------------ code stream
def segment_codes(idx, m, first, last):
    """One segment's codes: greedy longest match over a dictionary of tuples, a Clear after the
    code that adds entry 4095, the pending code, then a Clear or (last) the stop code; the first
    segment carries the stream's leading Clear."""
    clear = 1 << m
    codes = [clear] if first else []
    table, nxt = {}, clear + 2
    w = None
    for k in (int(v) for v in idx):
        if w is None:
            w = k
            continue
        if (w, k) in table:
            w = table[(w, k)]
            continue
        codes.append(w)
        table[(w, k)] = nxt
        nxt += 1
        if nxt == 4096:
            codes.append(clear)
            table, nxt = {}, clear + 2
        w = k
    codes.append(w)
    codes.append(clear + 1 if last else clear)
    return codes


def code_widths(codes, m):
    """The width the reader holds at each code (the rule of gifutil.pack_codes, restated)."""
    clear, stop = 1 << m, (1 << m) + 1
    width, nxt, prev = m + 1, clear + 2, False
    out = []
    for c in codes:
        out.append(width)
        if c == clear:
            width, nxt, prev = m + 1, clear + 2, False
        elif c != stop:
            if prev and nxt < 4096:
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
            prev = True
    return out


def stream(plane, m, segment_pixels=0):
    """-> (all codes, the bit offset of each segment's string: the first one's holds the leading Clear)."""
    idx = np.asarray(plane, np.uint8).reshape(-1)
    seg = segments(len(idx), segment_pixels)
    assert seg is not None
    codes, offs, bits = [], [], 0
    nseg = -(-len(idx) // seg)
    for s in range(nseg):
        c = segment_codes(idx[s * seg:(s + 1) * seg], m, s == 0, s == nseg - 1)
        offs.append(bits)
        bits += sum(code_widths(c, m))  # (a segment's widths depend on its own codes only)
        codes += c
    assert sum(code_widths(codes, m)) == bits
    return codes, offs


def write_gif(a, segment_pixels=0, dither=0, mode=AUTO):
    """The contract's file for the pixels a."""
    a = np.asarray(a, np.uint8)
    h, w = a.shape[:2]
    assert accepted(w, h, 1 if a.ndim == 2 else a.shape[2], segment_pixels, dither, mode)
    plane, table, tb, m = quantise(a, dither, mode)
    codes, _ = stream(plane, m, segment_pixels)
    scr = G.screen(w, h, table)
    flags = 0x80 | (tb - 1) << 4 | (tb - 1)
    scr = scr[:10] + bytes([flags]) + scr[11:]
    return scr + G.descriptor(0, 0, w, h) + bytes([m]) + G.sub_blocks(G.pack_codes(codes, m)) + b";"


def payload_size(a, segment_pixels=0, dither=0, mode=AUTO):
    plane, _, _, m = quantise(a, dither, mode)
    return len(G.pack_codes(stream(plane, m, segment_pixels)[0], m))


def segment_offsets(a, segment_pixels=0, dither=0, mode=AUTO):
    plane, _, _, m = quantise(a, dither, mode)
    return stream(plane, m, segment_pixels)[1]


def expected_pixels(a, dither=0, mode=AUTO):
    """What a reader gives back: the table's colours at the indices."""
    plane, table, _, _ = quantise(a, dither, mode)
    return table[plane]


def full_clear_positions(plane, m):
    """Pixel positions p (in a one-segment stream) whose mismatch filled the table: the Clear is
    written while pixel p is pending."""
    clear = 1 << m
    table, nxt, w, out = {}, clear + 2, None, []
    for p, k in enumerate(int(v) for v in np.asarray(plane).reshape(-1)):
        if w is None:
            w = k
        elif (w, k) in table:
            w = table[(w, k)]
        else:
            table[(w, k)] = nxt
            nxt += 1
            if nxt == 4096:
                out.append(p)
                table, nxt = {}, clear + 2
            w = k
    return out


# ------------------------------------------------------------------------------------ readers
def pil_pixels(f):
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    return np.asarray(im.convert("RGB"))


def reads_back(f, a, dither=0, mode=AUTO, name="", pil=True):
    exp = expected_pixels(a, dither, mode)
    code, w, h, px = G.decode(f)
    assert (code, w, h) == (G.OK, exp.shape[1], exp.shape[0]), (name, code)
    np.testing.assert_array_equal(px, exp, err_msg=str(name))
    if pil:
        np.testing.assert_array_equal(pil_pixels(f), exp, err_msg="PIL " + str(name))


# ------------------------------------------------------------------------------------ images
def colours(n, seed=0):
    """n distinct colours, in no particular order."""
    rng = np.random.default_rng(500 + seed)
    keys = rng.choice(1 << 24, n, replace=False)
    return np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)


def image(seed, h, w, d, n, kind="noise"):
    """(h, w, d) uint8 with min(n, h*w) distinct colours (d = 1: grey levels): noise, flat (one
    colour but for the first pixels, which carry the others) or smooth (index ramps)."""
    rng = np.random.default_rng(seed)
    N = h * w
    n = min(n, N, 256 if d == 1 else 1 << 24)
    if kind == "noise":
        idx = rng.integers(0, n, N)
    elif kind == "flat":
        idx = np.zeros(N, np.int64)
    else:
        idx = (np.arange(N) % w * n // max(w, 1) + np.arange(N) // w) % n
    idx[rng.permutation(N)[:n]] = np.arange(n)  # every colour is met
    if d == 1:
        pal = rng.permutation(256)[:n].astype(np.uint8)[:, None]
    else:
        pal = colours(n, seed)
        if d == 4:
            pal = np.concatenate([pal, rng.integers(0, 256, (n, 1), dtype=np.uint8)], axis=1)
    return pal[idx].reshape(h, w, d)


def many_colours(seed, h, w, d=3, smooth=False):
    """More than 256 colours where the size allows it (the cube's input)."""
    rng = np.random.default_rng(seed)
    if smooth:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 3) % 256] + ([x * 0 + 7] if d == 4 else []), axis=2)
        return a.astype(np.uint8)
    return rng.integers(0, 256, (h, w, d), dtype=np.uint8)


NCOL = (1, 2, 3, 4, 5, 16, 17, 128, 129, 255, 256, 257)
SEGS = (64, 65, 255, 4096, 0, -1)


def size_grid():
    """(w, h) of the GPU grid's sizes."""
    out = [(w, h) for w in range(1, 22) for h in range(1, 10)]
    out += [(w, h) for w in list(range(253, 260)) + list(range(509, 516)) for h in (1, 2, 3)]
    return out


def grid_cases():
    """(name, pixels, segment_pixels, dither, mode) over sizes x colours x d x content: each size
    with one d / colour count / content / segment size in turn, so that every pair of values is met
    many times without the product's cost."""
    out = []
    kinds = ("noise", "flat", "smooth")
    for i, (w, h) in enumerate(size_grid()):
        d = (1, 3, 4)[i % 3]
        n = NCOL[(i // 3) % len(NCOL)]
        kind = kinds[(i // 2) % 3]
        seg = SEGS[(i // 5) % len(SEGS)]
        if n == 257 and d == 1:
            n = 256
        if n == 257:
            a = many_colours(i, h, w, d, smooth=kind == "smooth")
            out.append((f"{w}x{h}_d{d}_many_dither{i & 1}_seg{seg}", a, seg, i & 1, AUTO))
        else:
            out.append((f"{w}x{h}_d{d}_n{n}_{kind}_seg{seg}", image(i, h, w, d, n, kind), seg, 0, AUTO))
    # every colour count with every d at sizes that hold it, the cube both ways, the forced cube
    for d in (1, 3, 4):
        for n in NCOL:
            for kind in kinds:
                w, h = (21, 9) if n <= 129 else (259, 3)
                if n == 257 and d == 1:
                    continue  # (grey has no more than 256)
                if n == 257:
                    a = many_colours(n + d, h, w, d, smooth=kind == "smooth")
                    for dither in (0, 1):
                        out.append((f"many_d{d}_{kind}_dither{dither}", a, 64, dither, AUTO))
                else:
                    out.append((f"n{n}_d{d}_{kind}", image(n * 7 + d, h, w, d, n, kind), 65, 0, AUTO))
        for dither in (0, 1):
            out.append((f"forced_cube_d{d}_dither{dither}", image(77 + d, 9, 21, d, 3, "noise"), 64, dither, CUBE))
    return out


def shape_for(N):
    """(h, w) with h * w = N and both sides in 1..65535, the widest such w."""
    for w in range(min(N, 65535), 0, -1):
        if N % w == 0 and N // w <= 65535:
            return N // w, w
    raise AssertionError(N)


def segment_end_cases():
    """N = k * seg and k * seg + 1 (a one-pixel last segment) for every segment size, noise and
    flat; flat at m = 2 and seg = 64 gives the shortest segment bit strings. The default size is met
    at k = 2 (65537 is prime, so no image has that many pixels); -1 is one segment whatever N."""
    out = []
    for seg in SEGS:
        for k in ((2,) if seg == 0 else (1,) if seg == -1 else (1, 2, 3)):
            for extra in (0, 1):
                N = {0: DEFAULT_SEG, -1: 300}.get(seg, seg) * k + extra
                h, w = shape_for(N)
                for kind, n in (("noise", 16), ("flat", 4), ("flat", 1)):
                    out.append((f"seg{seg}_k{k}+{extra}_{kind}{n}", image(seg + k + extra, h, w, 1, n, kind), seg, 0, AUTO))
    return out


def row_cases(m, nmax=600):
    """The 1 x N images N = 1 .. nmax of noise over 2^m colours (m = 2: four)."""
    n = 1 << m
    rng = np.random.default_rng(900 + m)
    pal = np.sort(rng.permutation(256)[:n]).astype(np.uint8)
    out = []
    for N in range(1, nmax + 1):
        idx = rng.integers(0, n, N)
        if N >= n:
            idx[rng.permutation(N)[:n]] = np.arange(n)
        out.append(pal[idx].reshape(1, N, 1))
    return out


def framing_cases():
    """1 x N grey noise whose payload is 254, 255, 256, 509, 510 and 511 bytes. A prefix's codes
    are a prefix of the longer image's, so the size grows with N: a bisection finds the first N
    that reaches the target. The sizes a stream can have depend on the code count and m alone (one
    entry per code), so where the size steps over the target another m is tried, not another seed."""
    out = []
    for target in (254, 255, 256, 509, 510, 511):
        for m in (4, 2, 3, 5, 6, 7):
            n = 1 << m
            rng = np.random.default_rng(4242 + m)
            base = (rng.integers(0, n, 3000) * (255 // (n - 1))).astype(np.uint8)
            base[:n] = np.arange(n) * (255 // (n - 1))  # every level at any length from n on
            lo, hi = n, 3000
            while lo < hi:
                mid = (lo + hi) // 2
                if payload_size(base[:mid].reshape(1, mid, 1), -1) >= target:
                    hi = mid
                else:
                    lo = mid + 1
            a = base[:lo].reshape(1, lo, 1)
            if payload_size(a, -1) == target:
                out.append((f"payload{target}_m{m}", a, -1, 0, AUTO))
                break
        else:
            raise AssertionError(("no image with a payload of", target))
    return out


def table_full_cases():
    """Two fills at m = 8, fills at m = 2, and segments ending 0, 1 and 2 pixels after the pixel
    that filled the table (so that a Clear, a code and the segment's Clear follow each other)."""
    a8 = image(31, 96, 96, 1, 256, "noise")
    a2 = image(32, 200, 200, 1, 4, "noise")
    out = [("noise256_96x96", a8, -1, 0, AUTO), ("noise4_200x200", a2, -1, 0, AUTO)]
    for name, a in (("m8", a8), ("m2", a2)):
        plane, _, _, m = quantise(a)
        full = full_clear_positions(plane, m)
        assert len(full) >= 2, name
        for after in (0, 1, 2):
            seg = full[0] + 1 + after
            assert full_clear_positions(plane.reshape(-1)[:seg], m) == full[:1]
            out.append((f"{name}_seg_ends_{after}_after_full", a, seg, 0, AUTO))
    return out


def multi_wave_case():
    return [("noise256_512x512_default", image(41, 512, 512, 3, 256, "noise"), 0, 0, AUTO)]


_CACHE = {}


def corpus():
    """Every case of the grid the CPU and GPU tests share (rows apart: row_cases), built once."""
    if "corpus" not in _CACHE:
        _CACHE["corpus"] = grid_cases() + segment_end_cases() + table_full_cases() + framing_cases() + multi_wave_case()
    return _CACHE["corpus"]


def restated(case):
    """The restatement's file of a case, computed once per session and not changed after."""
    name = case[0]
    if name not in _CACHE:
        _CACHE[name] = write_gif(*case[1:])
    return _CACHE[name]
