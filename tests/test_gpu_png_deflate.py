"""GPU: the PNG encoder's deflate coder (icx_png.hip) held to its tokens. lodepng filters every row
of a palette image with type 0, so an 8-bit palette image of 17 to 256 colours hands the coder a
byte stream the test chooses: a 0 byte and the row's palette indices (in first-seen order, a
bijection of the indices given), with row length w + 1 and pixel width 1. Each case steers the
coder down one of its paths, runs the parity contract (pngutil.check) and the audit of
deflate_read.py on the IDAT, and shows from the decoded tokens that the path was reached."""
import numpy as np
import pytest

import imagecodecs_amd as icx
from oracle import pyoracle as O
import deflate_read as R
import pngutil as P

pytestmark = pytest.mark.gpu

SEG, BASE = 4096, 262144  # LZ77 segment and base deflate block of the coder (bytes of the filtered stream)

# 256 distinct colours, none of them grey (r = i, b = 255 - i): lodepng takes a palette, never grey
PAL = np.stack([np.arange(256), (np.arange(256) * 7 + 13) & 255, 255 - np.arange(256)], axis=1).astype(np.uint8)


def pal8(indices):
    """A 2-D uint8 array of palette indices -> the RGB image of those colours."""
    return np.ascontiguousarray(PAL[np.asarray(indices, np.uint8)])


@pytest.fixture(scope="module")
def ctx():
    c = icx.Context(0)
    yield c
    c.close()


def run(ctx, idx, audit=True):
    """Encode pal8(idx): colour type 3 / depth 8, the parity contract, the audit.
    -> (IDAT bytes, blocks, filtered stream, audit's per-code figures)."""
    px = pal8(idx)
    h, w, d = px.shape
    m = O.png_choose(px.tobytes(), w, h, d)
    assert (m.colortype, m.bitdepth) == (3, 8)
    png = P.check(ctx, px)
    idat = P.info(png)["idat"]
    F = O.png_filtered(px.tobytes(), w, h, d, m)
    assert len(F) == h * (w + 1) and set(F[:: w + 1]) == {0}
    blocks = R.read_zlib(idat)  # (the 2-byte header, the Adler-32 and the stream's exact end checked)
    stats = R.audit(blocks, F, log=print) if audit else None
    return idat, blocks, F, stats


def both_seams(ctx, idx, monkeypatch):
    """run with the default switch and with ICX_PNG_SEAM=0: with it no match crosses a segment end
    and the stream is no shorter. -> (default blocks, cut blocks, filtered stream)."""
    idat, blocks, F, _ = run(ctx, idx)
    monkeypatch.setenv("ICX_PNG_SEAM", "0")
    idat0, blocks0, _, _ = run(ctx, idx)
    monkeypatch.delenv("ICX_PNG_SEAM")
    assert R.crossing(blocks0, SEG) == []
    assert len(idat0) >= len(idat)
    return blocks, blocks0, F


def starts(blocks):
    """Stream position -> the token that starts there."""
    out, p = {}, 0
    for t in R.tokens(blocks):
        out[p] = t
        p += 1 if isinstance(t, int) else t[0]
    return out


def noise(seed, shape, n=200):
    return np.random.default_rng(seed).integers(0, n, shape).astype(np.uint8)


# ------------------------------------------------------------------------------------ limiters
def shuffled(seed, w, h, counts, lead=False):
    """Index k `counts[k]` times (the first one takes what is left of w x h), shuffled: an
    i.i.d.-like stream whose histogram is exactly the one asked for. `lead`: one of every index
    comes first, in an order that spreads neighbours in `counts` apart; the palette is in
    first-seen order, so this decides which symbols are neighbours in the block header."""
    cnt = np.array(counts, np.int64)
    cnt[0] += w * h - cnt.sum()
    assert cnt.min() >= 1 and len(cnt) <= 256
    rng = np.random.default_rng(seed)
    if not lead:
        v = np.repeat(np.arange(len(cnt)), cnt)
        rng.shuffle(v)
    else:
        first = np.argsort((np.arange(len(cnt)) * 0.6180339887498949) % 1.0, kind="stable")
        rest = np.repeat(np.arange(len(cnt)), cnt - 1)
        rng.shuffle(rest)
        v = np.concatenate([first, rest])
    return v.astype(np.uint8).reshape(h, w)


def skewed(seed, w, h, weights, lead=False):
    """`shuffled` with counts in proportion to `weights`, every index at least once."""
    wt = np.asarray(weights, np.float64)
    return shuffled(seed, w, h, np.maximum(1, np.floor(wt / wt.sum() * w * h).astype(np.int64)), lead)


def flat_and_tail(nflat=8, tail=0.03, ntail=16):
    """`nflat` equal values sharing 1 - tail, and `ntail` values at tail x 2^-k."""
    return [(1 - tail) / nflat] * nflat + [tail * 2.0 ** -k for k in range(1, ntail + 1)]


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[::-1]


def _depths(stats):
    return {c: max(s["depth"] for s in stats if s["code"] == c) for c in ("ll", "d", "cl")}


def test_limiter_flat_and_tail(ctx):
    """Eight flat values and a tail of 16 at 3 % x 2^-k on 511 x 511 (one deflate block): the
    unlimited literal/length tree is deeper than 15, so the 15-bit limiter runs; audit holds its
    code complete, within the limit and close to package-merge. (This image sends about 30
    code-length symbols; a code-length tree deeper than 7 needs at least 88 of them, so the 7-bit
    limiter has a case of its own below.)"""
    _, blocks, _, stats = run(ctx, skewed(1, 511, 511, flat_and_tail()))
    assert len(blocks) == 1
    d = _depths(stats)
    print("limiter flat+tail: unlimited depths", d, "worst ratio", max(s["ratio"] for s in stats))
    assert d["ll"] > 15, d
    assert max(blocks[0].ll_lens) == 15


def test_limiter_fibonacci(ctx):
    """Exact Fibonacci counts F25 .. F1 on 444 x 443: the histogram that asks for the deepest tree
    (the matches the coder finds among the frequent values flatten it again, but not to 15)."""
    _, blocks, _, stats = run(ctx, shuffled(2, 444, 443, fibonacci(25)))
    d = _depths(stats)
    print("limiter fibonacci: unlimited depths", d, "worst ratio", max(s["ratio"] for s in stats))
    assert d["ll"] > 15, d
    assert max(blocks[0].ll_lens) == 15


def test_limiter_code_length_code(ctx):
    """The 7-bit limiter of the code-length code. 255 values in groups of 1, 2, 3, 5, ... 89 (and
    24 frequent ones) at probability 2^-4 .. 2^-14 get code lengths 4 .. 14 in Fibonacci numbers;
    led in so that equal lengths are not neighbours in the header (no repeat symbols), the
    code-length symbols themselves have a Fibonacci histogram, whose tree is deeper than 7."""
    groups = [(5, 24), (4, 1), (6, 2), (7, 3), (8, 5), (9, 8), (10, 13), (11, 21), (12, 34), (13, 55), (14, 89)]
    weights = [2.0 ** -l for l, n in groups for _ in range(n)]
    _, blocks, _, stats = run(ctx, skewed(3, 511, 511, weights, lead=True))
    assert len(blocks) == 1
    d = _depths(stats)
    print("limiter code-length code: unlimited depths", d, "symbols", len(blocks[0].cl_syms),
          "worst ratio", max(s["ratio"] for s in stats))
    assert d["cl"] > 7, d
    assert max(blocks[0].cl_lens) == 7


# ------------------------------------------------------------------- no match, one distance
def test_block_without_a_match(ctx):
    """200-colour noise, 64 x 60: no match in the block, so two distance codes of one bit are
    forced (HDIST = 2 codes) to keep the distance code complete."""
    _, blocks, _, _ = run(ctx, noise(3, (60, 64)))
    assert len(blocks) == 1 and blocks[0].matches() == []
    assert blocks[0].hdist + 1 == 2 and blocks[0].d_lens == [1, 1]


def test_block_with_one_distance(ctx):
    """20 colours at the start of row 0, then the first colour alone: the rest of the stream is
    zero bytes, every match is at distance 1 (distance code 0), and code 1 is the padding."""
    idx = np.zeros((60, 64), np.uint8)
    idx[0, :20] = np.arange(20)
    _, blocks, _, _ = run(ctx, idx)
    ms = blocks[0].matches()
    assert len(blocks) == 1 and ms and {d for _, d in ms} == {1}
    assert blocks[0].hdist + 1 == 2 and blocks[0].d_lens == [1, 1]


# --------------------------------------------------------------------------------- window edge
def _rows3(w, shift, seed):
    """Three rows: 200-colour noise, and twice the row above moved right by `shift` pixels (left
    if negative; 0 copies it), the vacated pixels noise."""
    rng = np.random.default_rng(seed)
    idx = np.empty((3, w), np.uint8)
    idx[0] = rng.integers(0, 200, w)
    for y in (1, 2):
        idx[y] = np.roll(idx[y - 1], shift)
        if shift > 0:
            idx[y, :shift] = rng.integers(0, 200, shift)
        elif shift < 0:
            idx[y, shift:] = rng.integers(0, 200, -shift)
    return idx


@pytest.mark.parametrize("w,shift,reach", [(32767, 0, True), (32766, 1, True), (32768, -1, True),
                                           (32767, 1, False), (32766, 2, False), (32768, 0, False)])
def test_window_edge(ctx, w, shift, reach):
    """Rows whose only repeat lies rowlen + shift back: at exactly 32768 (the row candidate
    rowlen, rowlen + 1 or rowlen - 1) the rows below the first are coded as 258-byte matches at
    that distance; at 32769 (one past the window, which the token format would fold to distance 1)
    the candidate is off, no token goes that far and the rows are literals."""
    dist = (w + 1) + shift
    assert dist == (32768 if reach else 32769)
    _, blocks, F, _ = run(ctx, _rows3(w, shift, 40 + w + shift))
    ms = [t for b in blocks for t in b.matches()]
    assert all(d <= 32768 for _, d in ms)
    far = [t for t in ms if t[1] == 32768]
    if reach:
        assert (258, 32768) in far and sum(n for n, _ in far) > 60000  # nearly all of rows 1 and 2
    else:
        assert far == [] and sum(n for n, _ in ms) < 2000  # (chance repeats of the noise only)


# ----------------------------------------------------------------------------------- tiny rows
@pytest.mark.parametrize("w", [1, 2, 3, 7])
def test_tiny_rows(ctx, w):
    """Rows of 2 to 8 bytes (more than two segments of them): the row candidates rowlen - 1, rowlen
    and rowlen + 1 collide with the pixel candidates 1, 1 and 2. The rows repeat in bands (the row
    above as it is, and moved one pixel to either side), so every candidate is worth taking; no
    distance outside the candidates may appear."""
    h = 8400 // (w + 1) + 1
    step = np.repeat(np.resize(np.array([0, 1, -1, 0], np.int64), (h + 39) // 40), 40)[:h]
    step[::97] += 5  # (a new band: nothing to copy)
    idx = ((np.arange(w)[None, :] + np.cumsum(step)[:, None]) % 19).astype(np.uint8)
    assert h * (w + 1) > 2 * SEG
    _, blocks, F, _ = run(ctx, idx)
    dists = {d for b in blocks for _, d in b.matches()}
    cands = {1, 2, w + 1, w, w + 2} - {0}
    assert dists and dists <= cands, (dists, cands)
    assert w + 1 in dists
    if w == 7:
        assert {7, 8, 9} <= dists, dists


# --------------------------------------------------------------------------------------- seams
def _const(w, h):
    idx = np.zeros((h, w), np.uint8)
    idx[0, :20] = np.arange(20)
    return idx


def test_seam_constant_stream_cuts(ctx, monkeypatch):
    """(i) zero bytes over more than three segments: a segment's own 258-byte matches and the
    re-parse from the overhang never meet within the 32 head slots, so the seams before whole
    segments cut: no match crosses those segment ends, with the switch or without. (The short last
    segment is re-parsed whole within the head, so the match into it stays.)"""
    blocks, blocks0, F = both_seams(ctx, _const(127, 100), monkeypatch)
    assert 3 * SEG < len(F) < 4 * SEG
    assert [c for c in R.crossing(blocks, SEG) if c[0] < 2 * SEG] == []
    assert [c[0] // SEG for c in R.crossing(blocks, SEG)] == [2]  # into the last segment only
    assert (258, 1) in R.tokens(blocks)


def _planted(seed, rows, plants):
    """200-colour noise of 255-pixel rows (row length 256: every 4096 multiple is a row's type
    byte) in which, for each (k, before, after), the bytes from `before` before stream position
    4096 k to `after` after it repeat the row above."""
    idx = noise(seed, (rows, 255))
    flat = np.zeros((rows, 256), np.uint8)
    flat[:, 1:] = idx
    s = flat.reshape(-1)
    for k, before, after in plants:
        p = SEG * k
        for i in range(p - before, p + after):  # (byte by byte: a repeat longer than its distance)
            s[i] = s[i - 256]
        for i in (p - before - 1, p + after):  # the repeat is exactly that long
            assert i % 256
            if s[i] == s[i - 256]:
                s[i] = (s[i] + 1) % 200
    assert (flat[:, 0] == 0).all()
    return np.ascontiguousarray(flat[:, 1:])


def test_seam_joins(ctx, monkeypatch):
    """(ii) repeats of the row above that run 1, 2, 3 and 257 bytes past a segment end: the next
    segment's parse is joined to the overhang (directly or through a re-parsed head), so the
    decoded matches cross those segment ends; with ICX_PNG_SEAM=0 none does."""
    plants = [(1, 40, 1), (2, 40, 2), (3, 40, 3), (4, 1, 300), (5, 100, 100)]
    blocks, blocks0, F = both_seams(ctx, _planted(5, 100, plants), monkeypatch)
    cross = {(p + n) - (p + n) // SEG * SEG: (p, n, d) for p, n, d in R.crossing(blocks, SEG)}
    print("seam joins: crossing matches by overhang", cross)
    assert cross, "no match crosses a segment end"
    assert {1, 2, 3, 257} <= set(cross), sorted(cross)
    assert all(d == 256 for _, _, d in cross.values())


def test_seam_cut_to_literals(ctx, monkeypatch):
    """(iii) a repeat that begins 1 or 2 bytes before a segment end: cut at the seam
    (ICX_PNG_SEAM=0) less than a match is left, and those bytes become literals in place."""
    plants = [(1, 1, 60), (2, 2, 60), (3, 3, 60)]
    blocks, blocks0, F = both_seams(ctx, _planted(6, 100, plants), monkeypatch)
    at, at0 = starts(blocks), starts(blocks0)
    for k, before, after in plants:
        p = SEG * k - before
        assert at[p] == (before + after, 256), (k, at.get(p))  # default: one match across the seam
        if before < 3:
            assert [at0.get(p + i) for i in range(before)] == list(F[p:p + before]), k
        else:
            assert at0[p] == (3, 256)
        assert at0[SEG * k] == (after, 256)


TAILS = {1: (2730, 3), 2: (481, 17), 3: (148, 55), 10: (1366, 6)}  # r -> (w, h): h (w + 1) = 8192 + r


@pytest.mark.parametrize("r", [1, 2, 3, 10])
@pytest.mark.parametrize("tail", ["run", "noise"])
def test_seam_final_short_segment(ctx, monkeypatch, r, tail):
    """(iv), (v) a last segment of r bytes. After a run of the first colour (zero bytes) the match
    that begins before 8192 runs to the end of the stream and swallows the last segment whole;
    after noise the last segment is r literals. Both also with ICX_PNG_SEAM=0."""
    w, h = TAILS[r]
    assert h * (w + 1) == 2 * SEG + r
    idx = noise(7 + r, (h, w))
    N = h * (w + 1)
    if tail == "run":
        idx[-1, -(100 + r + 1):] = idx[0, 0]
        idx[-1, -(100 + r + 2)] = (idx[0, 0] + 1) % 200  # the run begins there
    blocks, blocks0, F = both_seams(ctx, idx, monkeypatch)
    toks = R.tokens(blocks)
    if tail == "run":
        assert set(F[N - 100 - r - 1:]) == {0}
        assert toks[-1] == (100 + r, 1), toks[-3:]  # from 8092 to the end, over the segment end at 8192
        assert [c for c in R.crossing(blocks, SEG) if c[0] > SEG] == [(2 * SEG - 100, 100 + r, 1)]
        t0 = R.tokens(blocks0)
        assert t0[-2:] == ([(100, 1), (r, 1)] if r >= 3 else [(100, 1)] + [0] * r)[-2:]
    else:
        assert toks[-r:] == list(F[-r:])


# ---------------------------------------------------------------------------------- block ends
def _banded(w, h):
    """Compressible: every row the row above but for a few pixels, over a 20-colour noise row."""
    rng = np.random.default_rng(w + h)
    idx = np.empty((h, w), np.uint8)
    idx[0] = rng.integers(0, 20, w)
    for y in range(1, h):
        idx[y] = idx[y - 1]
        idx[y, rng.integers(0, w, 3)] = rng.integers(0, 20, 3)
    return idx


@pytest.mark.parametrize("w,h", [(511, 512), (511, 513), (52428, 5)])
@pytest.mark.parametrize("kind", ["noise", "banded"])
def test_block_ends(ctx, w, h, kind):
    """A stream that ends with its base block (262144 bytes), 512 bytes and one byte into the next
    one (52428 x 5: rows longer than the window, every row candidate off)."""
    idx = noise(w, (h, w)) if kind == "noise" else _banded(w, h)
    _, blocks, F, _ = run(ctx, idx)
    N = len(F)
    assert N == {512: BASE, 513: BASE + 512, 5: BASE + 1}[h]
    assert all(b.out[0] % BASE == 0 for b in blocks) and len(blocks) <= (N + BASE - 1) // BASE
    if kind == "noise":
        assert len(blocks) == (N + BASE - 1) // BASE  # too many symbols to share a block
        if N == BASE + 1:
            assert blocks[1].tokens == [F[-1]] and blocks[1].d_lens == [1, 1]
    if w == 52428:
        assert all(d <= 2 for b in blocks for _, d in b.matches())


# ------------------------------------------------------------------------------- merged blocks
def test_merged_blocks(ctx, monkeypatch):
    """4 MiB of filtered bytes (2047 x 2048: 16 base blocks) with a few thousand symbols per base
    block: the plan gives several base blocks one deflate block, and more than one such group.
    The same file with the plan's counts read from global memory (ICX_PNG_PLAN_LDS=0)."""
    w, h = 2047, 2048
    rng = np.random.default_rng(8)
    idx = np.empty((h, w), np.uint8)
    idx[0] = rng.integers(0, 200, w)
    for y in range(1, h):
        idx[y] = idx[y - 1]
        idx[y, rng.integers(0, w, 10)] = rng.integers(0, 200, 10)
        if y % 128 == 127:  # the last byte of a base block repeats nothing: no match runs into the next one
            idx[y, -1] = (idx[y - 1, -1] + 1 + rng.integers(0, 198)) % 200
    idat, blocks, F, _ = run(ctx, idx)
    nbase = len(F) // BASE
    assert len(F) == 16 * BASE and sum(len(b.tokens) for b in blocks) < 300000
    spans = [(b.out[0] // BASE, b.out[1] // BASE) for b in blocks]
    print("merged blocks: base blocks per deflate block", [e - s for s, e in spans])
    assert 1 < len(blocks) < nbase
    assert all(b.out[0] % BASE == 0 and b.out[1] % BASE == 0 for b in blocks)
    assert sum(1 for s, e in spans if e - s > 1) >= 2  # a second merged group
    monkeypatch.setenv("ICX_PNG_PLAN_LDS", "0")
    px = pal8(idx)
    assert P.info(ctx.png_encode(w, h, 3, px.tobytes()))["idat"] == idat


# ------------------------------------------------------------------------------- output bounds
def test_output_bounds(ctx):
    """The file at each of the 16 byte residues of the output address, in a buffer filled with
    0xAB: with cap = the file's size it is written and no byte outside it changes (the 16-byte
    zeroing before the emit stays inside the file); with cap one less nothing is written at all."""
    import torch
    idx = noise(9, (60, 100))
    px = pal8(idx)
    want = ctx.png_encode(100, 60, 3, px.tobytes())
    n = len(want)
    enc = icx.PngEncoder(ctx)
    d_src = torch.from_numpy(px).cuda()
    buf = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    first = (-buf.data_ptr()) % 16 + 64  # a 16-byte aligned address inside the buffer
    for res in range(16):
        base = first + res
        assert (buf.data_ptr() + base) % 16 == res
        buf.fill_(0xAB)
        rc, need = enc.encode_device(100, 60, 3, d_src.data_ptr(), buf.data_ptr() + base, n - 1)
        assert (rc, need) == (icx.OUT_OF_MEM, n), res
        assert bool((buf == 0xAB).all()), res
        rc, got = enc.encode_device(100, 60, 3, d_src.data_ptr(), buf.data_ptr() + base, n)
        assert (rc, got) == (icx.OK, n), res
        host = buf.cpu().numpy()
        assert host[base:base + n].tobytes() == want, res
        assert (host[:base] == 0xAB).all() and (host[base + n:] == 0xAB).all(), res
    enc.close()
