"""The crafted deflate corpus (deflate_craft): streams aimed at the edges of the two inflates
(exr_inflate in icx_exr_core.h, exr_inflate_wave in icx_inflate_wave.h) that a compressor's output
never reaches. Shared by the CPU tests (test_inflate_craft.py: zlib and the portable inflate) and
the GPU tests (test_gpu_inflate.py: the wave inflate behind the PNG and OpenEXR reads).

A Case holds the zlib stream `z`, `full` = the bytes it must inflate to, from its construction
(None: an invalid stream, every decoder must refuse it), `need` = the output size the caller
expects (the image's filtered bytes: the reads accept a stream only when it gives exactly that
many), and `lenient`: zlib refuses the stream, this project's inflate accepts it with `full`.
The first output byte of every valid stream is 0, a PNG row's filter type None."""
import functools
from collections import namedtuple

import numpy as np

import deflate_craft as D

WIN = 16384    # kPngdWin and the default ICX_EXR_WIN (a build-time knob of the OpenEXR read): the LDS ring
FLUSH = 4096   # exr_inflate_wave's kFlush: ring -> output every 4 KiB
FAST = 9       # kInfFast: codes up to 9 bits decode from the direct table

Case = namedtuple("Case", "name z full need lenient")


def case(name, z, full, need=None, lenient=False):
    return Case(name, bytes(z), full, (len(full) if full is not None else 64) if need is None else need, lenient)


def _rand(seed, n):
    """n random bytes, the first one 0."""
    b = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if n:
        b[0] = 0
    return b.tobytes()


def _ll(table, n=None):
    """{symbol: length} -> the list of lengths (n entries, default up to the last symbol, >= 257)."""
    n = max(257, max(table) + 1) if n is None else n
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


LL286 = [8] * 226 + [9] * 60   # a complete code over all 286 literal/length symbols
D30 = [4] * 2 + [5] * 28       # and over all 30 distance symbols
assert D.kraft(LL286) == 32768 and D.kraft(D30) == 32768


def _dyn(tokens, ll, dl, **kw):
    return D.zstream(D.Deflate().dynamic(tokens, ll, dl, final=True, **kw), D.apply(tokens))


# ------------------------------------------------------------------------------------ long codes
def long_codes():
    out = []
    # lengths 1..8 on eight literals, 128 symbols of 15 bits (256, 257, 285 among them); distance
    # lengths 1..15, 15
    longs = [256, 257, 285] + list(range(100, 225))
    assert len(longs) == 128
    ll = _ll({**{s: s + 1 for s in range(8)}, **{s: 15 for s in longs}}, 286)
    dl = list(range(1, 16)) + [15]
    assert D.kraft(ll) == 32768 and D.kraft(dl) == 32768
    tok = [0] + list(range(100, 225)) + list(range(8)) * 12
    tok += [(258, 1), 3, (3, 16), 5, (258, 193)]
    tok += [(3, d) for d in (25, 33, 49, 65, 97, 129, 193, 256)] + [7, (258, 1), (3, 2)]  # distance codes 9..15
    tok += [(258, 200), 101, (3, 13)]
    out.append(case("long: 1..8 and 128 x 15 bits", _dyn(tok, ll, dl), D.apply(tok)))
    # one symbol at each length 1..14 and two of 15: every lim[l] branch of inf_decode_w
    t = {s: s + 1 for s in range(9)}
    t.update({200: 10, 201: 11, 256: 12, 257: 13, 285: 14, 202: 15, 203: 15})
    ll = _ll(t, 286)
    assert D.kraft(ll) == 32768
    tok = [0] + [1, 2, 3, 4, 5, 6, 7, 8, 200, 201, 202, 203] * 20 + [(3, 7), 201, (258, 1), 203, (258, 240), 200, (3, 1)]
    out.append(case("long: one symbol per length 1..15", _dyn(tok, ll, dl), D.apply(tok)))
    # two symbols at each length 10..14, four of 15 (the second code of a length: off[l] + c)
    t = {s: s + 1 for s in range(8)}
    lits = iter(range(150, 170))
    for l in (10, 11, 12, 13, 14):
        t[next(lits)] = l
        t[next(lits)] = l
    t.update({256: 15, 257: 15, 285: 15, 170: 15})
    t[159], t[284] = 0, 14  # (a length symbol at 14 bits too)
    t = {s: l for s, l in t.items() if l}
    ll = _ll(t, 286)
    assert D.kraft(ll) == 32768, D.kraft(ll)
    used = sorted(s for s in t if s < 256)
    tok = [0] + used * 15 + [(258, 1), (227, 30), 170, (3, 2), (258, 100)]
    out.append(case("long: two symbols per length 10..14", _dyn(tok, ll, dl), D.apply(tok)))
    # the 9 / 10 bit split at kInfFast: two 9-bit and four 10-bit codes next to each other
    t = {s: s + 1 for s in range(7)}
    t.update({50: FAST, 256: FAST, 51: FAST + 1, 52: FAST + 1, 257: FAST + 1, 285: FAST + 1})
    ll = _ll(t, 286)
    assert D.kraft(ll) == 32768
    tok = [0] + [1, 2, 3, 4, 5, 6, 50, 51, 52] * 30 + [(3, 1), 51, (258, 9), 50, 52, (258, 256)]
    out.append(case("long: 9 and 10 bits at kInfFast", _dyn(tok, ll, dl), D.apply(tok)))
    return out


# ---------------------------------------------------------------------------------- header forms
def header_forms():
    out = []
    tok3 = [0, 0, 0, (3, 1), (3, 2), 0]
    # 16 as the first code-length symbol: nothing to repeat
    ll = _ll({0: 1, 256: 2, 257: 2})
    syms = [(16, 0)] + D.plain_cl(ll[3:] + [1, 1])
    z = D.zstream(D.Deflate().dynamic(tok3, ll, [1, 1], final=True, cl_syms=syms), D.apply(tok3))
    out.append(case("header: 16 first", z, None))
    # runs that cross from the literal/length lengths into the distance lengths
    ll = _ll({0: 1, 256: 2, 257: 2}, 270)
    dl = [0, 0, 0, 0, 0, 0, 1, 1]
    syms = D.plain_cl(ll[:258]) + [(18, 7)] + [(1, 0), (1, 0)]  # 18: ll 258..269 and distance 0..5
    assert D.expand_cl(syms) == ll + dl
    tok = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (3, 9), (3, 13), 0]  # distance codes 6 and 7
    out.append(case("header: 18 crosses into the distance lengths", _dyn(tok, ll, dl, cl_syms=syms), D.apply(tok)))
    ll = _ll({0: 1, 256: 2, 257: 2}, 258)
    dl = [2, 2, 2, 2]
    syms = D.plain_cl(ll[:257]) + [(16, 2)]  # 16: ll 257 and distance 0..3 repeat the 2 of symbol 256
    assert D.expand_cl(syms) == ll + dl
    tok = [0, 0, 0, 0, (3, 1), (3, 2), (3, 3), (3, 4), 0]
    out.append(case("header: 16 crosses into the distance lengths", _dyn(tok, ll, dl, cl_syms=syms), D.apply(tok)))
    ll = _ll({0: 1, 256: 2, 257: 2}, 261)
    dl = [0, 0, 1, 1]
    syms = D.plain_cl(ll[:258]) + [(17, 2), (1, 0), (1, 0)]  # 17: ll 258..260 and distance 0, 1
    assert D.expand_cl(syms) == ll + dl
    tok = [0, 0, 0, 0, (3, 3), (3, 4), 0]
    out.append(case("header: 17 crosses into the distance lengths", _dyn(tok, ll, dl, cl_syms=syms), D.apply(tok)))
    # a mix of all three run symbols, 18 at its longest (138)
    ll = _ll({0: 2, 1: 2, 2: 2, 256: 3, 257: 3}, 257 + 1)
    dl = [1, 1]
    syms = [(2, 0), (2, 0), (2, 0), (18, 127), (17, 7), (18, 94), (3, 0), (3, 0), (1, 0), (1, 0)]  # 3 + 138 + 10 + 105 = 256
    assert D.expand_cl(syms) == ll + dl
    tok = [0, 1, 2, 2, 1, (3, 1), (3, 2), 0]
    out.append(case("header: 17 and 18 at their longest", _dyn(tok, ll, dl, cl_syms=syms), D.apply(tok)))
    # a run that overshoots HLIT + HDIST by one
    ll = _ll({0: 1, 256: 2, 257: 2}, 270)
    syms = D.plain_cl(ll[:258]) + [(18, 10)]  # 21 zeros where 12 + 8 lengths are left
    d = D.Deflate().dynamic([], ll, [0] * 8, final=True, cl_syms=syms, header_only=True)
    d.b.put(0, 24)
    out.append(case("header: 18 overshoots by one", D.zstream(d, b""), None))
    ll = _ll({0: 1, 256: 2, 257: 2}, 258)
    syms = D.plain_cl(ll[:257]) + [(16, 3)]  # 6 repeats where 1 + 4 lengths are left
    d = D.Deflate().dynamic([], ll, [2, 2, 2, 2], final=True, cl_syms=syms, header_only=True)
    d.b.put(0, 24)
    out.append(case("header: 16 overshoots by one", D.zstream(d, b""), None))
    # HLIT 29 / 30 and HDIST 29 / 30
    tok = list(_rand(1, 300)) + [(258, 1), (3, 4), (258, 290), 9]
    out.append(case("header: HLIT 29 (286 codes)", _dyn(tok, LL286, D30), D.apply(tok)))
    ll287 = [8] * 225 + [9] * 62
    assert D.kraft(ll287) == 32768
    out.append(case("header: HLIT 30 (287 codes)", D.zstream(D.Deflate().dynamic(tok, ll287, D30, final=True), D.apply(tok)), None))
    d31 = [4] + [5] * 30
    assert D.kraft(d31) == 32768
    out.append(case("header: HDIST 30 (31 codes)", D.zstream(D.Deflate().dynamic(tok, LL286, d31, final=True), D.apply(tok)), None))
    tok = list(_rand(2, 40)) + [(5, 30), (258, 1)]
    out.append(case("header: HDIST 29 (30 codes)", _dyn(tok, LL286, D30), D.apply(tok)))
    # HCLEN 4: only 16, 17, 18 and 0 have a code -- every length is 0, no end-of-block code
    ll, dl = [0] * 257, [0]
    syms = [(18, 127), (18, 109)]  # 138 + 120 zeros
    assert D.expand_cl(syms) == ll + dl
    cl = [0] * 19
    cl[0], cl[18] = 1, 1
    d = D.Deflate().dynamic([], ll, dl, final=True, cl_syms=syms, cl_lens=cl, hclen=4, header_only=True)
    d.b.put(0, 16)
    out.append(case("header: HCLEN 4", D.zstream(d, b""), None))
    # HCLEN 19: the last code-length code in the RFC's order (15) is used
    ll = _ll({0: 1, 1: 2, 2: 3, 256: 4, 257: 5, 3: 6, 4: 7, 5: 8, 6: 9, 7: 10, 8: 11, 9: 12, 10: 13, 11: 14, 12: 15, 13: 15})
    assert D.kraft(ll) == 32768
    tok = list(range(14)) * 3 + [(3, 1), (3, 2)]
    d = D.Deflate().dynamic(tok, ll, [1, 1], final=True)
    out.append(case("header: HCLEN 19", D.zstream(d, D.apply(tok)), D.apply(tok)))
    # an over-subscribed and an incomplete code-length code
    ll = _ll({0: 1, 256: 2, 257: 2})
    for name, cl in (("over-subscribed", {0: 1, 1: 1, 2: 1}), ("incomplete", {0: 2, 1: 2, 2: 2})):
        d = D.Deflate().dynamic(tok3, ll, [1, 1], final=True, cl_lens=_ll(cl, 19))
        out.append(case("header: %s code-length code" % name, D.zstream(d, D.apply(tok3)), None))
    # a block whose only symbol is the end of block, one bit long, and no distance code
    data = _rand(3, 20)
    d = D.Deflate().stored(data).dynamic([], _ll({256: 1}), [0], final=True)
    out.append(case("header: only EOB, 1 bit, no distance code", D.zstream(d, data), data))
    d = D.Deflate().dynamic([], _ll({256: 1}), [0]).stored(data).dynamic([], _ll({256: 1}), [0]).fixed(final=True)
    out.append(case("header: only-EOB blocks first and in the middle", D.zstream(d, data), data))
    return out


def leniencies():
    """Streams zlib refuses and inf_build's rule (miniz's: an incomplete code fails only with two or
    more used symbols) accepts; `full` is what this project's inflate must give."""
    out = []
    data = _rand(4, 20)
    for l in (2, 7, 15):
        d = D.Deflate().stored(data).dynamic([], _ll({256: l}), [0], final=True)
        out.append(case("lenient: one literal/length code of %d bits" % l, D.zstream(d, data), data, lenient=True))
    ll = _ll({0: 1, 256: 2, 257: 2})
    tok = [0, 0, (3, 1), 0, (3, 1)]
    for l in (2, 9, 15):
        out.append(case("lenient: one distance code of %d bits" % l, _dyn(tok, ll, [l]), D.apply(tok), lenient=True))
    tok = [0, 0, 0, 0, 0, (3, 5)]  # the one code is not the first symbol
    out.append(case("lenient: one distance code (symbol 4) of 3 bits", _dyn(tok, ll, [0, 0, 0, 0, 3]), D.apply(tok), lenient=True))
    # the zlib header's window size above 32 KiB (CINFO 8..15): only the method's four bits are read
    tok = list(_rand(5, 30)) + [(4, 9)]
    body = D.Deflate().fixed(tok, final=True).raw()
    for cmf in (0x88, 0xF8):
        out.append(case("lenient: CMF %#x" % cmf, D.zwrap(body, D.apply(tok), cmf=cmf), D.apply(tok), lenient=True))
    return out


def zlib_headers():
    out = []
    tok = list(_rand(6, 30)) + [(4, 9)]
    body, data = D.Deflate().fixed(tok, final=True).raw(), D.apply(tok)
    for cmf in (0x08, 0x18, 0x48, 0x78):
        for level in (0, 1, 2, 3):
            flg = level << 6
            flg += (31 - (cmf * 256 + flg) % 31) % 31
            out.append(case("zlib: CMF %#x FLG %#x" % (cmf, flg), D.zwrap(body, data, cmf=cmf, flg=flg), data))
    out.append(case("zlib: FDICT", D.zwrap(body, data, flg=0x80 + 0x20 + (31 - (0x7800 + 0xA0) % 31) % 31), None))
    out.append(case("zlib: check bits off by one", D.zwrap(body, data, flg=0x9D), None))
    out.append(case("zlib: method 7", D.zwrap(body, data, cmf=0x77), None))
    out.append(case("zlib: method 9", D.zwrap(body, data, cmf=0x79), None))
    out.append(case("zlib: block type 3", D.zwrap(bytes([0x07, 0, 0]), b""), None))
    return out


# ------------------------------------------------------------------------------- invalid symbols
def invalid_symbols():
    out = []
    pre = list(_rand(7, 12))
    for s in (286, 287):
        d = D.Deflate().fixed(pre + [("ll", s), ("bits", 0, 10), 1, 2], final=True)
        out.append(case("symbol: fixed literal/length %d" % s, D.zstream(d, bytes(pre)), None))
    for c in (30, 31):
        d = D.Deflate().fixed(pre + [("dc", 3, c), ("bits", 0, 13), 1, 2], final=True)
        out.append(case("symbol: fixed distance %d" % c, D.zstream(d, bytes(pre)), None))
    ll = _ll({0: 1, 256: 2, 257: 2})
    tok = [0, 0, ("ll", 257), ("bits", 1, 1), 0]  # the one distance code is the bit 0
    d = D.Deflate().dynamic(tok, ll, [1], final=True)
    out.append(case("symbol: the absent code of a one-code distance table", D.zstream(d, b"\0\0\0\0\0\0"), None))
    tok = [0, 0, (3, 1), 0]
    out.append(case("symbol: the present code of a one-code distance table", _dyn(tok, ll, [1]), D.apply(tok)))
    tok = [0, 5, 6, (3, 3), 7]
    out.append(case("symbol: dist == out at 3", D.zstream(D.Deflate().fixed(tok, final=True), D.apply(tok)), D.apply(tok)))
    d = D.Deflate().fixed([0, 5, 6, (3, 4), 7], final=True)
    out.append(case("symbol: dist == out + 1 at 3", D.zstream(d, b"\0\5\6\0\5\6\7"), None, need=7))
    big = _rand(8, WIN + 6)
    for dist, ok in ((len(big), True), (len(big) + 1, False)):
        d = D.Deflate().stored(big).fixed([(3, dist), 7], final=True)
        full = big + big[:3] + b"\7"
        out.append(case("symbol: dist == out%s at %d" % ("" if ok else " + 1", len(big)), D.zstream(d, full),
                        full if ok else None, need=len(full)))
    return out


# -------------------------------------------------------------------------------- ring or output
def ring_or_output():
    """Matches on both sides of dist + len == W (from the ring, or from the flushed output) and of
    dist == W (the farthest byte the ring still holds), each followed by literals and (258, 1) so
    that a wrong byte spreads."""
    out = []
    for n in (3, 100, 258):
        for dist in (WIN - n - 1, WIN - n, WIN - n + 1, WIN, WIN + 1, 19999, 32768):
            pre = _rand(100 + n, 33000 if dist == 32768 else 20000)
            tok = [(n, dist), 1, 2, 3, (258, 1), (n, dist), (258, dist - 7), 9]
            d = D.Deflate().stored(pre).fixed(tok, final=True)
            full = D.apply(list(pre) + tok)
            out.append(case("ring: len %d dist %d" % (n, dist), D.zstream(d, full), full))
    return out


def repeats():
    """dist < len repeats (k % dist) that straddle a flush boundary and the ring's wrap."""
    out = []
    for dist in (1, 2, 3, 63, 64, 65, 257):
        a = _rand(200 + dist, FLUSH - 100)
        b = _rand(300 + dist, WIN - 100 - (FLUSH - 100 + 258))
        tok = list(a) + [(258, dist)] + list(b) + [(258, dist), 4, 5, (258, 1)]
        full = D.apply(tok)
        assert len(a) < FLUSH < len(a) + 258 and len(a) + 258 + len(b) == WIN - 100
        d = D.Deflate().stored(a).fixed([(258, dist)]).stored(b).fixed([(258, dist), 4, 5, (258, 1)], final=True)
        out.append(case("repeat: dist %d over 4096 and 16384" % dist, D.zstream(d, full), full))
    return out


# ---------------------------------------------------------------------------------- flush and cap
def flush_and_cap():
    out = []
    for n in (FLUSH - 1, FLUSH, FLUSH + 1, 2 * FLUSH, WIN - 1, WIN, WIN + 1):
        data = _rand(n, n)
        out.append(case("flush: %d literals" % n, D.zstream(D.Deflate().fixed(list(data), final=True), data), data))
        tok = list(data[:n - 200]) + [(200, 1000)]
        out.append(case("flush: %d ending in a match" % n, D.zstream(D.Deflate().fixed(tok, final=True), D.apply(tok)), D.apply(tok)))
        d = D.Deflate().stored(data[:n - 50]).stored(data[n - 50:], final=True)
        out.append(case("flush: %d stored" % n, D.zstream(d, data), data))
    # one byte more / fewer than the image needs
    for need in (300, FLUSH, 5000):
        for delta in (1, -1):
            n = need + delta
            data = _rand(need, n)
            how = "more" if delta > 0 else "fewer"
            z = D.zstream(D.Deflate().fixed(list(data), final=True), data)
            out.append(case("cap %d: one byte %s, literals" % (need, how), z, data, need=need))
            tok = list(data[:n - 40]) + [(40, 100)]
            z = D.zstream(D.Deflate().fixed(tok, final=True), D.apply(tok))
            out.append(case("cap %d: one byte %s, in a match" % (need, how), z, D.apply(tok), need=need))
            z = D.zstream(D.Deflate().fixed(list(data[:n - 30])).stored(data[n - 30:], final=True), data)
            out.append(case("cap %d: one byte %s, in a stored block" % (need, how), z, data, need=need))
    data = _rand(9, 1000 + FLUSH + 904)
    out.append(case("cap 1000: literals overrun by more than 4096", D.zstream(D.Deflate().fixed(list(data), final=True), data),
                    data, need=1000))
    return out


# ---------------------------------------------------------------------------------- stored blocks
def stored_blocks():
    out = []
    data = _rand(10, 60)
    lit = list(data)
    d = D.Deflate().stored().fixed(lit, final=True)
    out.append(case("stored: LEN 0 first", D.zstream(d, data), data))
    d = D.Deflate().fixed(lit[:30]).stored().stored().fixed(lit[30:], final=True)
    out.append(case("stored: LEN 0 in the middle", D.zstream(d, data), data))
    d = D.Deflate().fixed(lit).stored(final=True)
    out.append(case("stored: LEN 0 final", D.zstream(d, data), data))
    d = D.Deflate().stored(data, nlen=(60 ^ 0xFFFF) ^ 0x100, final=True)
    out.append(case("stored: wrong NLEN", D.zstream(d, data), None))
    d = D.Deflate().stored(data, nlen=60, final=True)
    out.append(case("stored: NLEN == LEN", D.zstream(d, data), None))
    d = D.Deflate().stored(data[:40], length=60, final=True)
    out.append(case("stored: cut in its data", D.zwrap(d.raw(), b"")[:-4], None))
    d = D.Deflate().stored(data[:56], length=60, final=True)
    out.append(case("stored: the trailer's bytes taken as data", D.zstream(d, data), None))
    offs = set()
    for j in range(8):  # j nine-bit literals: the stored block's header starts at each bit offset
        t = [0] + [200] * j + [1, 2]
        d = D.Deflate().fixed(t)
        o = d.b.nbits % 8
        offs.add(o)
        d.stored(data[1:]).fixed(t[1:]).stored(data[:7], final=True)
        full = bytes(t) + data[1:] + bytes(t[1:]) + data[:7]
        out.append(case("stored: after a fixed block ending at bit %d" % o, D.zstream(d, full), full))
    assert offs == set(range(8))
    return out


def stored_65535():
    data = _rand(11, 65535 + 10)
    d = D.Deflate().stored(data[:65535]).stored(data[65535:], final=True)
    return [case("stored: LEN 65535 and a second block", D.zstream(d, data), data)]


# -------------------------------------------------------------------------------------- input end
@functools.lru_cache(None)
def end_streams():
    """(name, z, full): a fixed block of 200 literals and a match; a dynamic stream of about 600 bytes."""
    tok = list(_rand(12, 200)) + [(20, 150)]
    a = D.zstream(D.Deflate().fixed(tok, final=True), D.apply(tok))
    tok2 = list(_rand(13, 490)) + [(30, 400), 7, (258, 1)]
    b = _dyn(tok2, LL286, D30)
    assert 550 <= len(b) <= 650, len(b)
    return (("fixed", a, D.apply(tok)), ("dynamic", b, D.apply(tok2)))


def truncations():
    return [case("end: %s cut to %d of %d" % (name, k, len(z)), z[:k], None, need=len(full))
            for name, z, full in end_streams() for k in range(len(z))]


def trailing_junk():
    return [case("end: %s and %d junk bytes" % (name, k), z + b"\xA5\x5A\xFF"[:k], full)
            for name, z, full in end_streams() for k in range(4)]


# ---------------------------------------------------------------------------------- window reader
def window_lengths():
    """Streams of every length around the 256- and 512-byte edges of InW's register window."""
    out = []
    for lo, hi, lits in ((250, 262, 180), (506, 518, 420)):
        tok = list(_rand(lo, lits)) + [(9, 33)]
        for n in range(lo, hi + 1):
            out.append(case("window: %d bytes" % n, D.stretch(tok, n), D.apply(tok)))
    return out


# ------------------------------------------------------------------------------------------ Adler
def _tune(data, want1=None, want2=None):
    """`data` with a few bytes changed so that the Adler-32 halves come out as asked."""
    b = np.frombuffer(data, np.uint8).astype(np.int64).copy()
    n = len(b)
    if want1 is not None:  # 1 + sum == want1 (mod 65521): move the sum byte by byte (not byte 0)
        need = (want1 - 1 - int(b.sum())) % 65521
        for i in range(1, n):
            step = min(need, 255 - int(b[i]))
            b[i] += step
            need -= step
        assert need == 0
    else:  # n + sum (n - i) b_i == want2: two bytes of different weight
        base = b.copy()
        base[n - 1] = base[n - 300] = 0
        rest = (n + int(((n - np.arange(n)) * base).sum())) % 65521
        x, y = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        hit = np.argwhere((rest + x * 1 + y * 300) % 65521 == want2)
        assert len(hit)
        base[n - 1], base[n - 300] = hit[0]
        b = base
    return b.astype(np.uint8).tobytes()


def adler_cases():
    import zlib
    out = []
    tok = list(_rand(14, 100)) + [(50, 60)]
    data = D.apply(tok)
    body = D.Deflate().fixed(tok, final=True).raw()
    good = zlib.adler32(data)
    for k in range(4):
        for bit in (0x01, 0x80):
            out.append(case("adler: trailer byte %d ^ %#x" % (k, bit), D.zwrap(body, data, adler=good ^ (bit << (8 * k))), None,
                            need=len(data)))
    for half, want in (("a1", 0), ("a1", 65520), ("a2", 0), ("a2", 65520)):
        data = _tune(_rand(15, 600), **({"want1": want} if half == "a1" else {"want2": want}))
        a = zlib.adler32(data)
        assert data[0] == 0 and (a & 0xFFFF if half == "a1" else a >> 16) == want
        out.append(case("adler: %s == %d" % (half, want), D.zstream(D.Deflate().fixed(list(data), final=True), data), data))
    return out


GROUPS = {"long_codes": long_codes, "header_forms": header_forms, "leniencies": leniencies, "zlib_headers": zlib_headers,
          "invalid_symbols": invalid_symbols, "ring_or_output": ring_or_output, "repeats": repeats,
          "flush_and_cap": flush_and_cap, "stored_blocks": stored_blocks, "stored_65535": stored_65535,
          "truncations": truncations, "trailing_junk": trailing_junk, "window_lengths": window_lengths,
          "adler_cases": adler_cases}


@functools.lru_cache(None)
def group(name):
    cases = GROUPS[name]()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)
