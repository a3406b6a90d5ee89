"""A deflate writer that does what it is told (RFC 1950 / 1951), for streams no compressor emits:
chosen code lengths, HLIT / HDIST / HCLEN fields, code-length runs, stored blocks with any LEN /
NLEN, raw symbols and raw bits. Plain Python; nothing here uses the library under test, and zlib
only for the Adler-32 of the trailer. The expected output of a stream comes from its construction
(`apply`), never from a decoder.

Tokens of a block's data:
  int b                 literal byte b
  (len, dist)           a match
  ("ll", sym)           the block's literal/length code of `sym`, nothing else
  ("dc", len, code)     the length symbol (+ extra bits) of `len`, then distance code `code` alone
  ("bits", v, n)        n raw bits of v, LSB first
Only the first two have an output; `apply` refuses the others (those streams are invalid)."""
import struct
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # 288 codes: 286 and 287 have codes and no meaning
FIXED_D = [5] * 32                                      # 32 codes: 30 and 31 likewise


class Bits:
    """LSB-first bit writer."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0  # bits in acc

    def put(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)."""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """A Huffman code of n bits, most significant first."""
        self.put(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def nbits(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        """The bytes so far, the last one padded with zero bits."""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canon(lengths):
    """Canonical codes (RFC 1951 §3.2.2): per symbol (code, length), None for length 0. The lengths
    are taken as they are: over-subscribed and incomplete sets give the codes the rule gives."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((nxt[l] & ((1 << l) - 1), l))  # (an over-subscribed set overflows l bits: truncated)
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def len_sym(n):
    i = max(k for k in range(29) if LBASE[k] <= n) if n < 258 else 28
    return 257 + i, n - LBASE[i], LEXT[i]


def dist_sym(d):
    i = max(k for k in range(30) if DBASE[k] <= d)
    return i, d - DBASE[i], DEXT[i]


def apply(tokens):
    """The bytes a token list must inflate to."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        assert len(t) == 2 and not isinstance(t[0], str), "token %r has no output" % (t,)
        n, d = t
        assert 3 <= n <= 258 and 1 <= d <= len(out), t
        for _ in range(n):
            out.append(out[-d])
    return bytes(out)


def tokenize(data, min_len=3):
    """Greedy longest-match tokens of `data` (brute force: for short payloads)."""
    out, i, n = [], 0, len(data)
    while i < n:
        best, bd = 0, 0
        for d in range(1, min(i, 4096) + 1):
            k = 0
            while k < 258 and i + k < n and data[i + k - d] == data[i + k]:
                k += 1
            if k > best:
                best, bd = k, d
        if best >= min_len:
            out.append((best, bd))
            i += best
        else:
            out.append(data[i])
            i += 1
    return out


def plain_cl(lengths):
    """Code-length symbols without runs: one symbol 0..15 per length."""
    return [(l, 0) for l in lengths]


def expand_cl(syms):
    """The lengths a list of code-length symbols (sym, extra) stands for."""
    out = []
    for s, x in syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def complete_lengths(used, n=19):
    """Lengths of a complete code over the symbols in `used` (at least two: a second one is added)."""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used + [0 if used[0] else 1]))
    k = (len(used) - 1).bit_length()
    short = (1 << k) - len(used)  # that many codes of k - 1 bits, the rest k bits
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    assert kraft(lens) == 32768 and max(lens) <= 7
    return lens


class Deflate:
    """A raw deflate stream, block by block."""

    def __init__(self):
        self.b = Bits()

    def stored(self, data=b"", final=False, length=None, nlen=None):
        """LEN = `length` (default len(data)), NLEN = `nlen` (default its complement), then `data`."""
        n = len(data) if length is None else length
        self.b.put(1 if final else 0, 1)
        self.b.put(0, 2)
        self.b.align()
        self.b.put(n, 16)
        self.b.put(n ^ 0xFFFF if nlen is None else nlen, 16)
        for c in data:
            self.b.put(c, 8)
        return self

    def _data(self, tokens, ll, dc, eob):
        b = self.b
        for t in tokens:
            if isinstance(t, int):
                b.code(*ll[t])
            elif t[0] == "ll":
                b.code(*ll[t[1]])
            elif t[0] == "bits":
                b.put(t[1], t[2])
            elif t[0] == "dc":
                s, x, nx = len_sym(t[1])
                b.code(*ll[s])
                b.put(x, nx)
                b.code(*dc[t[2]])
            else:
                s, x, nx = len_sym(t[0])
                b.code(*ll[s])
                b.put(x, nx)
                s, x, nx = dist_sym(t[1])
                b.code(*dc[s])
                b.put(x, nx)
        if eob:
            b.code(*ll[256])

    def fixed(self, tokens=(), final=False, eob=True):
        self.b.put(1 if final else 0, 1)
        self.b.put(1, 2)
        self._data(tokens, canon(FIXED_LL), canon(FIXED_D), eob)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, hlit=None, hdist=None, cl_syms=None, cl_lens=None, hclen=None,
                eob=True, header_only=False):
        """ll_lens / d_lens: the code lengths the data is written with. The header says what the
        caller chooses: hlit / hdist are the 5-bit fields (default len - 257 / len - 1), cl_syms the
        code-length symbols as (symbol, extra bits value) (default one symbol per length), cl_lens
        the 19 lengths of the code-length code (default a complete code over the symbols used),
        hclen the count of them written (default up to the last non-zero one in the RFC's order)."""
        b = self.b
        syms = plain_cl(list(ll_lens) + list(d_lens)) if cl_syms is None else cl_syms
        cl = complete_lengths([s for s, _ in syms]) if cl_lens is None else list(cl_lens)
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl[CL_ORDER[k]]])
        b.put(1 if final else 0, 1)
        b.put(2, 2)
        b.put(len(ll_lens) - 257 if hlit is None else hlit, 5)
        b.put(len(d_lens) - 1 if hdist is None else hdist, 5)
        b.put(hclen - 4, 4)
        for k in range(hclen):
            b.put(cl[CL_ORDER[k]], 3)
        cc = canon(cl)
        for s, x in syms:
            b.code(*cc[s])
            if s >= 16:
                b.put(x, {16: 2, 17: 3, 18: 7}[s])
        if not header_only:
            self._data(tokens, canon(ll_lens), canon(d_lens), eob)
        return self

    def raw(self):
        return self.b.bytes()


def zwrap(deflate, data, cmf=0x78, flg=None, adler=None):
    """A zlib stream: CMF / FLG (FLG default: level bits 2 and the check bits that make the pair a
    multiple of 31), the deflate bytes, the Adler-32 of `data` (or the `adler` given)."""
    if flg is None:
        flg = 0x80
        flg += (31 - (cmf * 256 + flg) % 31) % 31
    a = zlib.adler32(data) & 0xFFFFFFFF if adler is None else adler
    return bytes([cmf, flg]) + deflate + struct.pack(">I", a)


def zstream(d, data, **kw):
    return zwrap(d.raw() if isinstance(d, Deflate) else d, data, **kw)


def stretch(tokens, n):
    """A zlib stream of exactly n bytes for `tokens`: empty fixed blocks (10 bits each) and empty
    stored blocks in front of one final fixed block."""
    body = Deflate().fixed(tokens, final=True).b.nbits
    for s in range(0, 4):
        for f in range(0, 8 * n):
            bits = 10 * f
            for _ in range(s):
                bits = (bits + 3 + 7) // 8 * 8 + 32
            total = 2 + (bits + body + 7) // 8 + 4
            if total > n:
                break
            if total == n:
                d = Deflate()
                for _ in range(f):
                    d.fixed()
                for _ in range(s):
                    d.stored()
                d.fixed(tokens, final=True)
                z = zstream(d, apply(tokens))
                assert len(z) == n
                return z
    raise ValueError("no stretch of %d bits to %d bytes" % (body, n))


def png_of(z, width, split=0):
    """A one-row 8-bit grey PNG around the zlib stream z: `width` + 1 filtered bytes, the first of
    them the filter type (0: the others are the pixels as they are)."""
    import pngread_util as R
    return R.wrap(width, 1, 8, 0, z, split=split)
