"""The token-level deflate reader (tests/deflate_read.py) against zlib and the crafted corpus: the
tokens it reads, re-applied, are what zlib inflates; it refuses what RFC 1951 forbids; and its
cost helpers agree with zlib's own (optimal) trees, which is what lets `audit` hold the GPU
writers' code lengths to them."""
import random
import zlib

import numpy as np
import pytest

import deflate_craft as D
import deflate_read as R
import inflate_corpus as IC


def _inputs():
    rng = np.random.default_rng(11)
    text = (b"the quick brown fox jumps over the lazy dog; " * 40)[:1500]
    skew = rng.choice(np.arange(256), 40000, p=np.r_[[0.5, 0.25, 0.125], np.full(253, 0.125 / 253)]).astype(np.uint8).tobytes()
    noise = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    big = (rng.integers(0, 64, 400000, dtype=np.uint8) // np.repeat(rng.integers(1, 9, 4000), 100)).astype(np.uint8).tobytes()
    return {"empty": b"", "one": b"\0", "text": text, "skew": skew, "noise": noise, "zeros": bytes(70000), "multi-block": big}


INPUTS = _inputs()


def _compress(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("name", list(INPUTS))
@pytest.mark.parametrize("how", ["1", "6", "9", "fixed", "stored"])
def test_reads_zlib(name, how):
    data = INPUTS[name]
    z = _compress(data, 0, zlib.Z_DEFAULT_STRATEGY) if how == "stored" else \
        _compress(data, 6, zlib.Z_FIXED) if how == "fixed" else _compress(data, int(how))
    blocks = R.read_zlib(z)
    assert D.apply(R.tokens(blocks)) == zlib.decompress(z) == data
    assert blocks[-1].final and blocks[0].bits[0] == 0 and blocks[0].out[0] == 0
    for a, b in zip(blocks, blocks[1:]):
        assert a.bits[1] <= b.bits[0] < a.bits[1] + 8 and a.out[1] == b.out[0]  # (a stored block aligns)
    assert blocks[-1].out[1] == len(data)
    want = {"stored": {R.STORED}, "fixed": {R.FIXED}}.get(how)
    if want and data and (how, name) != ("fixed", "noise"):  # (zlib stores what a fixed block would inflate)
        assert {b.type for b in blocks} == want
    if name == "multi-block" and how in "169":
        assert len(blocks) > 1 and all(b.type == R.DYNAMIC for b in blocks)
    if name == "zeros" and how != "stored":
        assert any(t == (258, 1) for t in R.tokens(blocks))


def _padded(hist, lens):
    """Counts with 1 for every symbol that has a code and does not occur (zlib forces two distance codes)."""
    lens = list(lens) + [0] * (len(hist) - len(lens))
    return [c or (1 if l else 0) for c, l in zip(hist, lens)], lens


@pytest.mark.parametrize("name", ["skew", "zeros", "multi-block"])  # (the inputs zlib codes with dynamic blocks)
@pytest.mark.parametrize("level", [1, 6, 9])
def test_zlib_trees_cost_the_optimum(name, level):
    """zlib's dynamic trees are Huffman's where no length limit is met: sum count x length equals
    huffman_cost (and package_merge_cost, which has nothing to limit) for all three codes."""
    seen = 0
    for b in R.read_zlib(_compress(INPUTS[name], level)):
        if b.type != R.DYNAMIC:
            continue
        hl, hd = R.histograms(b)
        hc = [0] * 19
        for s, _ in b.cl_syms:
            hc[s] += 1
        for hist, lens, limit in ((hl, b.ll_lens, 15), (hd, b.d_lens, 15), (hc, b.cl_lens, 7)):
            hist, lens = _padded(hist, lens)
            assert all((c > 0) == (l > 0) for c, l in zip(hist, lens))
            cost, depth = R.huffman_cost(hist)
            if depth <= limit:
                assert sum(c * l for c, l in zip(hist, lens)) == cost == R.package_merge_cost(hist, limit)
                seen += 1
    assert seen >= 2  # (the skewed input's literal/length tree may be deeper than 15)


@pytest.mark.parametrize("g", [g for g in IC.GROUPS if any(c.full is not None and not c.lenient for c in IC.group(g))])
def test_reads_the_crafted_corpus(g):
    n = 0
    for c in IC.group(g):
        if c.full is None or c.lenient:
            continue
        blocks = R.read_zlib(c.z, junk_ok=g == "trailing_junk")
        assert D.apply(R.tokens(blocks)) == c.full == zlib.decompressobj().decompress(c.z), c.name
        n += 1
    assert n


@pytest.mark.parametrize("g", ["header_forms", "invalid_symbols", "stored_blocks", "truncations"])
def test_refuses_what_the_rfc_forbids(g):
    n = 0
    for c in IC.group(g):
        if c.full is not None:
            continue
        with pytest.raises(R.DeflateError):
            R.read_zlib(c.z)
        n += 1
    assert n


def test_refuses_lenient_codes_and_zlib_framing():
    for c in IC.group("leniencies") + IC.group("zlib_headers") + IC.group("adler_cases"):
        if c.full is None or c.lenient:
            with pytest.raises(R.DeflateError):
                R.read_zlib(c.z)


def test_block_fields():
    """What read reports of a crafted block is what the writer was told."""
    ll = [0] * 270
    ll[0], ll[256], ll[257] = 1, 2, 2
    dl = [0, 0, 0, 0, 0, 0, 1, 1]
    syms = D.plain_cl(ll[:258]) + [(18, 7), (1, 0), (1, 0)]
    tok = [0] * 10 + [(3, 9), (3, 13), 0]
    d = D.Deflate().stored(b"ab").dynamic(tok, ll, dl, cl_syms=syms).fixed([7, (4, 1)], final=True)
    s, dyn, f = R.read(d.raw())
    assert (s.type, s.tokens, s.out, s.final) == (R.STORED, [97, 98], (0, 2), False)
    assert (dyn.hlit, dyn.hdist, dyn.ll_lens, dyn.d_lens, dyn.cl_syms, dyn.tokens) == (13, 7, ll, dl, syms, tok)
    assert dyn.hclen + 4 == max(k + 1 for k in range(19) if dyn.cl_lens[D.CL_ORDER[k]])
    assert dyn.out == (2, 2 + 17) and f.out == (19, 24) and f.final and f.tokens == [7, (4, 1)]
    assert s.bits[0] == 0 and dyn.bits[0] == s.bits[1] == 56 and f.bits[0] == dyn.bits[1] and f.bits[1] == d.b.nbits
    assert R.crossing([s, dyn, f], 16) == [(15, 3, 13)] and R.crossing([s, dyn, f], 12) == []


def test_cost_helpers():
    # Fibonacci weights: the deepest tree of all; limiting it costs something
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
    cost, depth = R.huffman_cost(fib)
    assert depth == len(fib) - 1 and cost == sum(f * min(len(fib) - i, len(fib) - 1) for i, f in enumerate(fib))
    assert R.package_merge_cost(fib, 19) == cost < R.package_merge_cost(fib, 15) < R.package_merge_cost(fib, 7)
    assert R.package_merge_cost([5] * 8, 3) == 120 and R.package_merge_cost([1, 0, 9], 15) == 10
    assert R.huffman_cost([0, 7]) == (7, 1) and R.huffman_cost([]) == (0, 0)
    # brute force over every complete code of up to 5 symbols within 3 bits
    rnd = random.Random(5)

    def codes(n, limit):
        def rec(prefix):
            if len(prefix) == n:
                if D.kraft(prefix) == 32768:
                    yield prefix
                return
            for l in range(1, limit + 1):
                yield from rec(prefix + [l])
        return list(rec([]))
    for _ in range(200):
        n = rnd.randint(2, 5)
        h = [rnd.randint(1, 30) for _ in range(n)]
        for limit in (3, 4):
            best = min(sum(c * l for c, l in zip(h, ls)) for ls in codes(n, limit))
            assert R.package_merge_cost(h, limit) == best, (h, limit)
        assert R.huffman_cost(h)[0] == R.package_merge_cost(h, 8)
    assert R.tight_cl([0] * 150 + [3] * 9 + [0, 0] + [5] * 3) == \
        [(18, 127), (18, 1), (3, 0), (16, 3), (3, 0), (3, 0), (0, 0), (0, 0), (5, 0), (5, 0), (5, 0)]


def test_audit_sees_a_wasteful_code():
    """audit on a stream of our own making: passes with optimal lengths and tight runs, fails with a
    phantom symbol, a longer-than-needed code, or loose runs."""
    data = bytes([0] * 40 + [1] * 20 + [2] * 10 + [3] * 10)
    tok = list(data[:50]) + [(30, 50)]
    ll = [0] * 286
    ll[0], ll[1], ll[256], ll[D.len_sym(30)[0]] = 1, 2, 3, 3
    dl = [0] * 30
    dl[0], dl[1], dl[D.dist_sym(50)[0]] = 2, 2, 1
    hd = D.dist_sym(50)[0] + 1

    def stream(ll, dl, cl_syms=None, hlit=None):
        n = max(257, max(s for s, l in enumerate(ll) if l) + 1) if hlit is None else hlit
        lens = ll[:n] + dl[:hd]
        d = D.Deflate().dynamic(tok, ll[:n], dl[:hd], final=True, cl_syms=R.tight_cl(lens) if cl_syms is None else cl_syms)
        return R.read(d.raw())
    data = D.apply(tok)
    # the default code-length code of the crafter is flat, not optimal: check ll / d here
    st = R.audit_codes(stream(ll, dl)[0], codes=("ll", "d"))
    assert [s["ratio"] for s in st] == [1.0, 1.0]
    bad = list(ll)
    bad[0], bad[1], bad[256], bad[D.len_sym(30)[0]] = 2, 2, 2, 2  # complete, not optimal
    with pytest.raises(AssertionError):
        R.audit_codes(stream(bad, dl)[0], codes=("ll", "d"))
    ph = list(ll)
    ph[256], ph[5] = 4, 4  # a code for a literal that never occurs
    with pytest.raises(AssertionError):
        R.audit_codes(stream(ph, dl)[0], codes=("ll", "d"))
    with pytest.raises(AssertionError):
        R.audit_header(stream(ll, dl, hlit=286)[0])  # trailing zero lengths
    with pytest.raises(AssertionError):
        R.audit_header(stream(ll, dl, cl_syms=D.plain_cl(ll[:280] + dl[:hd]), hlit=280)[0])
    R.audit_header(stream(ll, dl)[0])
    assert D.apply(R.tokens(stream(ll, dl))) == data
