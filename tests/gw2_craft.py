"""Crafted baseline streams for the guess-write lanes' two-lookup write loop (k_gw_lane: a second
AC lookup of the same block per iteration when the block did not end and the reader's window still
holds more than 32 bits). Each case puts one kind of event where the second lookup meets it; the
error cases come in variants whose first block shifts the rest of the scan bit by bit, so the event
falls in either position whatever the reader's phase. Written symbol by symbol (tools/coefjpeg.py
only writes what coefficient arrays give: no invalid codes, no run past coefficient 63).

    streams() -> {name: bytes}, shared by tests/test_gw2_emu.py (CPU) and tests/test_gpu_gw2.py."""
import numpy as np

from tools import coefjpeg as CJ

QT = {0: [2] * 64, 1: [3] * 64}
STD = {("dc", 0): CJ.STD_DC_L, ("ac", 0): CJ.STD_AC_L, ("dc", 1): CJ.STD_DC_C, ("ac", 1): CJ.STD_AC_C}
EOB = ("ac", 0x00, 0, 0)
ZRL = ("ac", 0xF0, 0, 0)


def _mag(v):
    s = CJ._category(v)
    return s, (v if v >= 0 else v + (1 << s) - 1)


def dc(diff):
    s, e = _mag(diff)
    return ("dc", s, e, s)


def ac(run, v):
    s, e = _mag(v)
    return ("ac", (run << 4) | s, e, s)


def raw(bits, n):
    return ("raw", bits, n)


def _scan_start(j):
    p = 2
    while True:
        length = int.from_bytes(j[p + 2:p + 4], "big")
        if j[p + 1] == 0xDA:
            return p + 2 + length
        p += 2 + length


def stream(w, h, sampling, tabs, block_fn, cut=None, end=b"\xff\xd9"):
    """Headers as tools/coefjpeg.py writes them, then block_fn(n, ci)'s items for block n (component
    ci) in scan order: ("dc" | "ac", symbol, extra bits, n extra) or ("raw", bits, n). `cut`: keep
    that fraction of the entropy-coded bytes; `end`: what follows them."""
    comps = CJ.sampling_comps(sampling)
    head = CJ.write(w, h, comps, QT, CJ.empty_blocks(w, h, comps), huff=tabs)
    head = head[:_scan_start(head)]
    codes = {k: CJ._codes(*v) for k, v in tabs.items()}
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    nmcu = ((w + 8 * hmax - 1) // (8 * hmax)) * ((h + 8 * vmax - 1) // (8 * vmax))
    bw = CJ._Bits()
    n = 0
    for _ in range(nmcu):
        for ci, (hs, vs, _tq) in enumerate(comps):
            for _ in range(hs * vs):
                for it in block_fn(n, ci):
                    if it[0] == "raw":
                        bw.put(it[1], it[2])
                    else:
                        c, length = codes[(it[0], 0 if ci == 0 else 1)][it[1]]
                        bw.put(c, length)
                        bw.put(it[2], it[3])
                n += 1
    bw.flush()
    body = bytes(bw.out)
    if cut is not None:
        body = body[:int(len(body) * cut)]
        while body.endswith(b"\xff"):  # (never half a stuffed pair: `end` decides how the data ends)
            body = body[:-1]
    return head + body + end


def _fat(rng, lo=8, hi=24, size=5):
    """A valid block of lo..hi-1 coefficients of up to `size` magnitude bits, then EOB."""
    out = [dc(int(rng.integers(-40, 41)))]
    for _ in range(int(rng.integers(lo, hi))):
        v = int(rng.integers(1, 1 << size))
        out.append(ac(int(rng.integers(0, 2)), v if rng.integers(0, 2) else -v))
    return out + [EOB]


def _shifted(rng, k, bad_at, bad_block):
    """Fat valid blocks; block 0's DC difference has k + 1 magnitude bits (a k-bit shift of all that
    follows between variants); block `bad_at` is bad_block."""
    def fn(n, ci):
        if n == bad_at:
            return bad_block
        b = _fat(rng)
        if n == 0:
            b[0] = dc(1 << k)
        return b
    return fn


def streams():
    out = {}
    rng = np.random.default_rng(20260)
    # 1. 16-bit AC codes with 10 magnitude bits: 26 bits a lookup, the second is mostly refused for bits
    ac26 = CJ.skewed_table([0x00, 0x01, 0x02, 0x03, 0x11, 0xF0, 0x0A], short=2)
    assert CJ._codes(*ac26)[0x0A][1] == 16
    t26 = {("dc", 0): CJ.STD_DC_L, ("ac", 0): ac26, ("dc", 1): CJ.STD_DC_C, ("ac", 1): ac26}

    def long26(n, ci):
        vals = rng.integers(512, 1024, 3 + n % 13) * rng.choice([-1, 1], 3 + n % 13)
        return [dc(int(rng.integers(-9, 10)))] + [ac(0, int(v)) for v in vals] + [EOB]
    out["long26_420_128"] = stream(128, 128, "420", t26, long26)

    # 2. DC, one short AC code, EOB: the pair (code, EOB) is the second lookup and ends the block
    def short_eob(n, ci):
        return [dc(int(rng.integers(-3, 4))), ac(0, 1 if n % 3 else -1), EOB]
    out["short_eob_420_256"] = stream(256, 256, "420", STD, short_eob)

    # 3. all 63 AC coefficients, no EOB: the cursor reaches 64 in either position
    def full63(n, ci):
        out_ = [dc(int(rng.integers(-20, 21)))]
        for _ in range(63):
            v = int(rng.integers(1, 8))
            out_.append(ac(0, v if rng.integers(0, 2) else -v))
        return out_
    out["full63_444_96"] = stream(96, 96, "444", STD, full63)
    out["full63_gray_64"] = stream(64, 64, "gray", STD, full63)

    for k in range(8):
        few = [ac(0, 1)] * (k % 4)
        # 4. a ZRL run that passes coefficient 63 (the fourth ZRL: 1 + k % 4 + 64 > 64)
        out[f"zrl_past63_420_64_v{k}"] = stream(64, 64, "420", STD, _shifted(rng, k, 60, [dc(3)] + few + [ZRL] * 4))
        # 5. an invalid code (sixteen 1 bits: no Annex K code is all ones)
        out[f"invalid_420_64_v{k}"] = stream(64, 64, "420", STD, _shifted(rng, k, 57, [dc(-2)] + few + [ac(0, 5), raw(0xFFFF, 16)]))
    for k in range(4):
        # 7. data that stops mid-block: at the end of the file behind a lone FF (NanoJPEG's syntax
        # error at that byte: the lanes' error-byte bounds, the CHK instance), at a bad marker, and
        # at an early EOI (the rest is read from the 0xFF padding)
        cut = 0.55 + 0.1 * k
        out[f"cut_ff_420_64_v{k}"] = stream(64, 64, "420", STD, _shifted(rng, k, -1, None), cut=cut, end=b"\xff")
        out[f"cut_marker_420_64_v{k}"] = stream(64, 64, "420", STD, _shifted(rng, k, -1, None), cut=cut, end=b"\xff\x01\xff\xd9")
        out[f"cut_eoi_420_64_v{k}"] = stream(64, 64, "420", STD, _shifted(rng, k, -1, None), cut=cut)

    # 6. codes longer than the 10-bit AC window in the second position: a short code first, then
    # 15- / 16-bit ones (the pool) ...
    syms = [0x01, 0x00, 0x02, 0x03, 0x11, 0x12, 0x21, 0xF0, 0x04]
    acp = CJ.skewed_table(syms, short=2)
    tp = {("dc", 0): CJ.STD_DC_L, ("ac", 0): acp, ("dc", 1): CJ.STD_DC_C, ("ac", 1): acp}

    def pool(n, ci):
        out_ = [dc(int(rng.integers(-30, 31)))]
        for _ in range(int(rng.integers(4, 13))):
            s = syms[int(rng.integers(0, len(syms)))]
            if s in (0x00, 0xF0):
                s = 0x01
            v = int(rng.integers(1 << ((s & 15) - 1), 1 << (s & 15)))
            out_.append(ac(s >> 4, v if rng.integers(0, 2) else -v))
        return out_ + [EOB]
    out["pool_420_128"] = stream(128, 128, "420", tp, pool)
    # ... and every AC symbol but EOB at 12 bits, more 16-bit windows than the pool holds (the
    # canonical walk)
    others = sorted({(r << 4) | s for r in range(16) for s in range(1, 11)} | {0xF0})
    acs = ([1] + [0] * 10 + [len(others)] + [0] * 4, [0x00] + others)
    ts = {("dc", 0): CJ.STD_DC_L, ("ac", 0): acs, ("dc", 1): CJ.STD_DC_C, ("ac", 1): acs}

    def search(n, ci):
        out_ = [dc(int(rng.integers(-30, 31)))]
        for _ in range(int(rng.integers(3, 11))):
            v = int(rng.integers(1, 16))
            out_.append(ac(int(rng.integers(0, 3)), v if rng.integers(0, 2) else -v))
        return out_ + [EOB]
    out["search_420_96"] = stream(96, 96, "420", ts, search)
    return out


ERRORS = ("zrl_past63", "invalid", "cut_")  # name prefixes of the streams NanoJPEG refuses
