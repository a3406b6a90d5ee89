"""Crafted JPEG encoder inputs and a stream analyser -- TEST HELPER, not a test.

The GPU encoder's entropy stage (k_enc_run, k_stuff_count_b / k_stuff_write_b) has states that
smooth images never reach: 10-bit amplitudes behind 16-bit codes, category-11 DC differences,
three ZRLs in a row, a lone coefficient 63, FF bytes side by side on a stuffing lane's or
workgroup's edge. The generators below reach them from pixels; `analyse` reads a file the oracle
wrote and reports which states its stream holds, so the tests can assert that the inputs reach
them (conditions on the inputs: they never read the code under test).

numpy only, deterministic from the parameters: no pixel fixtures are committed. Every generator
returns an (h, w, comps) uint8 array (comps 3 or 4; the fourth channel is filler the encoders skip).
"""
from __future__ import annotations

import numpy as np

# natural (row-major) index of each zig-zag position (JPEG figure A.6)
DEZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                     13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
                     52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# colour axes: pixel = mid + a * axis drives one of Y / Cb / Cr (and, for the chroma axes, some Y)
VARIANTS = ("grey", "by", "rc")
_LO_HI = {"grey": ((0, 0, 0), (255, 255, 255)),      # Y -128 .. 127
          "by": ((255, 255, 0), (0, 0, 255)),        # yellow / blue: Cb -127.5 .. 127.5
          "rc": ((0, 255, 255), (255, 0, 0))}        # cyan / red:    Cr -127.5 .. 127.5
_AXIS = {"grey": (1, 1, 1), "by": (-1, -1, 1), "rc": (1, -1, -1)}


def basis(k: int) -> np.ndarray:
    """The 8x8 DCT basis function of zig-zag position k, values in -1 .. 1 ([y, x])."""
    v, u = divmod(int(DEZIGZAG[k]), 8)
    i = np.arange(8)
    return np.outer(np.cos((2 * i + 1) * v * np.pi / 16), np.cos((2 * i + 1) * u * np.pi / 16))


def _with_comps(rgb: np.ndarray, comps: int) -> np.ndarray:
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if comps == 3:
        return rgb
    h, w, _ = rgb.shape
    out = np.empty((h, w, 4), np.uint8)
    out[:, :, :3] = rgb
    out[:, :, 3] = (np.arange(w, dtype=np.uint8)[None, :] * 7 + np.arange(h, dtype=np.uint8)[:, None] * 13) | 1
    return out


def _two_level(mask: np.ndarray, variant: str) -> np.ndarray:
    lo, hi = _LO_HI[variant]
    return np.where(mask[:, :, None], np.array(hi, np.uint8), np.array(lo, np.uint8))


def _axis_blocks(vals: np.ndarray, variant: str) -> np.ndarray:
    """float (h, w) offsets from mid grey along the variant's colour axis -> rounded RGB."""
    ax = np.array(_AXIS[variant], np.float64)
    return np.clip(np.rint(128.0 + vals[:, :, None] * ax), 0, 255).astype(np.uint8)


def _lay_out(blocks, per_row: int, mirror: bool = True) -> np.ndarray:
    """Blocks (equal squares, (s, s, 3)) in raster order, rows of per_row, the last row padded with
    mid grey; with mirror, the same list reversed below, so every block meets another neighbour."""
    grey = np.full_like(blocks[0], 128)
    rows = []
    for lst in ([blocks, blocks[::-1]] if mirror else [blocks]):
        for i in range(0, len(lst), per_row):
            r = list(lst[i:i + per_row])
            r += [grey] * (per_row - len(r))
            rows.append(np.concatenate(r, axis=1))
    return np.concatenate(rows, axis=0)


def sign_block_list(variant: str = "grey", scale: int = 1, amp=None, ks=range(64)) -> list:
    """For each zig-zag position in ks and both signs, a two-level block following sign(basis(k))
    (k = 0: flat blocks). amp None: the variant's extreme colours (0 / 255 levels, the largest
    amplitude pixels can give coefficient k and the largest DC swing); else 128 +- amp along the
    variant's axis (other amplitude bits: the FF search's knob)."""
    blocks = []
    for k in ks:
        b = basis(k)
        for s in (1, -1):
            m = np.kron(s * b > 0 if k else np.full((8, 8), s > 0), np.ones((scale, scale), bool))
            blocks.append(_two_level(m, variant) if amp is None else
                          _axis_blocks(np.where(m, float(amp), -float(amp)), variant))
    return blocks


def sign_blocks(variant: str = "grey", scale: int = 1, comps: int = 3, width: int = 1024, amp=None,
                ks=range(64)) -> np.ndarray:
    """sign_block_list as one strip of blocks `width` pixels wide (several rows of blocks when
    they do not fit in one) and its reverse below: black / white neighbours everywhere. scale 2
    gives 16x16 blocks whose 2x2 means are the pattern: what the chroma units of 4:2:0 see."""
    return _with_comps(_lay_out(sign_block_list(variant, scale, amp, ks), width // (8 * scale)), comps)


# (k1, k2): two nonzero coefficients with exactly k2 - k1 - 1 zeros between them; the second of
# each triple of runs ends at coefficient 63
RUN_PAIRS = ((1, 17), (2, 19), (3, 21), (1, 33), (2, 35), (3, 37), (1, 49), (2, 51), (3, 53), (1, 63),
             (47, 63), (46, 63), (45, 63), (31, 63), (30, 63), (29, 63), (15, 63), (14, 63), (13, 63))


def single_coef_blocks(variant: str = "grey", amp: float = 60.0, comps: int = 3, width: int = 1024,
                       scale: int = 1) -> np.ndarray:
    """128 + amp * basis(k) along the variant's colour axis for k = 1 .. 63 (a zero run of k - 1
    before the only nonzero AC coefficient: every run 0 .. 62, up to three ZRLs, a lone
    coefficient 63 after a run of 62), a flat block, and the RUN_PAIRS blocks (amp * (basis(k1) +
    basis(k2)): runs of exactly 15, 16, 17, 31, 32, 33, 47, 48, 49 and 61 between two
    coefficients, and the same runs ending at coefficient 63). One strip and its reverse below.
    Along a chroma axis an offset a gives Cb (or Cr) = a and Y = -+0.772 a: luma and chroma units
    both see the pattern."""
    vals = [amp * basis(k) for k in range(1, 64)] + [np.zeros((8, 8))]
    for k1, k2 in RUN_PAIRS:
        vals.append(amp * (basis(k1) + basis(k2)))
    blocks = [_axis_blocks(np.kron(v, np.ones((scale, scale))), variant) for v in vals]
    return _with_comps(_lay_out(blocks, width // (8 * scale)), comps)


def dc_swing(w: int, h: int, sub: int = 444, variant: str = "grey", comps: int = 3, period: int = 1) -> np.ndarray:
    """Flat MCU-sized blocks alternating between the variant's two levels, every `period` MCUs in
    stream order (raster over MCUs, so with an odd number of MCUs per row the swing also falls
    between a row's last unit and the next row's first): every unit's DC differs from its
    predecessor's by the largest step its component can take, wherever the run boundaries are."""
    ms = 16 if sub == 420 else 8
    mbw, mbh = (w + ms - 1) // ms, (h + ms - 1) // ms
    m = (np.arange(mbw * mbh).reshape(mbh, mbw) // period) & 1
    mask = np.kron(m, np.ones((ms, ms), int))[:h, :w] > 0
    return _with_comps(_two_level(mask, variant), comps)


def noise01(seed: int, w: int, h: int, comps: int = 3) -> np.ndarray:
    """Independent 0 / 255 per channel: the longest streams pixels can give."""
    rng = np.random.RandomState(seed)
    return _with_comps((rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8), comps)


def edge_contrast(w: int, h: int, comps: int = 3) -> np.ndarray:
    """A smooth image whose last column and last row are the inverse of their neighbours: the
    encoders replicate the last column / row into the partial MCUs, so a clamp that is off by one
    (min(x, w - 1), min(y, h - 1)) changes bytes."""
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([(40 + 3 * x + y) % 200, (90 + x + 2 * y) % 180, (20 + 2 * x + 3 * y) % 220], axis=2)
    rgb = (rgb // 4 + 60).astype(np.uint8)  # smooth: 60 .. 115
    if w > 1:
        rgb[:, w - 1] = 255 - rgb[:, w - 2]
    if h > 1:
        rgb[h - 1, :] = 255 - rgb[h - 2, :]
    return _with_comps(rgb, comps)


def flat(w: int, h: int, rgb=(128, 128, 128), comps: int = 3) -> np.ndarray:
    return _with_comps(np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)), comps)


def ff_placed(sub: int, variant: str, amp: int, noise_mcus: int, fillers: int, seed: int = 11,
              comps: int = 3, width: int = 1024) -> np.ndarray:
    """The FF search's layout, MCUs in stream order: noise_mcus MCUs of 0 / 255 noise (about 300
    stream bytes each at quantiser 1), `fillers` mid-grey MCUs (14 bits each at 4:4:4, 32 at
    4:2:0: they move what follows through the byte phases and lane positions), then
    sign_block_list(variant, amp) and its reverse. The search picks the parameters so that FF
    bytes the sign blocks make fall where it wants them."""
    scale = 2 if sub == 420 else 1
    ms = 8 * scale
    rng = np.random.RandomState(seed)
    noise = [(rng.randint(0, 2, (ms, ms, 3)) * 255).astype(np.uint8) for _ in range(noise_mcus)]
    grey = [np.full((ms, ms, 3), 128, np.uint8)] * fillers
    sb = sign_block_list(variant, scale, amp)
    return _with_comps(_lay_out(noise + grey + sb + sb[::-1], width // ms, mirror=False), comps)


# ------------------------------------------------------------------------------- analyser
def scan_bytes(jpeg: bytes) -> np.ndarray:
    """The entropy-coded segment of a one-scan baseline file with the stuffing zeros removed:
    the bytes the GPU encoder holds before k_stuff_*."""
    d = bytes(jpeg)
    i = 2
    while True:
        assert d[i] == 0xFF, "marker expected"
        m, n = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        i += 2 + n
        if m == 0xDA:
            break
    assert d[-2:] == b"\xff\xd9"
    a = np.frombuffer(d[i:-2], np.uint8)
    stuffed = np.zeros(len(a), bool)
    stuffed[1:] = (a[:-1] == 0xFF) & (a[1:] == 0)
    return a[~stuffed]


def _sof(jpeg: bytes):
    i = 2
    while jpeg[i + 1] != 0xC0:
        i += 2 + ((jpeg[i + 2] << 8) | jpeg[i + 3])
    h, w = (jpeg[i + 5] << 8) | jpeg[i + 6], (jpeg[i + 7] << 8) | jpeg[i + 8]
    return w, h, 420 if jpeg[i + 11] == 0x22 else 444


def _category(v: np.ndarray) -> np.ndarray:
    a = np.abs(v.astype(np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def analyse(jpeg: bytes, decode_trace) -> dict:
    """States of the entropy coder that the file's stream holds. decode_trace is the oracle's
    (it returns quantised coefficients in natural order and absolute DCs, both per data unit in
    stream order: reordered to zig-zag and differenced per component here)."""
    code, coef, dc = decode_trace(jpeg)
    assert code == 0, code
    w, h, sub = _sof(jpeg)
    comp_of = np.array([0, 0, 0, 0, 1, 2] if sub == 420 else [0, 1, 2])
    comp = comp_of[np.arange(len(dc)) % len(comp_of)]
    zz = coef[:, DEZIGZAG].astype(np.int64)
    zz[:, 0] = 0
    res = {"w": w, "h": h, "sub": sub, "units": int(len(dc)), "comp": comp}
    cat = _category(zz)
    res["ac_cat"] = {"luma": int(cat[comp == 0].max(initial=0)), "chroma": int(cat[comp != 0].max(initial=0))}
    res["dc_diff"] = {}
    diffs = np.zeros(len(dc), np.int64)  # per unit, stream order
    for c, name in enumerate(("Y", "Cb", "Cr")):
        d = np.diff(np.concatenate([[0], dc[comp == c].astype(np.int64)]))
        diffs[comp == c] = d
        res["dc_diff"][name] = int(np.abs(d).max(initial=0))
    res["dc_diffs"] = diffs
    # every nonzero AC coefficient with the zero run before it (from the unit's previous nonzero
    # coefficient, or from the DC)
    uu, kk = np.nonzero(zz)
    first = np.ones(len(uu), bool)
    first[1:] = uu[1:] != uu[:-1]
    prev = np.zeros(len(uu), np.int64)
    prev[1:] = np.where(first[1:], 0, kk[:-1])
    run = kk - prev - 1
    last = np.ones(len(uu), bool)
    last[:-1] = first[1:]
    res.update(runs=set(int(x) for x in run), pair_runs=set(int(x) for x in run[~first]),
               runs_by_class={"luma": set(int(x) for x in run[comp[uu] == 0]),
                              "chroma": set(int(x) for x in run[comp[uu] != 0])},
               zrl_max=int(run.max(initial=0)) >> 4, coef63=int((last & (kk == 63)).sum()),
               lone63=int((first & last & (kk == 63)).sum()))
    s = scan_bytes(jpeg)
    ff = np.nonzero(s == 0xFF)[0]
    longest, cur, before = 0, 0, -2
    for p in ff:
        cur = cur + 1 if p == before + 1 else 1
        longest = max(longest, cur)
        before = p
    pair_first = ff[:-1][np.diff(ff) == 1] if len(ff) > 1 else ff[:0]  # position of the first FF of each pair
    res.update(ff_count=int(len(ff)), ff_longest=int(longest), ff_mod16=set(int(x) for x in ff % 16),
               ff_mod4096=set(int(x) for x in ff % 4096),
               ff_pair_16=bool(((pair_first % 16) == 15).any()),
               ff_pair_4096=bool(((pair_first % 4096) == 4095).any()),
               ff_first_of_chunk=bool(((ff % 16) == 0).any()), ff_last_of_chunk=bool(((ff % 16) == 15).any()),
               stream_len=int(len(s)), len_mod16=int(len(s) % 16), stuffed_len=int(len(s) + len(ff)),
               file_len=len(jpeg))
    bits = _stream_bits(jpeg, zz, diffs, comp, uu, kk, run)
    assert (bits + 7) // 8 == len(s), "the trace and the scan bytes disagree"
    res.update(stream_bits=bits, bits_mod32=bits % 32)
    return res


def _dht(jpeg: bytes) -> dict:
    """{(class, id): code length of each symbol} from the file's DHT segments."""
    out, i = {}, 2
    while jpeg[i + 1] != 0xDA:
        m, n = jpeg[i + 1], (jpeg[i + 2] << 8) | jpeg[i + 3]
        if m == 0xC4:
            p, end = i + 4, i + 2 + n
            while p < end:
                tc, counts = jpeg[p], jpeg[p + 1:p + 17]
                p += 17
                ln = np.zeros(256, np.int64)
                for L, c in enumerate(counts, 1):
                    for _ in range(c):
                        ln[jpeg[p]] = L
                        p += 1
                out[(tc >> 4, tc & 15)] = ln
        i += 2 + n
    return out


def _stream_bits(jpeg: bytes, zz, diffs, comp, uu, kk, run) -> int:
    """Bits of the entropy-coded stream before the final pad, from the trace and the file's own
    Huffman tables (the encoder's rule: DC diff; per nonzero AC a ZRL per 16 zeros, the (run, size)
    code and the amplitude; EOB unless coefficient 63 is nonzero)."""
    ln = _dht(jpeg)
    chroma = (comp != 0).astype(np.int64)
    dcl = np.stack([ln[(0, 0)], ln[(0, 1)]])
    acl = np.stack([ln[(1, 0)], ln[(1, 1)]])
    n = _category(diffs)
    bits = int((dcl[chroma, n] + n).sum())
    n = _category(zz[uu, kk])
    t = chroma[uu]
    bits += int(((run >> 4) * acl[t, 0xF0] + acl[t, ((run & 15) << 4) | n] + n).sum())
    bits += int(acl[chroma, 0][zz[:, 63] == 0].sum())
    return bits


# --------------------------------------------------------------------------- the crafted set
# What search_ff() found (run this file to repeat it): ff_placed parameters (quality, variant,
# amp, noise_mcus, fillers) whose stream holds an FF pair across a 16-byte stuffing lane's edge, one
# across a 4096-byte workgroup's edge, and three FF bytes in a row. Three is the most any stream of
# these tables can hold: a run of one bits is at most the 6 trailing ones of a code (FFBF), 10 of
# an amplitude and the 15 leading ones of the next code (FFFE), 31 bits, and a fourth FF needs 32.
FF_PLACED = {
    "tje": {"pair16": (3, "grey", 18, 0, 0), "pair4096": (3, "by", 64, 0, 2), "run3": (3, "rc", 100, 0, 2)},
    444: {"pair16": (100, "grey", 18, 0, 0), "pair4096": (100, "by", 64, 0, 2), "run3": (100, "rc", 100, 0, 2)},
    420: {"pair16": (100, "grey", 4, 0, 0), "pair4096": (100, "grey", 55, 0, 0), "run3": (100, "rc", 100, 0, 0)},
}
QUALITIES = {"tje": (1, 2, 3), 444: (100, 97, 90, 50, 1), 420: (100, 97, 90, 50, 1)}
FAMILIES = ("sign_blocks", "single_coef_blocks", "dc_swing", "noise01", "edge_contrast", "ff_placed")
NOISE_SMALL = (7, 256, 64)    # outgrows a fresh workspace's 64 KiB words buffer
NOISE_BIG = (8, 1024, 64)     # at quantiser 1 its file exceeds source + 64 KiB (4.7 bytes a pixel)


def crafted(kind, comps: int = 3) -> list:
    """The crafted inputs of one encoder ("tje", 444 or 420) as (family, name, pixels); the
    tests encode each at every quality of QUALITIES[kind]."""
    sub = 420 if kind == 420 else 444
    scale = 2 if sub == 420 else 1
    out = []
    for v in VARIANTS:
        out.append(("sign_blocks", f"sign_{v}", sign_blocks(v, scale, comps)))
    for v in VARIANTS:
        out.append(("single_coef_blocks", f"single_{v}", single_coef_blocks(v, comps=comps)))
    # 65 (33 at 4:2:0) MCUs a row: the second run of each row is a single MCU, and with an odd
    # count the swing also falls between a row's last unit and the next row's first
    w = 528 if sub == 420 else 520
    for v in VARIANTS:
        out.append(("dc_swing", f"swing_{v}_{w}x33", dc_swing(w, 33, sub, v, comps)))
    out.append(("noise01", "noise_small", noise01(*NOISE_SMALL, comps=comps)))
    out.append(("noise01", "noise_big", noise01(*NOISE_BIG, comps=comps)))
    out.append(("edge_contrast", "edge_1023x33", edge_contrast(1023, 33, comps)))
    out.append(("edge_contrast", "edge_129x9", edge_contrast(129, 9, comps)))  # (a stream length of 15 mod 16)
    for goal, (_, v, amp, a, b) in FF_PLACED[kind].items():
        out.append(("ff_placed", f"ff_{goal}", ff_placed(sub, v, amp, a, b, comps=comps)))
    return out


def search_ff(kind, budget_s: float = 600.0, seed: int = 11) -> dict:
    """The seeded CPU search behind FF_PLACED: over the quantiser-1 qualities' sign blocks of
    every variant and amplitude, behind 0..3 noise MCUs and 0..7 grey fillers, for the three FF
    goals, with the oracle as the encoder. Minutes at the most; the tests use the literals."""
    import time
    from oracle import pyoracle as O

    sub = 420 if kind == 420 else 444
    found, t0 = {}, time.time()
    for q in ((3,) if kind == "tje" else (100, 97, 90)):
        for a in range(4):
            for b in range(8):
                for v in VARIANTS:
                    for amp in range(1, 129):
                        px = ff_placed(sub, v, amp, a, b, seed)
                        h, w, c = px.shape
                        jp = O.tje_encode(q, w, h, c, px.tobytes()) if kind == "tje" else \
                            O.jpeg_encode(q, sub, w, h, c, px.tobytes())
                        s = scan_bytes(jp)
                        ff = np.nonzero(s == 0xFF)[0]
                        d = np.diff(ff)
                        first = ff[:-1][d == 1]
                        hit = {"pair16": bool((first % 16 == 15).any()), "pair4096": bool((first % 4096 == 4095).any()),
                               "run3": bool(len(d) > 1 and ((d[:-1] == 1) & (d[1:] == 1)).any())}
                        for goal, ok in hit.items():
                            if ok:
                                found.setdefault(goal, (q, v, amp, a, b))
                        if len(found) == 3 or time.time() - t0 > budget_s:
                            return found
    return found


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for kind_ in ("tje", 444, 420):
        print(repr(kind_), search_ff(kind_))
