"""Radiance .hdr files built packet by packet for the GPU read (icx_hdr.hip), with expectations
that come from the build plan and a plain restatement of how the read locates its scanlines.

The read picks one of three ways to find where each scanline starts:
  mode 1  every row is a plain RGBE row at ds + 4*w*y: no 4-byte group aligned to the data start
          ds begins 1 1 1 (an old-style run marker), and no row begins 2 2 <128;
  mode 2  the occurrences of "2 2 w>>8 w&255" in [ds, n) (at most 8192) are sorted, and the first h
          of them chain: the first is at ds and each scanline, walked through its four run-length
          coded components, ends where the next begins. A walk gives up at a packet header
          16*w + 64 bytes or more past its scanline's first byte;
  mode 3  anything else: one lane replays the reference's loop.
Mode 3 decodes the same pixels, so only `HdrBatch.locate_stats()` can tell a linked file from one
that fell back. `predict` restates the rule in numpy; `window_refills` restates when the unpack
kernel reloads its 4096-byte window, so that a test can prove where a crafted packet lands.

`scanline` is the packet-level writer: ("run", count 1..127, value) is written as the code
128 + count and the value byte, ("lit", bytes of length 0..128) as the length and the bytes. Code 0
is the empty literal and code 128 the 128-byte literal; a run of 0 cannot be written, because the
reader takes the code 128 for that literal (decrunchHDR tests code > 128).

`cases()` is the table: each row names the edge it is built to reach and the mode it is meant to
take. Device addresses: a file is placed in its batch blob after `blob_offset` padding bytes, and
torch allocations are at least 256-byte aligned, so (blob_offset + pos) mod 16 is the device
address residue of file byte pos.
"""
import functools
import re
from dataclasses import dataclass, field

import numpy as np

import hdrutil as H

CAND_CAP = 8192   # scanline starts the link step sorts per image
WIN = 4096        # bytes of one unpack window
LONGEST = 129     # the longest packet: code 128 and 128 literal bytes
OK, MALFORMED, TRUNCATED = 0, 3, 4


# --------------------------------------------------------------------------- the writer
def scanline(w: int, comps, header=None):
    """comps: 4 packet lists (R, G, B, E). -> (the scanline's bytes, the RGBE row (w, 4) the plan means)."""
    assert len(comps) == 4
    out = bytearray(header if header is not None else (2, 2, w >> 8, w & 255))
    row = np.empty((w, 4), np.uint8)
    for c, packets in enumerate(comps):
        vals = bytearray()
        for p in packets:
            if p[0] == "run":
                _, cnt, v = p
                assert 1 <= cnt <= 127, "code 128 is the 128-byte literal: a run of 0 cannot be written"
                out.append(128 + cnt)
                out.append(v)
                vals += bytes((v,)) * cnt
            else:
                assert p[0] == "lit" and len(p[1]) <= 128
                out.append(len(p[1]))
                out += p[1]
                vals += p[1]
        assert len(vals) == w, (c, len(vals), w)
        row[:, c] = np.frombuffer(bytes(vals), np.uint8)
    return bytes(out), row


def runs(n: int, v: int):
    """n pixels of value v as runs of at most 127."""
    out = []
    while n > 0:
        k = min(n, 127)
        out.append(("run", k, v))
        n -= k
    return out


def val(k: int) -> int:
    """A byte in 3..252: never 1 or 2, so no planned value builds a marker or a start pattern."""
    return 3 + k % 250


def vals(k: int, n: int) -> bytes:
    return bytes(val(k + 7 * i) for i in range(n))


def run_row(w: int, y: int):
    """A scanline of four long runs whose values depend on y."""
    return scanline(w, [runs(w, val(11 * y + 3 * c)) for c in range(4)])


def flat_file(px: np.ndarray, trailing: bytes = b"") -> bytes:
    h, w, _ = px.shape
    return H.header(w, h) + np.ascontiguousarray(px, np.uint8).tobytes() + trailing


def flat_px(seed: int, w: int, h: int) -> np.ndarray:
    """Pixels with every byte in 3..252."""
    rng = np.random.default_rng(seed)
    return rng.integers(3, 253, size=(h, w, 4)).astype(np.uint8)


# --------------------------------------------------------------------------- the restated rules
def parse_header(f: bytes):
    """-> (w, h, ds), or None where the read stops with a header error."""
    n = len(f)
    if n < 10 or f[:10] != b"#?RADIANCE":
        return None
    i = f.find(b"\n\n", 11)  # both bytes are read after the byte that follows the magic
    if i < 0:
        return None
    pos = i + 2
    nl = f.find(b"\n", pos)
    if nl < 0 or nl - pos + 1 > 255:
        return None
    m = re.match(rb"-Y[ \t\n\v\f\r]*([+-]?\d+)[ \t\n\v\f\r]*\+X[ \t\n\v\f\r]*([+-]?\d+)", f[pos:nl + 1])
    if not m:
        return None
    h, w = int(m.group(1)), int(m.group(2))
    if h <= 0 or w <= 0 or h > 1 << 20 or w > 1 << 20 or h * w > 1 << 30:
        return None
    return w, h, nl + 1


def walk_row(f: bytes, start: int, w: int):
    """The packets of the new-style scanline whose 4-byte header is at `start`: yields
    (header position, code, pixels) and stops where the data stops making sense."""
    n, pos = len(f), start + 4
    for _ in range(4):
        j = 0
        while j < w:
            if pos >= n:
                return
            code = f[pos]
            px = code & 127 if code > 128 else code
            size = 2 if code > 128 else 1 + code
            if j + px > w or pos + size > n:
                return
            yield pos, code, px
            pos += size
            j += px


def scanline_end(f: bytes, start: int, w: int, cap: int = 0):
    """The byte after the scanline at `start`, or None: it overflows w, the file ends first, or
    (cap > 0) one of its packet headers is `cap` bytes or more past `start`."""
    total, end = 0, start + 4
    if end > len(f):
        return None
    for pos, code, px in walk_row(f, start, w):
        if cap and pos - start >= cap:
            return None
        total += px
        end = pos + (2 if code > 128 else 1 + code)
    return end if total == 4 * w else None


def pattern_positions(f: bytes, w: int, ds: int):
    """File offsets in [ds, n) where the 4 bytes 2 2 w>>8 w&255 stand."""
    d = np.frombuffer(f, np.uint8)[ds:]
    if not (8 <= w <= 0x7fff) or len(d) < 4:
        return []
    m = (d[:-3] == 2) & (d[1:-2] == 2) & (d[2:-1] == w >> 8) & (d[3:] == (w & 255))
    return (np.flatnonzero(m) + ds).tolist()


def aligned_marker(f: bytes, ds: int) -> bool:
    """Does a whole 4-byte group at ds + 4k begin 1 1 1?"""
    d = np.frombuffer(f, np.uint8)[ds:]
    g = d[:len(d) // 4 * 4].reshape(-1, 4)
    return bool(((g[:, 0] == 1) & (g[:, 1] == 1) & (g[:, 2] == 1)).any())


def rows_plain(f: bytes, w: int, h: int, ds: int) -> bool:
    """The flat check: the file holds h rows of 4*w bytes and none of them selects the new-style decoder."""
    if ds + 4 * w * h > len(f):
        return False
    if not (8 <= w <= 0x7fff):
        return True
    d = np.frombuffer(f, np.uint8)
    r = ds + 4 * w * np.arange(h, dtype=np.int64)
    return not bool(((d[r] == 2) & (d[r + 1] == 2) & (d[r + 2] < 128)).any())


def predict(f: bytes):
    """(mode, ncand) as icx_hdr_batch_locate_stats reports them for this file."""
    hd = parse_header(f)
    if hd is None:
        return 0, 0
    w, h, ds = hd
    starts = pattern_positions(f, w, ds)
    ncand = len(starts)
    if rows_plain(f, w, h, ds) and not aligned_marker(f, ds):
        return 1, ncand
    if h <= ncand <= CAND_CAP and starts[0] == ds:
        cap = 16 * w + 64
        first = starts[:h] + [None]
        if all(e is not None and (nxt is None or e == nxt)
               for e, nxt in ((scanline_end(f, first[y], w, cap), first[y + 1]) for y in range(h))):
            return 2, ncand
    return 3, ncand


def window_refills(f: bytes, row_start: int, addr_mod16: int):
    """(base, lim) of every window the unpack kernel loads for the scanline at row_start, when file
    byte 0 sits at a device address = addr_mod16 (mod 16). A window holds file bytes
    [base, base + 4096), base being the packet header's position rounded down to a 16-byte device
    address; it is reloaded at the first packet header past lim = base + 4096 - 129."""
    w = parse_header(f)[0]
    out, lim = [], -1
    for pos, _, _ in walk_row(f, row_start, w):
        if pos > lim:
            base = pos - ((addr_mod16 + pos) & 15)
            lim = base + WIN - LONGEST
            out.append((base, lim))
    return out


def scan_tail_start(f: bytes) -> int:
    """The scan gives each lane 16 positions from ds on and reads them as dwords while 24 bytes
    remain; the chunks after that are read byte by byte. -> the first such chunk's file offset."""
    _, _, ds = parse_header(f)
    n = len(f)
    m = max(0, -(-(n - 23 - ds) // 16))  # smallest m with ds + 16 m + 24 > n
    return ds + 16 * m


# --------------------------------------------------------------------------- the case table
@dataclass
class Case:
    name: str
    group: str
    file: bytes
    blob_offset: int
    status: int
    pixels: object      # RGBE (h, w, 4) the plan means, or None: the oracle's result stands
    mode: int           # the locate path the file is built for
    edge: str
    aux: dict = field(default_factory=dict)

    @property
    def dims(self):
        return parse_header(self.file)[:2]


PACKETS = {
    "lit128": lambda k: ("lit", vals(k, 128)),
    "lit1": lambda k: ("lit", vals(k, 1)),
    "code0": lambda k: ("lit", b""),
    "run127": lambda k: ("run", 127, val(k)),
    "run1": lambda k: ("run", 1, val(k)),
}
DELTAS = (-1, 0, 1, 2)


class _Row:
    """A scanline under construction: packets go to the current component, which closes at w pixels."""

    def __init__(self, w, start, addr0, seed):
        self.w, self.start, self.addr0, self.k = w, start, addr0, seed
        self.comps, self.c, self.j, self.pos = [[], [], [], []], 0, 0, start + 4

    def lim_at(self, pos):
        return pos - ((self.addr0 + pos) & 15) + WIN - LONGEST

    def emit(self, p):
        px = p[1] if p[0] == "run" else len(p[1])
        assert self.j + px <= self.w
        self.comps[self.c].append(p)
        self.pos += 2 if p[0] == "run" else 1 + len(p[1])
        self.j += px
        self.k += 1
        if self.j == self.w and self.c < 3:
            self.c, self.j = self.c + 1, 0

    def fill(self, filler, until):
        """Filler packets while until(pos) is false. One-pixel runs move 2 bytes; a 2-byte literal
        (3 bytes) first where the distance is odd."""
        while not until(self.pos):
            if filler == "zero":
                self.emit(("lit", b""))
            else:
                self.emit(("run", 1, val(self.k)))

    def fill_to(self, filler, target):
        if filler != "zero" and (target - self.pos) & 1:
            self.emit(("lit", vals(self.k, 2)))
        self.fill(filler, lambda pos: pos >= target)
        assert self.pos == target, (self.pos, target)

    def finish(self, min_len=0):
        for c in range(self.c, 4):
            self.comps[c] += runs(self.w - (self.j if c == self.c else 0), val(self.k + c))
        data, row = scanline(self.w, self.comps)
        if len(data) < min_len:  # empty literals in front of the last component
            self.comps[3] = [("lit", b"")] * (min_len - len(data)) + self.comps[3]
            data, row = scanline(self.w, self.comps)
        return data, row


def window_row(w, start, addr0, which, delta, packet, filler, seed, min_len=0):
    """A scanline at file offset `start` whose packet under test has its header `delta` bytes past
    the lim of the first (which = 1) or second window. -> (bytes, row, header position)."""
    r = _Row(w, start, addr0, seed)
    lim = r.lim_at(r.pos)
    if which == 2:
        r.fill(filler, lambda pos: pos > lim)  # this header reloads the window
        lim = r.lim_at(r.pos)
    if filler == "zero" and delta == 2:  # no header at lim + 1: a 2-byte packet at lim
        r.fill_to(filler, lim)
        r.emit(("run", 1, val(seed + 1)))
    r.fill_to(filler, lim + delta)
    at = r.pos
    r.emit(PACKETS[packet](seed))
    data, row = r.finish(min_len)
    return data, row, at


def window_file(w, addr0, filler):
    """40 rows: {first, second window} x {lim-1, lim, lim+1, lim+2} x the five packets."""
    grid = [(which, delta, p) for which in (1, 2) for delta in DELTAS for p in PACKETS]
    head = H.header(w, len(grid))
    body, rows, marks = [], [], []
    pos = len(head)
    min_len = 16 * w + 64 + 8 if filler == "zero" else 0  # past the walk cap: left to the serial walk
    for y, (which, delta, p) in enumerate(grid):
        data, row, at = window_row(w, pos, addr0, which, delta, p, filler, 17 * y + addr0, min_len)
        marks.append(dict(row_start=pos, at=at, which=which, delta=delta, packet=p))
        body.append(data)
        rows.append(row)
        pos += len(data)
    return head + b"".join(body), np.stack(rows), marks


def _window_cases():
    out = []
    for a in range(16):
        f, px, marks = window_file(2200, a, "run1")
        out.append(Case(f"win_link_a{a}", "window", f, a, OK, px, 2,
                        "packet headers at lim-1..lim+2 of windows 1 and 2, one-pixel-run filler", dict(marks=marks)))
    for a in (0, 5, 10, 15):
        f, px, marks = window_file(300, a, "zero")
        out.append(Case(f"win_walk_a{a}", "window", f, a, OK, px, 3,
                        "the same grid behind empty-literal filler, scanlines past the walk cap", dict(marks=marks)))
    for k in range(16):  # the last row's window reaches past the file end: sizes at every residue
        rows = [run_row(8, 0), scanline(8, [[("lit", b"")] * k + runs(8, val(k))] + [runs(8, val(k + c)) for c in (1, 2, 3)])]
        f = H.header(8, 2) + b"".join(r[0] for r in rows)
        out.append(Case(f"win_eof_{len(f) % 16}", "eof", f, 0, OK, np.stack([r[1] for r in rows]), 2,
                        "a window load whose 16-byte chunk straddles the file end", dict(size_mod16=len(f) % 16)))
    return out


_MENU = [
    lambda k: runs(8, val(k)),
    lambda k: [("lit", vals(k, 8))],
    lambda k: [("run", 4, val(k)), ("lit", vals(k + 1, 4))],
    lambda k: [("lit", vals(k, 3)), ("run", 5, val(k + 9))],
    lambda k: [("lit", b""), ("run", 8, val(k))],
    lambda k: [("run", 1, val(k)), ("run", 2, val(k + 1)), ("run", 3, val(k + 2)), ("run", 2, val(k + 3))],
    lambda k: [("lit", vals(k, 1)), ("run", 7, val(k + 5))],
]
_PAT8 = bytes((2, 2, 0, 8))


def scan_tail_hits(f: bytes) -> int:
    w, _, ds = parse_header(f)
    return sum(p >= scan_tail_start(f) for p in pattern_positions(f, w, ds))


def scan_file(trailing: int):
    """w = 8 rows of 12..40 bytes whose starts fall on every (start - ds) mod 16, then a last row
    whose literals hold the start pattern three times and `trailing` bytes of that pattern. A
    new-style row is at least 12 bytes, so at most two true rows can start in the bytes the scan
    reads one at a time; the pattern copies in the last row and after it (all sorted behind the
    true starts, so the file still links) bring that count to three or more."""
    rng = np.random.default_rng(500 + trailing)
    last = [runs(8, 40), runs(8, 41), [("lit", vals(5, 4) + _PAT8)], [("lit", _PAT8 * 2)]]
    tail = (_PAT8 * 6)[:trailing]
    rows, starts, pos, k = [], set(), 0, 0
    while True:
        if len(rows) >= 18 and len(starts) == 16:
            cand = rows + [scanline(8, last)]
            f = H.header(8, len(cand)) + b"".join(r[0] for r in cand) + tail
            if scan_tail_hits(f) >= 3:
                return f, np.stack([r[1] for r in cand])
        r = scanline(8, [_MENU[int(rng.integers(len(_MENU)))](k + 13 * c) for c in range(4)])
        k += 1
        starts.add(pos & 15)
        rows.append(r)
        pos += len(r[0])


def _scan_cases():
    out = []
    for t in range(24):
        f, px = scan_file(t)
        for off in range(4):
            out.append(Case(f"scan_t{t}_o{off}", "scan", f, off, OK, px, 2,
                            "row starts at every chunk position, three patterns in the byte-wise tail", dict(trailing=t)))
    return out


def _new_file(w, rows, trailing=b""):
    return H.header(w, len(rows)) + b"".join(r[0] for r in rows) + trailing, np.stack([r[1] for r in rows])


def _width_cases():
    out = []
    w = 514  # the pattern is 2 2 2 2: it overlaps itself
    rows = [run_row(w, y) for y in range(3)]
    f, px = _new_file(w, rows)
    out.append(Case("w514", "width", f, 1, OK, px, 2, "self-overlapping pattern, no literal code 2 after a header"))
    rows[1] = scanline(w, [[("lit", vals(1, 2))] + runs(w - 2, 9)] + [runs(w, val(c)) for c in range(3)])
    f, px = _new_file(w, rows)
    out.append(Case("w514_lit2", "width", f, 2, OK, px, 3, "a literal code 2 after a row header: an adjacent false start"))
    rows = [run_row(257, y) for y in range(3)]
    f, px = _new_file(257, rows)
    out.append(Case("w257", "width", f, 3, OK, px, 2, "pattern 2 2 1 1"))
    rows = [scanline(32767, [runs(32766, val(y + c)) + [("lit", vals(y, 1))] for c in range(4)]) for y in range(2)]
    f, px = _new_file(32767, rows)
    out.append(Case("w32767", "width", f, 5, OK, px, 2, "the widest new-style scanline"))
    px = flat_px(1, 32768, 1)
    px[0, 0] = (2, 2, 0, 0)
    out.append(Case("w32768", "width", flat_file(px), 6, OK, px, 1, "2 2 0 0 at a width past 0x7fff: a pixel"))
    px = flat_px(2, 7, 3)
    px[1, 0] = (2, 2, 0, 7)
    out.append(Case("w7", "width", flat_file(px), 7, OK, px, 1, "2 2 0 7 at a width under 8: a pixel"))
    return out


def _link_cases():
    out = []
    w = 8

    def add(name, rows, mode, edge, trailing=b"", off=0):
        f, px = _new_file(w, rows, trailing)
        out.append(Case(name, "link", f, off, OK, px, mode, edge))

    def with_false(y):  # row y's G literal holds the start pattern
        return scanline(w, [runs(w, val(y)), [("lit", vals(y, 4) + _PAT8)], runs(w, val(y + 1)), runs(w, val(y + 2))])

    for h in (1, 2, 3, 1025):
        add(f"link_h{h}", [run_row(w, y) for y in range(h)], 2, "exactly h starts", off=h & 3)
    rows = [run_row(w, y) for y in range(3)]
    add("link_trailing_false", rows, 2, "a false start after the last row: the first h chain", _PAT8 + b"\x09\x09")
    add("link_false_mid", [rows[0], with_false(1), rows[2]], 3, "a false start inside a middle row")
    add("link_false_row0", [with_false(0), rows[1], rows[2]], 3, "a false start inside row 0")
    add("link_false_last", [rows[0], rows[1], with_false(2)], 2, "a false start inside the last row sorts behind")
    big = [run_row(w, y) for y in range(8193)]
    add("link_h8192", big[:8192], 2, "the sort's capacity, no padding keys", off=1)
    add("link_h8191_trailing", big[:8191], 2, "8191 rows and a trailing false start fill the capacity", _PAT8, off=2)
    add("link_h8193", big, 3, "one start more than the sort holds", off=3)
    rows4 = [run_row(w, y) for y in range(4)]
    bad = scanline(w, [runs(w, val(c)) for c in range(4)], header=(2, 2, 0, 99))
    add("link_width_mismatch", [bad] + rows4[1:], 3, "row 0's header names another width: still new-style, not a start")
    cap = 16 * w + 64
    for d in (-1, 0, 1, 2, 3):  # the last packet is a 2-byte run: its header is at length - 2
        n0 = len(run_row(w, 0)[0])
        rows = [scanline(w, [[("lit", b"")] * (cap + d - n0) + runs(w, val(y))] + [runs(w, val(y + c)) for c in (1, 2, 3)])
                for y in range(2)]
        assert all(len(r[0]) == cap + d for r in rows)
        add(f"link_cap{d:+d}", rows, 2 if d <= 1 else 3, "scanlines of cap-1..cap+3 bytes, cap = 16 w + 64")
    return out


def _plain_cases():
    out = []
    px = flat_px(3, 9, 3)
    px[1, 3, 2:] = (1, 1)
    px[1, 4] = (1, 77, 1, 1)
    px[1, 5, :2] = (1, 9)
    out.append(Case("plain_111_straddle", "plain", flat_file(px), 0, OK, px, 1, "1 1 1 across two pixels is no marker"))
    for b, mode in ((200, 1), (100, 3)):
        px = flat_px(4, 9, 3)
        px[1, 0] = (2, 2, b, 130)
        f = flat_file(px)
        out.append(Case(f"plain_22_{b}", "plain", f, 1, None if mode == 3 else OK, None if mode == 3 else px, mode,
                        "row 1 starts 2 2 b: a pixel when b >= 128, else the new-style decoder takes it"))
    w = 16  # R's literal data starts at ds + 5: data[3..6] is the group at ds + 8
    rows = [scanline(w, [[("lit", vals(y, 3) + bytes((1, 1, 1, 140)) + vals(y, 9))]] + [runs(w, val(y + c)) for c in range(3)])
            for y in range(2)]
    f, px = _new_file(w, rows)
    out.append(Case("new_with_marker", "plain", f, 2, OK, px, 2, "an aligned 1 1 1 E inside a literal: still linked"))
    w = 12
    r0 = scanline(w, [runs(w, 50), runs(w, 60), runs(w, 70), [("lit", b"")] + runs(w, 130)])  # 13 bytes
    p = flat_px(5, w, 2)
    for marker in (True, False):
        q = p.copy()
        if marker:
            q[0, 2:5] = q[0, 1]
            row1 = q[0, :2].tobytes() + bytes((1, 1, 1, 3)) + q[0, 5:].tobytes()
        else:
            row1 = q[0].tobytes()
        f = H.header(w, 3) + r0[0] + row1 + q[1].tobytes()
        px = np.stack([r0[1], q[0], q[1]])
        out.append(Case("mixed_row_marker" if marker else "mixed_misaligned_flat", "plain", f, 3, OK, px, 3,
                        "a flat-coded row off the data start's alignment" + (", with a marker only its row sees" if marker else "")))
    return out


def _convert_cases():
    out = []
    v = np.arange(256, dtype=np.uint8)
    px = np.empty((256, 256, 4), np.uint8)
    px[..., 0], px[..., 1], px[..., 2] = v[None, :], 255 - v[None, :], v[None, :] ^ 0x55
    px[..., 3] = v[:, None]
    out.append(Case("convert_flat", "convert", flat_file(px), 0, OK, px, 1, "every exponent x every mantissa, flat"))
    rows = [scanline(256, [[("lit", px[y, :128, c].tobytes()), ("lit", px[y, 128:, c].tobytes())] for c in range(3)]
                     + [runs(256, y)]) for y in range(256)]
    f, px2 = _new_file(256, rows)
    out.append(Case("convert_new", "convert", f, 0, OK, px2, 2, "every exponent x every mantissa, new-style"))
    for w in (1, 2, 5):
        for off in range(4):
            px = flat_px(10 * w + off, w, 3)
            out.append(Case(f"flat_w{w}_o{off}", "convert", flat_file(px), off, OK, px, 1,
                            "the last pixel of a flat file that ends with it"))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_window_cases() + _scan_cases() + _width_cases() + _link_cases() + _plain_cases() + _convert_cases())


GROUPS = ("window", "eof", "scan", "width", "link", "plain", "convert")


@functools.lru_cache(maxsize=None)
def expectations():
    """name -> (oracle result, predict's (mode, ncand)): computed once, shared by the tests."""
    from oracle import pyoracle as O
    return {c.name: (O.hdr_decode(c.file), predict(c.file)) for c in cases()}


def place(group_cases, pad_byte=0xEE):
    """The batch blob: each file after padding that brings it to its blob_offset (mod 16).
    -> (blob, offsets, sizes)"""
    blob, offs = bytearray(), []
    for c in group_cases:
        blob += bytes((pad_byte,)) * ((c.blob_offset - len(blob)) % 16)
        offs.append(len(blob))
        blob += c.file
    return bytes(blob), offs, [len(c.file) for c in group_cases]
