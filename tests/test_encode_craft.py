"""The crafted JPEG encoder inputs (tests/jpegenc_craft.py) reach the entropy coder's extremes.

CPU only. The coverage conditions below are conditions on the INPUTS, asserted on what the oracle
encoders write for them (they never read the code under test): tests/test_gpu_encode_craft.py
then compares the GPU encoder with the oracle on exactly these inputs, so a state listed here is
a state the GPU comparison exercises. The oracle itself is pinned to the reference encoder on
every crafted tiny_jpeg input where the reference build is present.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
import jpegenc_craft as J

KINDS = ("tje", 444, 420)
# the qualities whose quantiser is all ones: the largest amplitudes and DC steps
Q1 = {"tje": 3, 444: 100, 420: 100}


def encode(kind, q, px):
    h, w, c = px.shape
    if kind == "tje":
        return O.tje_encode(q, w, h, c, px.tobytes())
    return O.jpeg_encode(q, kind, w, h, c, px.tobytes())


_CACHE = {}


def files(kind):
    """{(family, name, quality): (pixels, the oracle's file, analyse())}, computed once."""
    if kind not in _CACHE:
        out = {}
        for fam, name, px in J.crafted(kind):
            for q in J.QUALITIES[kind]:
                jp = encode(kind, q, px)
                assert jp is not None
                out[(fam, name, q)] = (px, jp, J.analyse(jp, O.decode_trace))
        _CACHE[kind] = out
    return _CACHE[kind]


def _swing_geometry_ok(a, name):
    """dc_swing at a width of one MCU more than a whole number of 512-pixel runs: the MCU that is
    a run of its own takes the full DC step coming in (a run boundary) and the next one, the first
    of the next MCU row, takes it going out (a row boundary), in every MCU row."""
    ms = 16 if a["sub"] == 420 else 8
    upm = 6 if a["sub"] == 420 else 3
    mbw, mbh = (a["w"] + ms - 1) // ms, (a["h"] + ms - 1) // ms
    if mbw % (512 // ms) != 1 or mbh < 2:
        return False
    c = {"grey": 0, "by": 1, "rc": 2}[name.split("_")[1]]
    firstk = {0: 0, 1: upm - 2, 2: upm - 1}[c]  # the component's first unit in an MCU
    step = 2040
    d = np.abs(a["dc_diffs"])
    for r in range(mbh):
        alone = r * mbw + mbw - 1
        if d[alone * upm + firstk] != step:
            return False
        if r + 1 < mbh and d[(alone + 1) * upm + firstk] != step:
            return False
    return True


def _clamp_binds(kind, px):
    """edge_contrast's last column and row differ from their neighbours enough that replicating
    column w - 2 or row h - 2 instead (a clamp off by one) changes the file."""
    q = Q1[kind]
    h, w, _ = px.shape
    if w % 16 == 0 or h % 16 == 0:
        return False
    want = encode(kind, q, px)
    col = px.copy()
    col[:, w - 1] = col[:, w - 2]
    row = px.copy()
    row[h - 1] = row[h - 2]
    # the partial MCUs hold only replicated pixels, so these differ from `want` through the
    # replicated column / row as well as through the one real column / row
    return encode(kind, q, col) != want and encode(kind, q, row) != want


def coverage_failures(kind, drop_family=None):
    """Names of the coverage conditions the crafted set of `kind` (without drop_family) misses."""
    fs = {k: v for k, v in files(kind).items() if k[0] != drop_family}
    q1 = [a for (fam, name, q), (_, _, a) in fs.items() if q == Q1[kind]]
    every = [a for (_, _, a) in fs.values()]
    # tiny_jpeg: the amplitude, DC, run and FF conditions at quality 3; stream-length residues over
    # its three qualities (the GPU test runs all three through the same stuffing kernels)
    sel = q1 if kind == "tje" else every
    fails = []

    def need(name, ok):
        if not ok:
            fails.append(name)

    need("ac category 10, luma", max((a["ac_cat"]["luma"] for a in sel), default=0) == 10)
    need("ac category 10, chroma", max((a["ac_cat"]["chroma"] for a in sel), default=0) == 10)
    need("dc diff 2040, Y", max((a["dc_diff"]["Y"] for a in sel), default=0) == 2040)
    need("dc diff >= 2000, Cb", max((a["dc_diff"]["Cb"] for a in sel), default=0) >= 2000)
    need("dc diff >= 2000, Cr", max((a["dc_diff"]["Cr"] for a in sel), default=0) >= 2000)
    runs = set().union(*[a["runs"] for a in sel]) if sel else set()
    need("every zero run 15..62", set(range(15, 63)) <= runs)
    for cls in ("luma", "chroma"):  # the two ZRL codes differ (11 and 10 bits); any quality
        rc = set().union(*[a["runs_by_class"][cls] for a in every]) if every else set()
        need(f"runs of 16, 32 and 48 and more, {cls}", {16, 32, 48, 62} <= rc)
    need("three ZRLs", max((a["zrl_max"] for a in sel), default=0) == 3)
    pair = set().union(*[a["pair_runs"] for a in sel]) if sel else set()
    need("exact runs between two coefficients", {15, 16, 17, 31, 32, 33, 47, 48, 49} <= pair)
    need("a lone coefficient 63", any(a["lone63"] for a in sel))
    need("coefficient 63 after a second coefficient", any(a["coef63"] > a["lone63"] for a in sel))
    need("FF pair on a 16-byte edge", any(a["ff_pair_16"] for a in sel))
    need("FF pair on a 4096-byte edge", any(a["ff_pair_4096"] for a in sel))
    need("FF last in a 16-byte chunk", any(a["ff_last_of_chunk"] for a in sel))
    need("FF first in a 16-byte chunk", any(a["ff_first_of_chunk"] for a in sel))
    need("three FF bytes in a row", max((a["ff_longest"] for a in sel), default=0) >= 3)
    need("stream length residues mod 16", {a["len_mod16"] for a in every} == set(range(16)))
    need("dc swing on run and row boundaries",
         any(_swing_geometry_ok(a, name) for (fam, name, q), (_, _, a) in fs.items()
             if fam == "dc_swing" and q == Q1[kind]))
    need("edge clamp binds",
         any(_clamp_binds(kind, px) for (fam, name, q), (px, _, _) in fs.items()
             if fam == "edge_contrast" and q == Q1[kind]))
    if kind != 420:  # (4:2:0 tops out near 2.3 bytes a pixel: below both bounds)
        need("small image past 64 KiB of stream",
             any(a["w"] * a["h"] * 3 // 4 <= 65536 < a["stream_len"] for (fam, _, _), (_, _, a) in fs.items()
                 if fam == "noise01"))
        need("stuffed stream past source + 64 KiB",
             any(a["stuffed_len"] > a["w"] * a["h"] * 3 + 65536 for (fam, _, _), (_, _, a) in fs.items()
                 if fam == "noise01"))
    else:
        need("stream past the first words buffer",
             any(a["stream_len"] > max(65536, a["w"] * a["h"] * 3 // 4) for (fam, _, _), (_, _, a) in fs.items()
                 if fam == "noise01"))
    return fails


@pytest.mark.parametrize("kind", KINDS)
def test_crafted_set_reaches_the_coder_states(kind, capsys):
    with capsys.disabled():
        print("\n" + states_table(kind))
    assert coverage_failures(kind) == []


@pytest.mark.parametrize("family", J.FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_family_is_needed(kind, family):
    """Without any one family at least one coverage condition fails: the conditions bind."""
    assert coverage_failures(kind, drop_family=family) != []


def states_table(kind):
    """The coder states each family reaches (the table in DESIGN.md is this output)."""
    rows = [f"| {kind} | family | largest AC category Y / C | largest DC diff Y / Cb / Cr | zero runs >= 15 | "
            "most ZRLs | lone coef 63 | longest FF run | FF pair on 16 / 4096 edge |", "|---|---|---|---|---|---|---|---|---|"]
    for fam in J.FAMILIES:
        aa = [a for (f, _, q), (_, _, a) in files(kind).items() if f == fam and (kind != "tje" or q == 3)]
        runs = sorted(r for r in set().union(*[a["runs"] for a in aa]) if r >= 15)
        span = f"{len(runs)} of 48" if runs else "none"
        rows.append("| {} | {} | {} / {} | {} / {} / {} | {} | {} | {} | {} | {} / {} |".format(
            kind if kind != "tje" else "tje q3", fam, max(a["ac_cat"]["luma"] for a in aa),
            max(a["ac_cat"]["chroma"] for a in aa), max(a["dc_diff"]["Y"] for a in aa),
            max(a["dc_diff"]["Cb"] for a in aa), max(a["dc_diff"]["Cr"] for a in aa), span,
            max(a["zrl_max"] for a in aa), "yes" if any(a["lone63"] for a in aa) else "no",
            max(a["ff_longest"] for a in aa), "yes" if any(a["ff_pair_16"] for a in aa) else "no",
            "yes" if any(a["ff_pair_4096"] for a in aa) else "no"))
    return "\n".join(rows)


def test_ff_literals_are_what_they_claim():
    """Each FF_PLACED entry, at its own quality, holds the FF placement it is named after."""
    for kind in KINDS:
        for goal, (q, *_rest) in J.FF_PLACED[kind].items():
            a = files(kind)[("ff_placed", f"ff_{goal}", q)][2]
            assert {"pair16": a["ff_pair_16"], "pair4096": a["ff_pair_4096"], "run3": a["ff_longest"] >= 3}[goal], \
                (kind, goal)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_decodes_every_crafted_file(kind):
    for (fam, name, q), (px, jp, a) in files(kind).items():
        code, w, h, n, pix = O.decode(jp)
        assert code == 0 and (h, w) == px.shape[:2] and n == 3 and len(pix) == w * h * 3, (name, q)


@pytest.mark.skipif(not O.ref_available(), reason="the reference build (oracle/_ref) is not present")
@pytest.mark.parametrize("comps", [3, 4])
def test_oracle_matches_reference_on_crafted_inputs(comps):
    """The oracle is a restatement; at these extremes it had never been compared with the
    reference encoder itself."""
    for fam, name, px in J.crafted("tje", comps):
        h, w, c = px.shape
        for q in (1, 2, 3):
            want = O.ref_tje_encode(q, w, h, c, px.tobytes(), cap=8 * w * h + 65536)  # (past 4.8 bytes a pixel)
            assert want is not None and O.tje_encode(q, w, h, c, px.tobytes()) == want, (name, q)
