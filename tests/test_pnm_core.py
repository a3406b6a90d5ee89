"""The Netpbm read and write without a GPU: icx_pnm_core.h (header walk, byte classes, serial decode
and encode) through icx_pnm_probe and through tests/cxx/pnm_core_demo.cpp (built with g++, and again
with -fsanitize=address,undefined as a program of its own), against the restatement in
tests/pnmutil.py, the reference's data/test.pbm / .pgm / .ppm / .pnm / .pfm and PIL."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import imagecodecs_amd as icx
import pnmutil as U

TILE = icx.PNM_ASCII_TILE
FIXTURES = {n: open(os.path.join(GOLDEN, "pnm", n), "rb").read()
            for n in ("test.pbm", "test.pgm", "test.ppm", "test.pnm", "test_48rows.pfm")}
FIXTURE_DIMS = {"test.pbm": (499, 289, 1, U.UBYTE, 255), "test.pgm": (499, 289, 1, U.UBYTE, 255),
                "test.ppm": (499, 289, 3, U.UBYTE, 255), "test.pnm": (499, 289, 3, U.UBYTE, 255),
                "test_48rows.pfm": (499, 48, 3, U.FLOAT, 0)}


def crafted_files():
    """Every crafted file of the corpus (what the GPU tests decode) -> [(name, file)]."""
    out = [(n, f) for n, f, _ in U.header_cases()] + [(n, f) for n, f, _ in U.text_error_cases()]
    for kind in U.BINARY_KINDS:
        out += [(n, f) for n, f, _ in U.binary_cases(kind)]
    out += U.align_cases() + U.maxval_cases() + U.float_cases() + U.text_general_cases(TILE) + U.text_edge_cases(TILE)
    out += [(n, f) for n, (f, _) in U.p1_cases(TILE)] + U.prefix_and_flip_cases()
    return out


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "pnm_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "pnm_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "pnm_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_codes_and_constants_match_the_headers():
    assert (icx.PNM_OK, icx.PNM_NOT_PNM, icx.PNM_BAD_HEADER, icx.PNM_UNSUPPORTED, icx.PNM_BAD_DATA, icx.PNM_TRUNCATED,
            icx.PNM_TOO_LARGE, icx.PNM_INVALID_ARGUMENT) == (U.OK, U.NOT_PNM, U.BAD_HEADER, U.UNSUPPORTED, U.BAD_DATA,
                                                             U.TRUNCATED, U.TOO_LARGE, U.INVALID_ARGUMENT)
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    for name, v in (("OK", 0), ("NOT_PNM", 1), ("BAD_HEADER", 2), ("UNSUPPORTED", 3), ("BAD_DATA", 4), ("TRUNCATED", 5),
                    ("TOO_LARGE", 6), ("INVALID_ARGUMENT", 7), ("INTERNAL_ERR", -1), ("P4", 4), ("P5", 5), ("P6", 6), ("PF", 8),
                    ("UBYTE", 0), ("USHORT", 1), ("FLOAT", 2)):
        assert re.search(rf"\bICX_PNM_{name} = {v}\b", src), name
    core = open(os.path.join(ROOT, "imagecodecs_amd", "csrc", "icx_pnm_core.h")).read()
    assert int(re.search(r"constexpr int kPnmTile = (\d+);", core).group(1)) == TILE and TILE <= 16384
    assert (icx.PNM_P4, icx.PNM_P5, icx.PNM_P6, icx.PNM_PF) == (U.P4, U.P5, U.P6, U.PF)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_probe_fixtures(name):
    assert icx.pnm_probe(FIXTURES[name]) == (icx.PNM_OK, *FIXTURE_DIMS[name]) == U.probe(FIXTURES[name])


def test_fixtures_are_the_reference_files():
    assert [len(FIXTURES[n]) for n in ("test.pbm", "test.pgm", "test.ppm", "test.pnm")] == [18264, 144272, 432694, 432694]
    assert [FIXTURES[n][:2] for n in ("test.pbm", "test.pgm", "test.ppm", "test.pnm")] == [b"P4", b"P5", b"P6", b"P6"]
    pfm = FIXTURES["test_48rows.pfm"]
    assert pfm[:15] == b"PF\n499 48\n-1.0\n" and len(pfm) == 15 + 499 * 48 * 12 < 1 << 20
    for n in FIXTURES:
        assert U.decode(FIXTURES[n])[:6] == (U.OK, *FIXTURE_DIMS[n])


@pytest.mark.parametrize("case", U.header_cases(), ids=lambda c: c[0])
def test_probe_crafted_headers(case):
    name, data, code = case
    got = icx.pnm_probe(data)
    assert got[0] == code
    assert got == U.probe(data)
    if code != U.OK:
        assert got[1:] == (0, 0, 0, 0, 0)


def test_probe_equals_restatement_on_the_corpus():
    seen = set()
    for name, data in crafted_files():
        got = icx.pnm_probe(data)
        assert got == U.probe(data), name
        seen.add(got[0])
    assert seen == {U.OK, U.NOT_PNM, U.BAD_HEADER, U.UNSUPPORTED, U.TRUNCATED, U.TOO_LARGE}


def test_encode_bound():
    for w, h in ((499, 289), (1, 1), (9, 3), (32768, 32768)):
        for d in (1, 3, 4):
            for typ in (U.UBYTE, U.USHORT, U.FLOAT):
                for fmt in (U.P4, U.P5, U.P6, U.PF, 7, 0):
                    assert icx.pnm_encode_bound(w, h, d, typ, fmt) == U.encode_bound(w, h, d, typ, fmt), (w, h, d, typ, fmt)
    assert icx.pnm_encode_bound(499, 289, 3, U.UBYTE, U.P6) == len(b"P6\n499 289\n255\n") + 499 * 289 * 3
    for w, h in ((0, 4), (4, 0), (-1, 4), (32769, 32768), (1 << 30, 2)):
        assert icx.pnm_encode_bound(w, h, 1, U.UBYTE, U.P5) == 0


def test_restatement_knows_its_inputs():
    """The builders' pixels are what the restatement decodes, and the expected codes of the error
    files are the restatement's."""
    for kind in U.BINARY_KINDS:
        for name, data, px in U.binary_cases(kind):
            got = U.decode(data)
            assert got[0] == U.OK and got[6].tobytes() == px.tobytes(), name
    for name, (data, px) in U.p1_cases(TILE):
        got = U.decode(data)
        assert got[0] == U.OK and (got[6] == px).all() and len(data) - U.parse(data)[1]["rs"] > TILE, name
    for name, data, code in U.text_error_cases():
        assert U.decode(data)[0] == code, name
    general = U.text_general_cases(TILE)
    for name, data in general + U.text_edge_cases(TILE):
        assert U.decode(data)[0] == U.OK, name
    assert all(len(f) - U.parse(f)[1]["rs"] >= 3 * TILE for _, f in general)
    assert sum(U.comment_spans_edge(f, TILE) for _, f in general) >= 2
    for e in (1, 2):
        for k in range(6):
            data, rs = U.edge_token_file(TILE, e, k)
            tok = re.compile(rb"[0-9]+").search(data, rs + e * TILE - k)
            assert tok.start() == rs + e * TILE - k and tok.end() - tok.start() == 5, (e, k)
            assert k == 0 or data[rs + e * TILE - k - 1:rs + e * TILE - k] == b" "
    codes = {U.decode(f)[0] for _, f in U.prefix_and_flip_cases()}
    assert codes >= {U.OK, U.NOT_PNM, U.BAD_HEADER, U.BAD_DATA, U.TRUNCATED}


def _pil(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_restatement_equals_pil():
    """8-bit fixtures, PIL-written P4 / P5 / P6 / Pf files and hand-written P1 / P2 / P3 text with
    maxval 255. (PIL rescales for other values of maxval and does not read PF.)"""
    from PIL import Image
    for name in ("test.pbm", "test.pgm", "test.ppm", "test.pnm"):
        im, ref = _pil(FIXTURES[name]), U.decode(FIXTURES[name])
        assert ref[0] == U.OK
        want = np.asarray(im.convert("L") if im.mode == "1" else im).reshape(ref[6].shape)
        assert (want == ref[6]).all(), name
    grey, rgb = U.synth(1, 67, 9, 1)[:, :, 0], U.synth(2, 67, 9, 3)
    mono = U.bitmap(3, 67, 9)[:, :, 0]
    flt = np.random.default_rng(4).standard_normal((9, 67)).astype(np.float32)
    for px, mode, fmt, ext in ((mono, "1", "PPM", "P4"), (grey, "L", "PPM", "P5"), (rgb, "RGB", "PPM", "P6"), (flt, "F", "PPM", "Pf")):
        buf = io.BytesIO()
        (Image.fromarray(px).convert("1") if mode == "1" else Image.fromarray(px, mode)).save(buf, fmt)
        data = buf.getvalue()
        assert data[:2] == ext.encode(), data[:16]
        ref = U.decode(data)
        assert ref[0] == U.OK and (ref[6].reshape(px.shape) == px).all(), ext
        assert (np.asarray(_pil(data).convert("L") if mode == "1" else _pil(data)).reshape(px.shape) == px).all()
    texts = [b"P1\n# a bitmap\n5 3\n01010\n1 0 1 0 1\n00 # c\n111\n",
             b"P2\n4 2 255\n0 1 2 3\n252\t253\r\n254 255",
             b"P3 2 2 255  255 0 0  0 255 0\n# mid\n0 0 255  17 18 19 "]
    for data in texts:
        im, ref = _pil(data), U.decode(data)
        assert ref[0] == U.OK
        want = np.asarray(im.convert("L") if im.mode == "1" else im).reshape(ref[6].shape)
        assert (want == ref[6]).all(), data[:2]


def _run_jobs(exe, tmp_path, jobs):
    lst = tmp_path / "jobs.txt"
    lst.write_text("".join(" ".join(str(x) for x in j) + "\n" for j in jobs))
    r = subprocess.run([exe, str(lst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(jobs)
    return [[int(x) for x in ln.split()] for ln in lines]


def _encode_inputs():
    out = []
    for w in (1, 7, 8, 9, 65):
        for h in (1, 3):
            out.append((U.bitmap(w + h, w, h), U.P4))
            for typ in (U.UBYTE, U.USHORT):
                out.append((U.synth(w, w, h, 1, typ), U.P5))
                out.append((U.synth(w, w, h, 3, typ), U.P6))
                out.append((U.synth(w, w, h, 4, typ), U.P6))
            out.append((U.synth(w, w, h, 1, U.FLOAT), U.PF))
            out.append((U.synth(w, w, h, 3, U.FLOAT), U.PF))
    out += [(U.synth(1, 4, 4, 3), U.P5), (U.synth(1, 4, 4, 1), U.P6), (U.synth(1, 4, 4, 1, U.FLOAT), U.P5),
            (U.synth(1, 4, 4, 3, U.USHORT), U.P4), (U.synth(1, 4, 4, 4, U.FLOAT), U.PF), (U.synth(1, 4, 4, 3), 7)]
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_program(which, demo, demo_san, tmp_path):
    """The C++ core as a program of its own: serial decode == restatement on every crafted file and
    the fixtures; serial encode == restatement, refusals included. The sanitized build runs the same
    jobs clean."""
    exe = demo if which == "plain" else demo_san
    files = crafted_files() + sorted(FIXTURES.items())
    jobs = []
    for k, (name, data) in enumerate(files):
        (tmp_path / f"in{k}").write_bytes(data)
        jobs.append(("decode", tmp_path / f"in{k}", tmp_path / f"out{k}"))
    got = _run_jobs(exe, tmp_path, jobs)
    for k, (name, data) in enumerate(files):
        ref = U.decode(data)
        assert tuple(got[k]) == ref[:6], name
        assert (tmp_path / f"out{k}").read_bytes() == (ref[6].tobytes() if ref[0] == U.OK else b""), name
    inputs = _encode_inputs()
    jobs = []
    for k, (px, fmt) in enumerate(inputs):
        (tmp_path / f"px{k}").write_bytes(px.tobytes())
        h, w, d = px.shape
        jobs.append(("encode", tmp_path / f"px{k}", w, h, d, U.type_of(px), fmt, tmp_path / f"file{k}"))
    got = _run_jobs(exe, tmp_path, jobs)
    for k, (px, fmt) in enumerate(inputs):
        want = U.encode(px, fmt) or b""
        assert got[k] == [len(want), len(want)], (px.shape, px.dtype, fmt)
        assert (tmp_path / f"file{k}").read_bytes() == want, (px.shape, px.dtype, fmt)
        if want:
            back = U.decode(want)
            kept = px[:, :, :3] if fmt == U.P6 else px
            assert back[0] == U.OK and back[6].tobytes() == np.ascontiguousarray(kept).tobytes(), (px.shape, px.dtype, fmt)
