"""The DDS read and write without a GPU: icx_dds_core.h (header walk, block decoders, range-fit block
encoders, masked and copied forms, serial decode and encode, header writer) through icx_dds_probe and
through tests/cxx/dds_core_demo.cpp (built with g++, and again with -fsanitize=address,undefined as a
program of its own), against the numpy restatement in tests/ddsutil.py, the reference's data/test.dds
and PIL."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import imagecodecs_amd as icx
import ddsutil as D

FIXTURE = open(os.path.join(GOLDEN, "dds", "test.dds"), "rb").read()
PPM = open(os.path.join(GOLDEN, "pnm", "test.ppm"), "rb").read()


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "dds_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "dds_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "dds_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def corpus():
    """(name, file) of every shared case list, the fixture, prefixes and bit flips included."""
    files = [("fixture", FIXTURE)] + D.block_cases() + D.alias_cases() + D.mask_cases() + D.field_sweep_cases()
    files += [(n, f) for n, f, _ in D.error_cases() if len(f) < 1 << 20]
    for k, src in enumerate(D.fuzz_sources(FIXTURE)):
        pre = D.prefixes(src)
        assert len(pre) <= 300
        files += [(f"prefix{k}_{len(p)}", p) for p in pre]
        flips = D.bit_flips(src, 77 + k)
        assert len(flips) == 200
        files += [(f"flip{k}_{j}", p) for j, p in enumerate(flips)]
    return files


@pytest.fixture(scope="module")
def expected(corpus):
    """The restatement's result for every file of the corpus, computed once."""
    return [D.decode(f) for _, f in corpus]


@pytest.fixture(scope="module")
def encoder_corpus():
    """(name, pixels, format) for RAW and BC, d = 1..4, the exhaustive alpha image included."""
    out = [(f"{n}_d{d}_f{fmt}", px, fmt) for d in (1, 2, 3, 4) for n, px in D.encoder_images(d) for fmt in (D.RAW, D.BC)]
    out.append(("alpha_exhaustive", D.alpha_exhaustive_image(), D.BC))
    return out


def test_codes_match_the_header():
    assert (icx.DDS_OK, icx.DDS_NOT_DDS, icx.DDS_BAD_HEADER, icx.DDS_UNSUPPORTED, icx.DDS_TRUNCATED, icx.DDS_TOO_LARGE,
            icx.DDS_INVALID_ARGUMENT, icx.DDS_INTERNAL_ERR) == (D.OK, D.NOT_DDS, D.BAD_HEADER, D.UNSUPPORTED, D.TRUNCATED,
                                                                 D.TOO_LARGE, D.INVALID_ARGUMENT, -1)
    assert (icx.DDS_RAW, icx.DDS_BC) == (D.RAW, D.BC) == (0, 1)
    src = open(os.path.join(ROOT, "include", "icx.h")).read()
    for name, v in (("OK", 0), ("NOT_DDS", 1), ("BAD_HEADER", 2), ("UNSUPPORTED", 3), ("TRUNCATED", 4), ("TOO_LARGE", 5),
                    ("INVALID_ARGUMENT", 6), ("INTERNAL_ERR", -1)):
        assert f"ICX_DDS_{name} = {v}," in src or f"ICX_DDS_{name} = {v} " in src, name
    assert "ICX_DDS_RAW = 0, ICX_DDS_BC = 1" in src
    assert (icx.PNM_UBYTE, icx.PNM_USHORT, icx.PNM_FLOAT) == (D.UBYTE, D.USHORT, D.FLOAT)


def test_fixture_is_the_reference_file():
    assert len(FIXTURE) == 432761 == 128 + 499 * 289 * 3
    assert struct.unpack_from("<4s4I", FIXTURE, 0)[:2] == (b"DDS ", 124) and struct.unpack_from("<2I", FIXTURE, 12) == (289, 499)
    assert struct.unpack_from("<8I", FIXTURE, 76) == (32, 0x40, 0, 24, 0xFF0000, 0xFF00, 0xFF, 0)
    code, w, h, d, t, px = D.decode(FIXTURE)
    assert (code, w, h, d, t) == (D.OK, 499, 289, 3, D.UBYTE)
    assert PPM[-499 * 289 * 3:] == px.tobytes()
    raw = np.frombuffer(FIXTURE, np.uint8, 499 * 289 * 3, 128).reshape(289, 499, 3)
    assert (raw[:, :, ::-1] == px).all()  # B,G,R in the file


def test_probe_fixture():
    assert icx.dds_probe(FIXTURE) == (icx.DDS_OK, 499, 289, 3, icx.PNM_UBYTE)
    assert icx.dds_probe(b"") == (icx.DDS_NOT_DDS, 0, 0, 0, 0)


def test_probe_equals_restatement(corpus):
    """Size, channels, type and code of the host header walk, every file of the corpus."""
    for name, f in corpus:
        assert icx.dds_probe(f) == D.probe(f), name


@pytest.mark.parametrize("case", D.error_cases(), ids=lambda c: c[0])
def test_error_cases_are_what_they_say(case):
    name, f, code = case
    assert D.probe(f)[0] == code
    assert icx.dds_probe(f)[0] == code


def test_every_status_and_form_is_in_the_corpus(corpus, expected):
    codes = {e[0] for e in expected}
    assert codes == {D.OK, D.NOT_DDS, D.BAD_HEADER, D.UNSUPPORTED, D.TRUNCATED, D.TOO_LARGE}
    forms = {(e[3], e[4]) for e in expected if e[0] == D.OK}
    assert forms == {(1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2)}
    names = {n for n, _ in corpus}
    assert {f"{cc.decode()}_{w}x{h}" for cc in D.BLOCK_FOURCCS for w in range(1, 22) for h in range(1, 10)} <= names
    assert {f"cc_{cc.decode()}" for cc in D.FOURCC_BC} | {f"dxgi_{v}" for v in D.DXGI_BC} <= names


def test_encode_bound():
    assert icx.dds_encode_bound(499, 289, 3, icx.DDS_RAW) == 128 + 499 * 289 * 3 == D.encode_bound(499, 289, 3, D.RAW)
    assert icx.dds_encode_bound(499, 289, 3, icx.DDS_BC) == 128 + 125 * 73 * 8
    assert icx.dds_encode_bound(5, 2, 4, icx.DDS_BC) == 128 + 2 * 16 and icx.dds_encode_bound(5, 2, 1, icx.DDS_BC) == 128 + 2 * 8
    assert icx.dds_encode_bound(5, 2, 2, icx.DDS_BC) == 128 + 2 * 16 and icx.dds_encode_bound(5, 2, 2, icx.DDS_RAW) == 128 + 20
    assert icx.dds_encode_bound(65535, 65535, 4, icx.DDS_RAW) == 128 + 4 * 65535 * 65535
    for w, h, d, fmt in ((0, 4, 3, 0), (4, 0, 3, 0), (65536, 1, 3, 1), (1, 65536, 1, 0), (4, 4, 0, 0), (4, 4, 5, 1), (-1, 4, 3, 0),
                         (4, 4, 3, 2), (4, 4, 3, -1)):
        assert icx.dds_encode_bound(w, h, d, fmt) == 0 == D.encode_bound(w, h, d, fmt)
    for d in (1, 2, 3, 4):
        for fmt in (D.RAW, D.BC):
            for w, h in ((1, 1), (4, 4), (5, 9), (499, 289)):
                assert icx.dds_encode_bound(w, h, d, fmt) == D.encode_bound(w, h, d, fmt) == len(D.encode(D.synth(1, w, h, d), fmt))


# ------------------------------------------------------------------------------------ PIL
def _pil(data):
    """The file as PIL reads it, (h, w, bands), or None where PIL does not open it."""
    from PIL import Image  # (no skip: the comparison is part of what these tests check)
    try:
        im = Image.open(io.BytesIO(data))
        im.load()
    except Exception:
        return None
    a = np.asarray(im)
    return a[:, :, None] if a.ndim == 2 else a


def _pil_field_table(width):
    """PIL scales a field of `width` <= 8 bits as int(v / m * 255), truncating, where the contract
    rounds ((v * 510 + m) / (2 m), BMP's scaling). Both are increasing in v and PIL's is one to one,
    so PIL's value names v: the table maps it to the contract's value."""
    m = (1 << width) - 1
    t = np.zeros(256, np.int64) - 1
    for v in range(m + 1):
        t[int((v / m) * 255)] = (v * 510 + m) // (2 * m)
    return t


def _same_as_pil(px, pil, widths):
    """Channel c of the restatement against PIL's, through the field's width (None or 8: equal)."""
    for c in range(px.shape[2]):
        ours, theirs = px[:, :, c].astype(np.int64), pil[:, :, c].astype(np.int64)
        n = widths[c] if widths else 8
        if n == 8:
            ok = (ours == theirs).all()
        elif n < 8:
            ok = (_pil_field_table(n)[theirs] == ours).all()
        else:
            # a wider field: the contract gives the top 8 bits, floor(v * 256 / 2^n); PIL gives
            # floor(v * 255 / (2^n - 1)). The second ratio is the smaller one, by less than
            # (2^n - 256) / (2^n - 1) < 1 over the field's range, so PIL's value is ours or one less
            ok = ((theirs == ours) | (theirs == ours - 1)).all()
        if not ok:
            return False
    return True


def test_restatement_equals_pil():
    """Wherever PIL opens the file. BC1 is compared on the first three channels (PIL adds an alpha),
    BC5 on the first two (PIL adds a zero blue), files with fewer masks than R,G,B on the channels they
    have. An X8 file must give 3 channels with the fourth byte dropped. PIL reads masked files with the
    masks but scales a field by truncation where the contract rounds: _same_as_pil compares through
    that relation, exactly for fields of up to 8 bits. One form is left out: for a luminance file PIL
    ignores the masks and returns the stored byte, so A4L4 is not what the contract says it is."""
    cases = [("fixture", FIXTURE, None)] + [(n, f, None) for n, f in D.block_cases() + D.alias_cases()]
    for k, (name, bits, masks, pff) in enumerate(D.MASK_SETS):
        if name == "a4l4":
            continue
        widths = [bin(m).count("1") for m in D._channels(bits, masks, bool(pff & 0x20000))]
        cases += [(n, f, widths) for n, f in D.mask_cases() if n.startswith(f"mask_{name}_")]
    cases += [(n, f, [bin(m).count("1") for m in D._channels(bits, masks, bool(pff & 0x20000))])
              for n, f in D.field_sweep_cases() for name, bits, masks, pff in D.MASK_SETS if n == f"sweep_{name}" and name != "a4l4"]
    opened = set()
    for name, f, widths in cases:
        pil = _pil(f)
        if pil is None:
            continue
        opened.add(name)
        code, w, h, d, t, px = D.decode(f)
        assert code == D.OK and t == D.UBYTE and pil.shape[:2] == (h, w) and pil.shape[2] >= d, name
        assert _same_as_pil(px, pil, widths), name
    # what PIL 10 and later open of these: every DXT1 / DXT3 / DXT5 / ATI1 / ATI2 file, the fixture and
    # the files under the RGB flag, 8-bit luminance and 16-bit luminance with alpha
    must = {"fixture"} | {n for n, _ in D.block_cases()} | {"cc_DXT1", "cc_DXT3", "cc_DXT5", "cc_ATI1", "cc_BC4U", "cc_ATI2", "cc_BC5U"}
    must |= {f"mask_{n}_7x3" for n in ("r8g8b8", "b8g8r8", "a8r8g8b8", "a8b8g8r8", "x8r8g8b8", "x8b8g8r8", "r5g6b5", "a1r5g5b5",
                                       "a4r4g4b4", "a2r10g10b10", "g16r16", "r3g3b2", "l8", "a8l8")}
    must |= {"sweep_r5g6b5", "sweep_a1r5g5b5", "sweep_a4r4g4b4", "sweep_x4r4g4b4", "sweep_a8r3g3b2", "sweep_r3g3b2"}
    assert must <= opened, sorted(must - opened)[:10]
    # the X8 form by name: three channels, PIL's first three
    f = dict(D.mask_cases())["mask_x8r8g8b8_7x3"]
    px, pil = D.decode(f)[5], _pil(f)
    assert px.shape == (3, 7, 3) and (pil[:, :, :3] == px).all()
    stored = np.frombuffer(f, np.uint8, 7 * 3 * 4, 128).reshape(3, 7, 4)
    assert (stored[:, :, 2::-1] == px).all() and stored[:, :, 3].any()  # the fourth byte held something and is dropped


def test_written_files_open_in_pil(encoder_corpus):
    """PIL opens every written file and decodes it to what the restatement decodes (RAW: the pixels)."""
    for name, px, fmt in encoder_corpus:
        if name == "alpha_exhaustive":
            continue  # (2048 x 1664: the blocks are checked against the restatement, below)
        f = D.encode(px, fmt)
        pil = _pil(f)
        assert pil is not None, name
        code, w, h, d, t, back = D.decode(f)
        assert (code, w, h, d, t) == (D.OK, px.shape[1], px.shape[0], px.shape[2], D.UBYTE), name
        assert pil.shape[2] >= d and (pil[:, :, :d] == back).all(), name
        if fmt == D.RAW:
            assert (back == px).all(), name


# ------------------------------------------------------------------------------------ the C++ core
def _demo_decode(exe, tmp_path, files):
    lines = []
    for k, f in enumerate(files):
        p = tmp_path / f"{k}.dds"
        p.write_bytes(f)
        lines.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "decode", str(tmp_path / "list.txt"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    heads = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    return heads, (tmp_path / "out.bin").read_bytes()


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_decode(which, demo, demo_san, tmp_path, corpus, expected):
    """The C++ core as a program of its own: serial decode == restatement on the whole corpus --
    status, size, channels, type and every byte (NaN payloads as stored). The sanitized build runs the
    same inputs clean."""
    exe = demo if which == "plain" else demo_san
    heads, blob = _demo_decode(exe, tmp_path, [f for _, f in corpus])
    assert len(heads) == len(corpus)
    at = 0
    for (name, _), got, (code, w, h, d, t, px) in zip(corpus, heads, expected):
        assert got == (code, w, h, d, t), name
        if code == D.OK:
            want = px.tobytes()
            assert blob[at:at + len(want)] == want, name
            at += len(want)
    assert at == len(blob)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_encode(which, demo, demo_san, tmp_path, encoder_corpus):
    """Serial encode == restatement byte for byte, RAW and BC, d = 1..4: noise, flat and two-colour
    blocks, gradients, crafted ties, widths and heights 1-9 and the exhaustive alpha set."""
    exe = demo if which == "plain" else demo_san
    lines = []
    for k, (name, px, fmt) in enumerate(encoder_corpus):
        (tmp_path / f"{k}.bin").write_bytes(px.tobytes())
        lines.append(f"{tmp_path / f'{k}.bin'} {px.shape[1]} {px.shape[0]} {px.shape[2]} {fmt} {tmp_path / f'{k}.dds'}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "write", str(tmp_path / "list.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k, (name, px, fmt) in enumerate(encoder_corpus):
        assert (tmp_path / f"{k}.dds").read_bytes() == D.encode(px, fmt), name


def test_encoder_corpus_is_what_it_says():
    """The exhaustive alpha set holds every pair a1 < a0 with every value strictly between; the tie
    images hold pixels equidistant from two palette entries, in alpha and in colour."""
    b = D.alpha_exhaustive()
    assert 190000 < len(b) < 220000 and (b[:, 0] > b[:, 1]).all()
    assert (b[:, 2:] > b[:, 1:2]).all() and (b[:, 2:] < b[:, 0:1]).all()
    seen = np.zeros((256, 256, 256), bool)
    seen[np.repeat(b[:, 0], 14), np.repeat(b[:, 1], 14), b[:, 2:].reshape(-1)] = True
    a0, a1, v = np.ogrid[0:256, 0:256, 0:256]
    assert (seen == ((a1 < v) & (v < a0))).all()
    img = D.alpha_exhaustive_image()
    assert img.shape[2] == 1 and img.shape[1] == 2048 and img.shape[0] * 512 >= len(b)

    def ties(dist):  # pixels whose least distance is met by two entries
        s = np.sort(dist, -1)
        return int((s[..., 0] == s[..., 1]).sum())

    a = np.array(D.TIE_ALPHA, np.int64)
    assert ties(np.abs(a[:, None] - D.alpha_palette(np.array([a.max()]), np.array([a.min()]))[0][None, :].astype(np.int64))) >= 7
    px = D.tie_image(3).reshape(4, 3, 4, 3).transpose(1, 0, 2, 3).reshape(3, 16, 3).astype(np.int64)
    enc = D.encode_color_blocks(px.astype(np.uint8))
    c = enc[:, :4].copy().view("<u2")
    pal = D.color_palette(c[:, 0], c[:, 1], True).astype(np.int64)
    for k in range(3):
        assert ties(((px[k][:, None, :] - pal[k][None, :, :]) ** 2).sum(2)) >= 3, k


def test_raw_round_trip_and_the_fixture():
    """decode(encode(x, RAW)) == x, and writing the fixture's pixels as RAW d = 3 reproduces its
    bytes from offset 128."""
    for d in (1, 2, 3, 4):
        for name, px in D.encoder_images(d):
            got = D.decode(D.encode(px, D.RAW))
            assert got[:5] == (D.OK, px.shape[1], px.shape[0], d, D.UBYTE) and (got[5] == px).all(), (name, d)
    px = D.decode(FIXTURE)[5]
    out = D.encode(px, D.RAW)
    assert out[128:] == FIXTURE[128:] and len(out) == len(FIXTURE)
    assert struct.unpack_from("<2I", out, 12) == struct.unpack_from("<2I", FIXTURE, 12)
    assert struct.unpack_from("<8I", out, 76) == struct.unpack_from("<8I", FIXTURE, 76)


def test_bc_encoder_is_no_worse_than_pil():
    """The quality condition: PSNR of decode(encode(x, BC)) for d = 3 is no lower than that of PIL's
    own DXT1 encoder on the same pixels, on the reference photograph's pixels (golden/pnm/test.ppm),
    uniform noise and waves plus noise."""
    from PIL import Image
    images = [("test.ppm", np.frombuffer(PPM[-499 * 289 * 3:], np.uint8).reshape(289, 499, 3)),
              ("noise", D.rng(11).integers(0, 256, (128, 128, 3), dtype=np.uint8)), ("waves", D.waves())]
    for name, x in images:
        ours = D.psnr(D.decode(D.encode(x, D.BC))[5], x)
        buf = io.BytesIO()
        try:
            Image.fromarray(x).save(buf, "DDS", pixel_format="DXT1")
        except (KeyError, OSError, ValueError, TypeError) as e:
            pytest.skip(f"this PIL does not write DXT1: {e}")
        theirs = D.psnr(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")), x)
        print(f"{name}: ours {ours:.2f} dB, PIL {theirs:.2f} dB")
        assert ours >= theirs, (name, ours, theirs)
