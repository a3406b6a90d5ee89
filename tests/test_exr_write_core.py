"""The OpenEXR write without a GPU: icx_exrw_core.h (float_to_half_full, chunk sample bytes,
CompressZip's reorder + predictor, the header) compiled with g++ into tests/cxx/exrw_core_demo.cpp,
against the numpy restatement in tests/exrw_util.py and against tinyexr's own files under
tests/golden/exrw; and the restatement pinned to the reference where its library is built."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
import exrw_util as U

CASES = sorted(U.golden_cases())


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cxx") / "exrw_core_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "exrw_core_demo.cpp"), "-o", exe], check=True)
    return exe


def test_half_edge_table(demo, tmp_path):
    """float_to_half_full on the edge table (+ seeded random patterns) equals the restatement; a few
    values are spelled out so that the restatement cannot drift with the code."""
    rng = np.random.default_rng(11)
    bits = np.concatenate([U.HALF_EDGES, rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    p = tmp_path / "bits.bin"
    p.write_bytes(bits.astype("<u4").tobytes())
    r = subprocess.run([demo, "half", str(p)], capture_output=True, text=True, check=True)
    got = np.array([int(x, 16) for x in r.stdout.split()], np.uint16)
    assert (got == U.half_full(bits)).all()
    known = {0x00000001: 0x0000, 0x807FFFFF: 0x8000, 0x33800000: 0x0001, 0x33000000: 0x0001, 0x32800000: 0x0000,
             0x387FFFFF: 0x0400, 0x38800000: 0x0400, 0x3F801000: 0x3C01, 0x3F803000: 0x3C02, 0x3F800FFF: 0x3C00,
             0x3FFFF000: 0x4000, 0x477FE000: 0x7BFF, 0x477FF000: 0x7C00, 0x49742400: 0x7C00, 0xFF800000: 0xFC00,
             0x7F800001: 0x7E00, 0xFFC00001: 0xFE00}
    for f, h in known.items():
        assert int(U.half_full(np.array([f], np.uint32))[0]) == h, hex(f)


@pytest.mark.parametrize("name", CASES)
def test_core_matches_restatement_and_golden(demo, tmp_path, name):
    """Header, sample bytes and predictor bytes of every chunk: the C++ core == numpy == tinyexr's
    file (its raw payloads, and its compressed payloads after zlib.decompress)."""
    a, fp16, gold = U.load_golden(name)
    h, w, c = a.shape
    p = tmp_path / "in.bin"
    p.write_bytes(np.ascontiguousarray(a, np.float32).view(np.uint32).astype("<u4").tobytes())
    r = subprocess.run([demo, "chunks", str(p), str(w), str(h), str(c), str(int(fp16))], capture_output=True, text=True,
                       check=True)
    lines = r.stdout.splitlines()
    assert bytes.fromhex(lines[0].split()[1]) == U.header(a, fp16)
    ghdr, goffs, gch = U.split(a, fp16, gold)
    assert ghdr == U.header(a, fp16)
    S_all = sum(len(U.chunk_raw(a, fp16, k)) for k in range(len(gch)))
    assert int(lines[1].split()[1]) == len(ghdr) + 16 * len(gch) + S_all
    zipc = U.geometry(a, fp16)[5]
    for k, (y, size, payload, at) in enumerate(gch):
        raw = bytes.fromhex(lines[2 + 2 * k].split()[2])
        pred = bytes.fromhex(lines[3 + 2 * k].split()[2])
        assert raw == U.chunk_raw(a, fp16, k)
        assert pred == U.predict(raw)
        assert goffs[k] == at and y == k * U.geometry(a, fp16)[4]
        if not zipc or size == len(raw):
            assert payload == raw
        else:
            assert zlib.decompress(payload) == pred


def test_goldens_are_what_the_cases_say():
    """The committed inputs have the cases' shapes (and their bits where no libm is involved), the all-raw case
    is all raw in tinyexr's file (8448, 8448 and 4224 bytes), and every golden file stays small."""
    man = U.load_manifest()
    assert sorted(man) == CASES
    for name, (make, fp16) in U.golden_cases().items():
        a, gfp16, gold = U.load_golden(name)
        assert gfp16 == fp16 and a.dtype == np.float32
        b = make()
        assert a.shape == b.shape, name
        if name in ("raw_33x40_rgba", "half_edges_64x16_rgba"):  # (no libm in these two: bit for bit)
            assert (a.view(np.uint32) == b.view(np.uint32)).all(), name
        assert len(gold) < 64 * 1024 and a.nbytes < 64 * 1024
    a, fp16, gold = U.load_golden("raw_33x40_rgba")
    assert [c[1] for c in U.split(a, fp16, gold)[2]] == [8448, 8448, 4224]
    # the smooth ZIP cases are ones tinyexr compresses
    for name in ("zip_33x20_rgba", "zip_33x17_rgb_half", "zip_16x17_a"):
        a, fp16, gold = U.load_golden(name)
        assert all(c[1] < len(U.chunk_raw(a, fp16, k)) for k, c in enumerate(U.split(a, fp16, gold)[2])), name


@pytest.mark.skipif(not os.path.exists(U.REFLIB), reason="the reference's tinyexr is not built here")
@pytest.mark.parametrize("name", CASES)
def test_reference_pin(name):
    """Regenerating a golden from its .npy with the reference's SaveEXRToMemory gives the committed
    bytes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_exr_write_goldens as G
    a, fp16, gold = U.load_golden(name)
    assert G.ref_save(a, fp16) == gold
