"""The device deflate writer's serial part without a GPU: icx_deflate_core.h (len_code / dist_code,
pad_block_counts, huff_lengths, canon_codes, BitW, token_code) through
tests/cxx/deflate_core_demo.cpp, built with g++ and again with -fsanitize=address,undefined as a
program of its own. The demo calls them in the order thread 0 of the two huff kernels does (that
sequence stays in the kernels, see icx_deflate_core.h; the demo restates it).

The tokens are zlib's own parse of each input (deflate_read.tokens of zlib.compress(data, 6)),
converted to the kernels' uint16 slots. The demo's stream must inflate to the input and pass the
audit the GPU writers' streams pass (deflate_read.audit: complete codes, no unused symbols, the
optimal cost or close to package-merge where a limiter ran, tight headers), with the same
limiter_worst table. The demo itself exits non-zero when huff_lengths gives other code lengths from
its own insertion sort than from the order of a serial restatement of rank_order.

The 7-bit limiter of the code-length code: no input here reaches it (the unlimited code-length
trees printed below are at most 7 deep; a deeper one needs at least 88 code-length symbols with a
Fibonacci-like histogram, which test_gpu_png_deflate.py builds from a 511 x 511 image's own parse).
tests/test_gpu_deflate_pin.py covers that path (png_limiter_7)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
import deflate_read as R


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp("cxx") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cxx", "deflate_core_demo.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    return _build(tmp_path_factory, "deflate_core_demo", [])


@pytest.fixture(scope="module")
def demo_san(tmp_path_factory):
    return _build(tmp_path_factory, "deflate_core_demo_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def slots_of(toks):
    """deflate_read tokens -> the kernels' slots, and the slot index after each token."""
    out, ends = [], []
    for t in toks:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= 32768
            out += [0x4000 | (n - 3), 0x8000 | (d - 1)]
        ends.append(len(out))
    return out, ends


def flat_and_geometric_tail(n, nflat, ratio, top, seed, first=60):
    """test_gpu_exr_write.py's skewed predictor bytes (restated: that module needs the GPU package):
    a tail of counts 1, ratio, ratio^2 .. top and `nflat` values sharing the rest, shuffled."""
    tail, x = [], 1.0
    while round(x) <= top:
        if not tail or round(x) > tail[-1]:
            tail.append(int(round(x)))
        x *= ratio
    cnt = np.array([(n - sum(tail)) // nflat] * nflat + tail[::-1], np.int64)
    cnt[0] += n - cnt.sum()
    v = np.repeat(first + np.arange(len(cnt)), cnt)
    np.random.default_rng(seed).shuffle(v)
    return v


def _jobs():
    """[(name, data, blocks, cap)]: `blocks` deflate blocks of about equal token counts."""
    skew = flat_and_geometric_tail(65536, 64, 1.8, 1000, 50).astype(np.uint8).tobytes()
    noise = np.random.default_rng(51).integers(40, 200, 32768).astype(np.uint8).tobytes()
    return [("one_byte", b"\x2a", 1, 0),
            ("zeros_70000", bytes(70000), 1, 0),
            ("noise_32k", noise, 1, 0),
            ("skewed", skew, 1, 0),
            ("skewed_cap", skew, 1, 1 << 18),
            ("three_blocks", noise[:9000] + bytes(3000) + skew[:9000], 3, 0)]


def run_demo(exe, tmp_path, jobs):
    src, dst = tmp_path / "jobs.bin", tmp_path / "streams.bin"
    with open(src, "wb") as f:
        for slots, ends, cap in jobs:
            f.write(struct.pack("<iiI", len(slots), len(ends), cap))
            f.write(struct.pack("<%di" % len(ends), *ends))
            f.write(np.asarray(slots, np.uint16).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    blob, at, out = dst.read_bytes(), 0, []
    for _ in jobs:
        (size,) = struct.unpack_from("<Q", blob, at)
        out.append(blob[at + 8:at + 8 + size])
        at += 8 + size
    assert at == len(blob)
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_core_streams(which, demo, demo_san, tmp_path):
    exe = demo if which == "plain" else demo_san
    cases, jobs = _jobs(), []
    for name, data, nblocks, cap in cases:
        toks = R.tokens(R.read_zlib(zlib.compress(data, 6)))
        slots, ends = slots_of(toks)
        cut = [ends[len(ends) * (k + 1) // nblocks - 1] for k in range(nblocks)]  # (a block ends after a whole token)
        assert cut[-1] == len(slots) and len(set(cut)) == nblocks
        jobs.append((slots, cut, cap))
    streams = run_demo(exe, tmp_path, jobs)
    by_name = {}
    for (name, data, nblocks, cap), z in zip(cases, streams):
        by_name[name] = z
        assert zlib.decompress(z) == data, name
        blocks = R.read_zlib(z)
        assert [b.final for b in blocks] == [False] * (nblocks - 1) + [True], name  # BFINAL on the last block only
        stats = R.audit(blocks, data, limiter_worst=R.LIMITER_WORST, log=print)
        depth = {c: max(s["depth"] for s in stats if s["code"] == c) for c in ("ll", "d", "cl")}
        print("deflate core:", name, len(z), "bytes, unlimited depths", depth)
        if name.startswith("skewed"):
            assert depth["ll"] > 15 and max(blocks[0].ll_lens) == 15, depth  # the 15-bit limiter ran
    # 65,536 tokens at most: the cap of k_exrw_huff (2^18) does not act, the stream is the same
    assert by_name["skewed_cap"] == by_name["skewed"]
    b = R.read_zlib(by_name["zeros_70000"])[0]
    assert (258, 1) in b.matches() and {d for _, d in b.matches()} == {1}  # length 258, distance 1 only
    assert b.d_lens == [1, 1]  # distance code 0 and the padding
    assert R.read_zlib(by_name["one_byte"])[0].d_lens == [1, 1]  # no match: both forced distance codes


def test_scaling_cap_acts(demo, tmp_path):
    """A cap below the block's token count scales the counts before the codes are built (used
    symbols stay used): still a valid stream of the same bytes with complete codes, no longer
    held to the optimum of its own histogram."""
    data = flat_and_geometric_tail(65536, 64, 1.8, 1000, 50).astype(np.uint8).tobytes()
    slots, ends = slots_of(R.tokens(R.read_zlib(zlib.compress(data, 6))))
    plain, capped = run_demo(demo, tmp_path, [(slots, [len(slots)], 0), (slots, [len(slots)], 1 << 10)])
    assert zlib.decompress(capped) == data and capped != plain
    b = R.read_zlib(capped)[0]
    assert R.kraft(list(b.ll_lens)) == 32768 and R.kraft(list(b.d_lens)) == 32768 and len(capped) >= len(plain)
