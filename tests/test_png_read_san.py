"""ASan + UBSan over the PNG read's chunk walk (icx_pngd_core.h: the host probe's code, which the
device parse and gather kernels run too), through the stand-alone driver tests/san/pngd_san.cpp:
the reference's test.png and crafted files of every colour type, each as it is and under 500
single-byte and truncation damages. A sanitizer report aborts the driver (non-zero exit)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import pngread_util as R

SAN = os.path.join(ROOT, "tests", "san")


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", SAN, "-f", "pngd.mk", "pngd_san"], check=True)
    return os.path.join(SAN, "pngd_san")


def crafted(tmp_path):
    rng = np.random.default_rng(7)
    plte = bytes(rng.integers(0, 256, 48, dtype=np.uint8))
    files = {
        "rgba8": R.make_png(R.random_samples(rng, 9, 7, 8, 6), 8, 6, types=R.filter_types("cycle", 7)),
        "rgb16_key": R.make_png(R.random_samples(rng, 9, 7, 16, 2), 16, 2, trns=bytes(6)),
        "grey2_key": R.make_png(R.random_samples(rng, 9, 7, 2, 0), 2, 0, trns=b"\0\1"),
        "greyalpha8": R.make_png(R.random_samples(rng, 9, 7, 8, 4), 8, 4),
        "pal4_trns": R.make_png(R.random_samples(rng, 9, 7, 4, 3), 4, 3, plte=plte, trns=bytes(5)),
        "pal8_split1": R.make_png(R.random_samples(rng, 19, 17, 8, 3), 8, 3, plte=plte, split=1),
        "ancillary_no_iend": R.make_png(R.random_samples(rng, 5, 5, 8, 0), 8, 0, iend=False,
                                        pre=R.chunk(b"tEXt", b"k\0v") + R.chunk(b"gAMA", bytes(4))),
    }
    paths = []
    for name, data in files.items():
        p = tmp_path / (name + ".png")
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def test_chunk_walk_under_asan_ubsan(driver, tmp_path):
    files = [os.path.join(GOLDEN, "png", "test.png")] + crafted(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, *files], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    assert f"sanitized {len(files)} files ({len(files)} accepted" in r.stdout
