#!/usr/bin/env python3
"""Timing aid (GPU box): the Radiance .hdr write.

  * N images of S x S pixels (tools/synth.c synth_rgbe turned into the read's floats on the device;
    --distinct pictures are generated and every image of the batch is one of them with its rows
    rotated by a different amount, so each has its own N-th of the input in HBM and no two files
    are equal) are written on the box by Context.hdr_encode_device_batch, d = 4 and d = 3, flat and
    run-length coded, and left in HBM: gigapixels per second over warm-up + repeats (median, min,
    max). Image 0 of every d = 4 batch is read back through icx_hdr_decode and must give its source.
  * For the flat form, the algorithmic bytes (4*d in, 4 out per pixel) over the call's time as a
    share of the 8 TB/s HBM peak.
  * For the run-length form, the payload against the flat payload; the same for tests/golden/test.hdr,
    there also against the file's own size.
  * The serial core (icx_hdrw_core.h, tests/cxx/hdrw_core_demo.cpp built with g++ -O2) on one core of
    the same machine, on image 0 of the same batch (its file has the GPU file's size), for context.

Times are a host clock around the call, which synchronises with its stream. --out writes the
figures as JSON."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imagecodecs_amd as icx  # noqa: E402
import hdrutil as H  # noqa: E402
from tools import synthpy as S  # noqa: E402

HBM_PEAK = 8e12  # bytes per second (MI355X specification)
READ_GP_S = {"rle": 126, "flat": 169}  # the read of the same batch (README: Radiance .hdr read)


def rate(gp, ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "gp_per_s_median": gp / statistics.median(ms) * 1e3, "gp_per_s_min": gp / max(ms) * 1e3,
            "gp_per_s_max": gp / min(ms) * 1e3}


def floats_on_device(torch, dev, rgbe):
    """The read's formula, v = m * 2^(E - 136) and E as a float (numpy, exact) -> (h, w, 4) float32 in HBM."""
    return torch.from_numpy(H.expected_floats(rgbe)).to(dev)


def encode_on_device(torch, dev, ctx, srcs, n, w, h, d, rle, warmup, reps):
    stride = (icx.hdr_encode_bound(w, h, d, rle) + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    ptrs = [s.data_ptr() for s in srcs]
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        rc = ctx.hdr_encode_device_batch(ptrs, [w] * n, [h] * n, d, rle, files.data_ptr(), stride, sizes.data_ptr(),
                                         status.data_ptr())  # (synchronises)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == icx.HDR_OK
    assert (status.cpu().numpy() == icx.HDR_OK).all(), status.cpu().numpy()
    return files, stride, sizes.cpu().numpy(), rate(n * w * h / 1e9, ms)


def cpu_baseline(px, rle, reps=3):
    """The serial core on one core over `px` (h, w, d) float32, the batch's image 0 -> ms, rate, file size."""
    h, w, d = px.shape
    with tempfile.TemporaryDirectory(prefix="hdrw_") as tmp:
        exe, job = os.path.join(tmp, "hdrw_core_demo"), os.path.join(tmp, "job.bin")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cxx", "hdrw_core_demo.cpp"), "-o", exe], check=True)
        with open(job, "wb") as f:
            f.write(np.array([w, h, d, int(rle)], np.int32).tobytes())
            f.write(np.ascontiguousarray(px, np.float32).tobytes())
        r = subprocess.run([exe, "time", job, str(reps)], capture_output=True, text=True, check=True)
    ms, size = r.stdout.split()
    return {"ms": float(ms), "gp_per_s": w * h / 1e9 / float(ms) * 1e3, "file_bytes": int(size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=4, help="generated pictures; each image is one with its rows rotated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hdr_write_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    res = {}
    n, s = a.images, a.size
    base = [floats_on_device(torch, dev, S.rgbe(60 + k, s, s)) for k in range(min(a.distinct, n))]
    for d in (4, 3):
        srcs = [torch.roll(base[i % len(base)], 7 * (i // len(base)), 0)[..., :d].contiguous() for i in range(n)]
        if d == 3:
            del base
        for rle in (False, True):
            key = f"d{d}_{'rle' if rle else 'flat'}"
            files, stride, sizes, r = encode_on_device(torch, dev, ctx, srcs, n, s, s, d, rle, a.warmup, a.reps)
            r.update({"images": n, "width": s, "height": s, "file_bytes_mean": float(np.mean(sizes)),
                      "read_gp_per_s_for_comparison": READ_GP_S["rle" if rle else "flat"]})
            head = len(b"#?RADIANCE\nSOFTWARE=GEGL\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (s, s))
            if rle:
                r["payload_over_flat_payload"] = float(np.mean(sizes) - head) / (4.0 * s * s)
            else:
                moved = n * s * s * (4.0 * d + 4.0)
                r["algorithmic_bytes"] = moved
                r["share_of_hbm_peak_median"] = moved / (r["ms_median"] * 1e-3) / HBM_PEAK
            if d == 4:  # the read gives the source back
                code, w2, h2, rows, px = ctx.hdr_decode(bytes(files[: int(sizes[0])].cpu().numpy()))
                assert (code, w2, h2, rows) == (icx.HDR_OK, s, s, s)
                assert px.tobytes() == srcs[0].cpu().numpy().tobytes(), "image 0 does not read back as its source"
            cpu = cpu_baseline(srcs[0].cpu().numpy().reshape(s, s, d), rle)
            assert cpu["file_bytes"] == int(sizes[0]), "the serial core's file of image 0 has another size than the GPU's"
            r["cpu_serial_core_one_core"] = cpu
            res[key] = r
            print(key, json.dumps(r), flush=True)
            del files
        del srcs
    fx = open(os.path.join(ROOT, "tests", "golden", "test.hdr"), "rb").read()
    code, w, h, rows, px = ctx.hdr_decode(fx)
    _, flat = ctx.hdr_encode(px, False)
    _, packed = ctx.hdr_encode(px, True)
    head = len(flat) - 4 * w * h
    res["test_hdr"] = {"width": w, "height": h, "file_bytes": len(fx), "flat_bytes": len(flat), "rle_bytes": len(packed),
                       "payload_over_flat_payload": (len(packed) - head) / (4.0 * w * h),
                       "rle_over_file": len(packed) / len(fx), "flat_equals_file": flat == fx}
    print("test_hdr", json.dumps(res["test_hdr"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
