#!/usr/bin/env python3
"""Timing aid (GPU box): the OpenEXR write.

N images of S x S RGBA floats resident in HBM through one icx_exr_encode_device_batch per step,
as FLOAT and as HALF files: gigapixels per second over warm-up + repeats (median, min, max), the
files' size against the raw sample bytes and against zlib level 6 on the same predictor bytes
(what tinyexr's compress() produces; measured on the first image), and the share of chunks stored
raw. Input "waves": sines plus noise (tools/exr_time.py's); "smooth": tests/exrw_util.smooth.

Times are a host clock around the call (it synchronises with its stream). --out writes JSON."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imagecodecs_amd as icx  # noqa: E402
import exrw_util as U  # noqa: E402


def make_image(kind, s, k):
    if kind == "smooth":
        return U.smooth(s, s, 4, 100 + k)
    y, x = np.mgrid[0:s, 0:s].astype(np.float32)
    rng = np.random.default_rng(1 + k)
    return np.stack([(np.sin(x * (0.01 + 0.003 * c + 0.001 * k)) * np.cos(y * 0.013) * 50
                      + rng.normal(0, 0.05, (s, s))).astype(np.float32) for c in range(4)], axis=2)


def run(torch, dev, ctx, images, n, s, fp16, warmup, reps):
    srcs = [torch.from_numpy(a).to(dev) for a in images]
    cap = icx.lib().icx_exr_encode_bound(s, s, 4, int(fp16))
    outs = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    sp = [srcs[i % len(srcs)].data_ptr() for i in range(n)]
    op = [outs.data_ptr() + i * cap for i in range(n)]
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        codes, sizes = ctx.exr_encode_device_batch(sp, [s] * n, [s] * n, 4, fp16, op, [cap] * n)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert (codes == 0).all(), codes
    # the first file: the contract, its chunks, zlib -6 on the same predictor bytes
    data = bytes(outs[: int(sizes[0])].cpu().numpy())
    a = images[0]
    nraw = U.check_file(a, fp16, data)
    chunks = U.split(a, fp16, data)[2]
    z6 = raw_bytes = z6_raw = 0
    for kc in range(len(chunks)):
        raw = U.chunk_raw(a, fp16, kc)
        zl = len(zlib.compress(U.predict(raw), 6))
        raw_bytes += len(raw)
        z6 += min(len(raw), zl)
        z6_raw += zl >= len(raw)
    ours = sum(c[1] for c in chunks)
    gp = n * s * s / 1e9
    return {"images": n, "size": s, "fp16": bool(fp16), "ms_median": statistics.median(ms), "ms_min": min(ms),
            "ms_max": max(ms), "gp_per_s_median": gp / statistics.median(ms) * 1e3, "gp_per_s_min": gp / max(ms) * 1e3,
            "gp_per_s_max": gp / min(ms) * 1e3, "file_bytes_mean": float(np.mean(sizes.astype(np.float64))),
            "first_image": {"raw_payload_bytes": raw_bytes, "payload_bytes": ours, "zlib6_payload_bytes": z6,
                            "of_raw": ours / raw_bytes, "zlib6_of_raw": z6 / raw_bytes, "of_zlib6": ours / z6,
                            "chunks": len(chunks), "chunks_stored_raw": nraw,
                            "chunks_raw_under_zlib6": int(z6_raw)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=4, help="distinct source images, cycled over the batch")
    ap.add_argument("--input", default="waves", choices=["waves", "smooth"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exr_write_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    images = [make_image(a.input, a.size, k) for k in range(min(a.distinct, a.images))]
    res = {"input": a.input}
    for fp16 in (False, True):
        key = "half" if fp16 else "float"
        res[key] = run(torch, dev, ctx, images, a.images, a.size, fp16, a.warmup, a.reps)
        print(key, json.dumps(res[key]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
