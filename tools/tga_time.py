#!/usr/bin/env python3
"""Timing aid (GPU box): the Targa read and write.

  * N images of S x S RGBA (tests/pngutil.synth_rgba: "plain", and "runs" = the same quantised to
    8 levels per channel, which gives real runs; --distinct pictures are generated and every
    image of the batch is one of them with its rows rotated by a different amount, so each has its
    own N-th of the input in HBM and no two files are equal) are packed on the box by
    Context.tga_encode_device_batch, raw and run-length coded, left in HBM and read back through
    TgaBatch.decode_device: megapixels per second over warm-up + repeats (median, min, max) and
    the per-stage split of the last repeat. The encode is timed the same way.
  * For the raw read, the bytes the streaming kernel must move (file in, pixels out) over its stage
    time, as a share of the 8 TB/s HBM peak.
  * PIL on one core of the same machine for context, if PIL is there.

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_tga_batch_stage_times). --out writes the figures as JSON."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imagecodecs_amd as icx  # noqa: E402
import pngutil as P  # noqa: E402

HBM_PEAK = 8e12  # bytes per second (MI355X specification)


def rate(mp, ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "mp_per_s_median": mp / statistics.median(ms) * 1e3, "mp_per_s_min": mp / max(ms) * 1e3,
            "mp_per_s_max": mp / min(ms) * 1e3}


def encode_on_device(torch, dev, ctx, srcs, n, w, h, rle, warmup, reps):
    """n files from the n device images `srcs` -> (device buffer, stride, sizes, timing)."""
    stride = (icx.tga_encode_bound(w, h, 4) + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    ptrs = [s.data_ptr() for s in srcs]
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        rc = ctx.tga_encode_device_batch(ptrs, [w] * n, [h] * n, 4, rle, files.data_ptr(), stride, sizes.data_ptr(),
                                         status.data_ptr())  # (synchronises)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == icx.TGA_OK
    assert (status.cpu().numpy() == icx.TGA_OK).all(), status.cpu().numpy()
    return files, stride, sizes.cpu().numpy(), rate(n * w * h / 1e6, ms)


def time_batch(torch, dev, ctx, files, stride, sizes, n, w, h, warmup, reps, srcs):
    d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int64)).to(dev)
    out_stride = 4 * w * h
    out = torch.zeros(n * out_stride, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    b = icx.TgaBatch(ctx, n, w, h)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        b.decode_device(n, files.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), out_stride,
                        st.data_ptr(), dims.data_ptr())
        torch.cuda.synchronize(dev)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    stages = b.stage_times()
    assert (st.cpu().numpy() == icx.TGA_OK).all(), st.cpu().numpy()
    for i in range(n):  # the decode gives back the encoder's input, every image of the batch
        assert torch.equal(out[i * out_stride:(i + 1) * out_stride], srcs[i]), f"image {i} differs from its source"
    b.close()
    res = {"images": n, "width": w, "height": h, "file_bytes_mean": float(np.mean(sizes)),
           "stage_ms_last_repeat": stages, "bounding_stage": max(stages, key=stages.get)}
    res.update(rate(n * w * h / 1e6, ms))
    return res


def time_pil(data, w, h, reps=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        Image.open(io.BytesIO(data)).load()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": w * h / 1e6 / statistics.median(ms) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8, help="generated pictures; each image is one with its rows rotated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tga_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    res = {}
    n, s = a.images, a.size
    plain = [P.synth_rgba(40 + k, s, s) for k in range(min(a.distinct, n))]
    kinds = {"plain": plain, "runs": [np.ascontiguousarray(px & 0xE0) for px in plain]}
    for kind, images in kinds.items():
        base = [torch.from_numpy(px.reshape(s, s * 4)).to(dev) for px in images]
        srcs = [torch.roll(base[i % len(base)], 7 * (i // len(base)), 0).reshape(-1).contiguous() for i in range(n)]
        for rle in (False, True):
            if kind == "runs" and not rle:
                continue  # (the raw path does not look at the pixels)
            key = f"{kind}_{'rle' if rle else 'raw'}"
            files, stride, sizes, enc = encode_on_device(torch, dev, ctx, srcs, n, s, s, rle, a.warmup, a.reps)
            r = time_batch(torch, dev, ctx, files, stride, sizes, n, s, s, a.warmup, a.reps, srcs)
            r["encode"] = enc
            if not rle:
                moved = float(np.sum(sizes)) + n * s * s * 4.0
                t = r["stage_ms_last_repeat"]["raw"] * 1e-3
                r["raw_stage_bytes_moved"] = moved
                r["raw_stage_share_of_hbm_peak"] = moved / t / HBM_PEAK
            pil = time_pil(bytes(files[: int(sizes[0])].cpu().numpy()), s, s)
            if pil:
                r["pil_one_core"] = pil
            res[key] = r
            print(key, json.dumps(r), flush=True)
            del files
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
