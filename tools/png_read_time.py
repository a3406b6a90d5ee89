#!/usr/bin/env python3
"""Timing aid (GPU box): the PNG read.

  * batch: N files of S x S RGBA (tests/pngutil.synth_rgba, encoded on the box by
    PngEncoder.encode_device_batch and left in HBM) through PngBatch.decode_device: megapixels per
    second over warm-up + repeats (median, min, max) and the per-stage split of the last repeat.
  * single: one file of T x T, to show what one wave's inflate costs.
  * PIL on one core of the same machine for context, if PIL is there.

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_png_batch_stage_times). --out writes the figures as JSON."""
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


def encode_on_device(torch, dev, ctx, images, n, w, h):
    """n files from the distinct source `images` (cycled) -> (device buffer, stride, sizes)."""
    srcs = [torch.from_numpy(px.reshape(-1)).to(dev) for px in images]
    stride = (4 * w * h + 4 * h + (1 << 16) + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    enc = icx.PngEncoder(ctx)
    torch.cuda.synchronize(dev)
    status, sizes = enc.encode_device_batch(w, h, 4, [srcs[i % len(srcs)].data_ptr() for i in range(n)],
                                            files.data_ptr(), stride)
    torch.cuda.synchronize(dev)
    enc.close()
    assert (status == icx.OK).all(), status
    return files, stride, sizes


def time_batch(torch, dev, ctx, files, stride, sizes, n, w, h, warmup, reps, images):
    d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int64)).to(dev)
    out_stride = 4 * w * h
    out = torch.zeros(n * out_stride, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    b = icx.PngBatch(ctx, n, w, h)
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
    assert (st.cpu().numpy() == icx.PNGR_OK).all(), st.cpu().numpy()
    for i in (0, n - 1):  # the decode gives back the encoder's input
        got = out[i * out_stride:(i + 1) * out_stride].cpu().numpy()
        assert np.array_equal(got, images[i % len(images)].reshape(-1)), f"image {i} differs from its source"
    b.close()
    mp = n * w * h / 1e6
    return {"images": n, "width": w, "height": h, "file_bytes_mean": float(np.mean(sizes)),
            "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "mp_per_s_median": mp / statistics.median(ms) * 1e3, "mp_per_s_min": mp / max(ms) * 1e3,
            "mp_per_s_max": mp / min(ms) * 1e3, "stage_ms_last_repeat": stages,
            "bounding_stage": max(stages, key=stages.get)}


def time_pil(data, w, h, reps=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        Image.open(io.BytesIO(data)).convert("RGBA").load()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": w * h / 1e6 / statistics.median(ms) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--single", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=8, help="distinct source images, cycled over the batch")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("png_read_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    res = {}
    n, s = a.images, a.size
    images = [P.synth_rgba(40 + k, s, s) for k in range(min(a.distinct, n))]
    files, stride, sizes = encode_on_device(torch, dev, ctx, images, n, s, s)
    res["batch"] = time_batch(torch, dev, ctx, files, stride, sizes, n, s, s, a.warmup, a.reps, images)
    print("batch ", json.dumps(res["batch"]), flush=True)
    pil = time_pil(bytes(files[: int(sizes[0])].cpu().numpy()), s, s)
    if pil:
        res["pil_one_core"] = pil
        print("pil   ", json.dumps(pil), flush=True)
    del files
    if a.single > 0:
        t = a.single
        big = np.ascontiguousarray(np.tile(images[0], (-(-t // s), -(-t // s), 1))[:t, :t])
        f1, stride1, sizes1 = encode_on_device(torch, dev, ctx, [big], 1, t, t)
        res["single"] = time_batch(torch, dev, ctx, f1, stride1, sizes1, 1, t, t, 1, max(2, a.reps // 2), [big])
        print("single", json.dumps(res["single"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
