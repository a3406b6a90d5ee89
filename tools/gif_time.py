#!/usr/bin/env python3
"""Timing aid (GPU box): the GIF read.

  * N distinct S x S files of two kinds, written by PIL: "photo" (a 256-colour picture of
    gradients plus noise: LZW strings of 1-3 bytes) and "graphics" (flat rectangles in 16 colours:
    strings of hundreds of bytes). --distinct pictures are generated per kind and every file is
    one of them rolled by its own amount in both directions, so no two streams are equal. The
    files are left in HBM and read through GifBatch.decode_device: megapixels per second over
    warm-up + repeats (median, min, max) and the per-stage split of the last repeat. Every image
    of the batch is compared with PIL's decode.
  * PIL's decode of the same files on one core of the same machine, for context.

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_gif_batch_stage_times). --out writes the figures as JSON."""
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
import imagecodecs_amd as icx  # noqa: E402


def rate(mp, ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "mp_per_s_median": mp / statistics.median(ms) * 1e3, "mp_per_s_min": mp / max(ms) * 1e3,
            "mp_per_s_max": mp / min(ms) * 1e3}


def pictures(kind, count, s):
    out = []
    for k in range(count):
        rng = np.random.default_rng(900 + k)
        if kind == "photo":
            y, x = np.mgrid[0:s, 0:s]
            v = x * rng.uniform(0.05, 0.2) + y * rng.uniform(0.05, 0.2) + rng.normal(0, 5, (s, s))
            out.append((v.astype(np.int64) % 256).astype(np.uint8))
        else:
            a = np.zeros((s, s), np.uint8)
            for _ in range(150):
                x0, y0 = (int(v) for v in rng.integers(0, s, 2))
                w, h = (int(v) for v in rng.integers(s // 32, s // 3, 2))
                a[y0:y0 + h, x0:x0 + w] = rng.integers(0, 16)
            out.append(a)
    return out


def write_files(Image, kind, n, s, distinct, interlace):
    base = pictures(kind, min(distinct, n), s)
    pal = np.random.default_rng(5).integers(0, 256, 768, dtype=np.uint8).tobytes()
    files = []
    for i in range(n):
        k, r = i % len(base), i // len(base)
        im = Image.fromarray(np.roll(base[k], (13 * r, 29 * r), (0, 1)), "P")
        im.putpalette(pal)
        b = io.BytesIO()
        im.save(b, "GIF", interlace=bool(interlace))
        files.append(b.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--interlace", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        sys.exit("gif_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    res = {"png_read_mp_per_s_for_comparison": 625.0}
    for kind in ("photo", "graphics"):
        files = write_files(Image, kind, n, s, a.distinct, a.interlace)
        sizes = np.array([len(f) for f in files], np.int64)
        offs = np.zeros(n, np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        data = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev)
        d_off, d_sz = torch.from_numpy(offs).to(dev), torch.from_numpy(sizes).to(dev)
        stride = 3 * s * s
        out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
        b = icx.GifBatch(ctx, n, s, s)
        torch.cuda.synchronize(dev)
        ms = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            b.decode_device(n, data.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), stride, st.data_ptr(),
                            dims.data_ptr())
            torch.cuda.synchronize(dev)
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        stages = b.stage_times()
        b.close()
        assert (st.cpu().numpy() == icx.GIF_OK).all(), st.cpu().numpy()
        got = out.cpu().numpy().reshape(n, s, s, 3)
        pil_ms = []
        for i, f in enumerate(files):
            t0 = time.perf_counter()
            im = Image.open(io.BytesIO(f))
            im.load()
            pil_ms.append((time.perf_counter() - t0) * 1e3)
            assert (np.asarray(im.convert("RGB")) == got[i]).all(), f"{kind} image {i} differs from PIL's decode"
        r = {"images": n, "width": s, "height": s, "interlaced": bool(a.interlace), "file_bytes_mean": float(np.mean(sizes)),
             "stage_ms_last_repeat": stages, "bounding_stage": max(stages, key=stages.get),
             "pil_one_core": {"ms_per_image_median": statistics.median(pil_ms),
                              "mp_per_s": s * s / 1e6 / statistics.median(pil_ms) * 1e3}}
        r.update(rate(n * s * s / 1e6, ms))
        res[kind] = r
        print(kind, json.dumps(r), flush=True)
        del data, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
