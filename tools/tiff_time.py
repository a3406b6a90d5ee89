#!/usr/bin/env python3
"""Timing aid (GPU box): the TIFF read.

  * N distinct S x S RGB files per set, written by PIL / libtiff in 64-row strips: uncompressed,
    PackBits, LZW, LZW + predictor 2, Deflate, Deflate + predictor 2; and one set of 256 x 256
    Deflate tiles written here (PIL writes no tiles). The pictures are the synthetic photographs of
    tools/gif_time.py in three channels; --distinct of them are generated and every file is one of
    them rolled by its own amount in both directions, so no two streams are equal. The files are
    left in HBM and read through TiffBatch.decode_device: gigapixels per second over warm-up +
    repeats (median, min, max) and the per-stage split of the last repeat. Every image of the
    batch is compared with the picture it was written from.
  * PIL / libtiff's decode of the first --pil files of each set on one core of the same machine
    (compared with the GPU's pixels too), for context.
  * Next to them the PNG read's figure from profiles/png_read_time.json: one zlib stream per image
    there, one per strip or tile here.

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_tiff_batch_stage_times). --out writes the figures as JSON."""
import argparse
import io
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import imagecodecs_amd as icx  # noqa: E402

SETS = (("none", "raw", 1), ("packbits", "packbits", 1), ("lzw", "tiff_lzw", 1), ("lzw_pred", "tiff_lzw", 2),
        ("deflate", "tiff_adobe_deflate", 1), ("deflate_pred", "tiff_adobe_deflate", 2), ("deflate_tiles256", None, 1))


def rate(gp, ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "gp_per_s_median": gp / statistics.median(ms) * 1e3, "gp_per_s_min": gp / max(ms) * 1e3,
            "gp_per_s_max": gp / min(ms) * 1e3}


def pictures(count, s):
    out = []
    for k in range(count):
        rng = np.random.default_rng(900 + k)
        y, x = np.mgrid[0:s, 0:s]
        planes = [x * rng.uniform(0.05, 0.2) + y * rng.uniform(0.05, 0.2) + rng.normal(0, 5, (s, s)) for _ in range(3)]
        out.append((np.stack(planes, axis=2).astype(np.int64) % 256).astype(np.uint8))
    return out


def tiled_deflate(a, t):
    """A little-endian RGB file of t x t Adobe-Deflate tiles (zlib level 6), tiles padded with zeros."""
    h, w, _ = a.shape
    across, down = -(-w // t), -(-h // t)
    body, offs, cnts = bytearray(), [], []
    for k in range(across * down):
        blk = np.zeros((t, t, 3), np.uint8)
        part = a[(k // across) * t:(k // across + 1) * t, (k % across) * t:(k % across + 1) * t]
        blk[:part.shape[0], :part.shape[1]] = part
        z = zlib.compress(blk.tobytes(), 6)
        offs.append(8 + len(body))
        cnts.append(len(z))
        body += z
    if len(body) & 1:
        body += b"\0"
    arrays = {258: struct.pack("<3H", 8, 8, 8), 324: struct.pack(f"<{len(offs)}I", *offs), 325: struct.pack(f"<{len(cnts)}I", *cnts)}
    at = {}
    for tag, raw in arrays.items():
        at[tag] = 8 + len(body)
        body += raw
    ent = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 3, at[258]), (259, 3, 1, 8), (262, 3, 1, 2), (277, 3, 1, 3), (284, 3, 1, 1),
           (322, 4, 1, t), (323, 4, 1, t), (324, 4, len(offs), at[324]), (325, 4, len(cnts), at[325])]
    ifd = struct.pack("<H", len(ent)) + b"".join(struct.pack("<HHII", *e) for e in ent) + struct.pack("<I", 0)
    return b"II" + struct.pack("<HI", 42, 8 + len(body)) + bytes(body) + ifd


_BASE = {}


def source(i, s, distinct):
    """Picture i: one of `distinct` generated pictures, rolled by its own amount."""
    k, r = i % distinct, i // distinct
    if (k, s) not in _BASE:
        _BASE[(k, s)] = pictures(k + 1, s)[k]
    return np.roll(_BASE[(k, s)], (13 * r, 29 * r), (0, 1))


def write_file(job):
    """(i, compression, predictor, size, distinct, rows per strip) -> the file's bytes. Runs in worker
    processes that never touch the GPU (started before it is initialised)."""
    i, comp, pred, s, distinct, rps = job
    a = source(i, s, distinct)
    if comp is None:
        return tiled_deflate(a, 256)
    from PIL import Image
    b = io.BytesIO()
    info = {278: rps}
    if pred == 2:
        info[317] = 2
    Image.fromarray(a, "RGB").save(b, "TIFF", compression=comp, tiffinfo=info)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--rows-per-strip", type=int, default=64)
    ap.add_argument("--pil", type=int, default=16, help="files per set also decoded by PIL on one core")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--jobs", type=int, default=8, help="processes that write the files")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import multiprocessing
    pool = multiprocessing.get_context("fork").Pool(a.jobs)  # (before the GPU is initialised)
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        sys.exit("tiff_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    res = {}
    png = os.path.join(ROOT, "profiles", "png_read_time.json")
    if os.path.exists(png):
        p = json.load(open(png))["batch"]
        res["png_read_for_comparison"] = {"file": "profiles/png_read_time.json", "images": p["images"], "width": p["width"],
                                          "height": p["height"], "gp_per_s_median": p["mp_per_s_median"] / 1e3}
    distinct = min(a.distinct, n)
    src = [source(i, s, distinct) for i in range(n)]
    for name, comp, pred in SETS:
        files = pool.map(write_file, [(i, comp, pred, s, distinct, a.rows_per_strip) for i in range(n)], chunksize=4)
        sizes = np.array([len(f) for f in files], np.int64)
        offs = np.zeros(n, np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        data = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to(dev)
        d_off, d_sz = torch.from_numpy(offs).to(dev), torch.from_numpy(sizes).to(dev)
        stride = 4 * s * s
        out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
        b = icx.TiffBatch(ctx, n, s, s)
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
        assert (st.cpu().numpy() == icx.TIFF_OK).all(), st.cpu().numpy()
        got = out.cpu().numpy().reshape(n, stride)[:, :3 * s * s].reshape(n, s, s, 3)
        for i in range(n):
            assert (got[i] == src[i]).all(), f"{name} image {i} differs from its source"
        pil_ms = []
        for i, f in enumerate(files[:a.pil]):
            t0 = time.perf_counter()
            im = Image.open(io.BytesIO(f))
            im.load()
            pil_ms.append((time.perf_counter() - t0) * 1e3)
            assert (np.asarray(im) == got[i]).all(), f"{name} image {i} differs from PIL's decode"
        gp = n * s * s / 1e9
        r = {"images": n, "width": s, "height": s, "chunks_per_image": int((-(-s // 256)) ** 2 if comp is None else -(-s // a.rows_per_strip)),
             "file_bytes_mean": float(np.mean(sizes)), "stage_ms_last_repeat": stages,
             "stage_gp_per_s": {k: gp / v * 1e3 for k, v in stages.items() if v > 0},
             "bounding_stage": max(stages, key=stages.get),
             "pil_one_core": {"files": len(pil_ms), "ms_per_image_median": statistics.median(pil_ms),
                              "gp_per_s": s * s / 1e9 / statistics.median(pil_ms) * 1e3}}
        r.update(rate(gp, ms))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del data, out, got
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()
    pool.close()
    pool.join()


if __name__ == "__main__":
    main()
