#!/usr/bin/env python3
"""Timing aid (GPU box): the BMP read and write, beside the Targa read of the same session.

  * N files of S x S per form, built on the host (tests/bmputil.py) and left in HBM, read through
    BmpBatch.decode_device: megapixels per second over warm-up + repeats (median, min, max) and the
    per-stage split of the last repeat. Raw forms (24-bit, 8-bit paletted, 1-bit, 16-bit 5-6-5,
    32-bit bitfields with alpha) hold random raster bytes: the raw path does not look at them.
    --distinct rasters are generated and every file is one of them with its rows rotated.
  * RLE8 on the two index pictures tools/gif_time.py uses, "photo" (gradients plus noise) and "flat"
    (rectangles in 16 colours), rows coded as run packets (a run of one pixel where neighbours
    differ: "photo_runs" is close to a packet per pixel, the most packets a stream of that size can
    hold); "photo_literal" is the photo with every row as absolute packets of 255 pixels.
  * The write for d = 3 and d = 4 from random pixels in HBM (Context.bmp_encode_device_batch).
  * In the same session the raw (d = 3) and run-length (tools/tga_time.py's "runs" RGBA) Targa read,
    each timed twice: the difference of the two medians is the session's spread, and
    "bmp24_vs_tga_raw" says whether the 24-bit BMP read is slower than the raw Targa read by more.
  * One core of the same machine: PIL, and the serial core (tests/cxx/bmp_core_demo.cpp built with
    g++ -O2; a process that decodes the file twice, less one that decodes it once).

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_bmp_batch_stage_times). --out writes the figures as JSON."""
import argparse
import io
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import imagecodecs_amd as icx  # noqa: E402
import bmputil as B  # noqa: E402
import pngutil as P  # noqa: E402
import gif_time as G  # noqa: E402

HBM_PEAK = 8e12  # bytes per second (MI355X specification)


def rate(mp, ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "mp_per_s_median": mp / statistics.median(ms) * 1e3, "mp_per_s_min": mp / max(ms) * 1e3,
            "mp_per_s_max": mp / min(ms) * 1e3}


def raw_files(bits, n, s, distinct, **form):
    """n files of one raw form: `distinct` random rasters, each file one of them with its rows rotated."""
    first = B.raw_file(500 + bits, bits, s, s, **form)
    off = int.from_bytes(first[10:14], "little")
    stride = (len(first) - off) // s
    base = [np.random.default_rng(600 + k).integers(0, 256, (s, stride), dtype=np.uint8) for k in range(min(distinct, n))]
    return [first[:off] + np.roll(base[i % len(base)], 7 * (i // len(base)), 0).tobytes() for i in range(n)]


def rle8_rows_runs(a):
    """Every row of the index picture as run packets (n, v), n <= 255, and an end-of-line."""
    rows = []
    for r in a[::-1]:  # bottom row first
        start = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
        length = np.diff(np.concatenate((start, [r.size])))
        parts = (length + 254) // 255  # a run longer than 255 is cut
        v = np.repeat(r[start], parts)
        n = np.full(v.size, 255, np.int64)
        last = np.cumsum(parts) - 1
        n[last] = length - 255 * (parts - 1)
        rows.append(np.stack([n.astype(np.uint8), v], 1).tobytes() + B.EOL)
    return rows


def rle8_rows_literal(a):
    rows = []
    for r in a[::-1]:
        rows.append(b"".join(B.lit(r[x:x + 255].tolist(), 8) if r.size - x >= 3 else b"".join(B.run(1, int(v)) for v in r[x:])
                             for x in range(0, r.size, 255)) + B.EOL)
    return rows


def rle8_files(kind, n, s, distinct):
    pics = G.pictures("photo" if kind.startswith("photo") else "graphics", min(distinct, n), s)
    coded = [(rle8_rows_literal if kind == "photo_literal" else rle8_rows_runs)(p) for p in pics]
    files = []
    for i in range(n):
        rows, r = coded[i % len(coded)], (11 * (i // len(coded))) % s
        files.append(B.rle_file(8, s, s, b"".join(rows[r:] + rows[:r]) + B.EOB, seed=3))
    return files


def upload(torch, dev, files):
    stride = (max(len(f) for f in files) + 255) & ~255
    host = np.zeros((len(files), stride), np.uint8)
    for i, f in enumerate(files):
        host[i, :len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(host.reshape(-1)).to(dev), stride, np.array([len(f) for f in files], np.int64)


def time_batch(torch, dev, batch_cls, ok, ctx, blob, stride, sizes, n, w, h, warmup, reps, check=None):
    d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int64)).to(dev)
    out_stride = 4 * w * h
    out = torch.zeros(n * out_stride, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    b = batch_cls(ctx, n, w, h)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        b.decode_device(n, blob.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), out_stride,
                        st.data_ptr(), dims.data_ptr())
        torch.cuda.synchronize(dev)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    stages = b.stage_times()
    assert (st.cpu().numpy() == ok).all(), st.cpu().numpy()
    if check is not None:  # image 0 and the last one against the restatement
        for i in (0, n - 1):
            want = B.decode(check[i])[4]
            got = out[i * out_stride:i * out_stride + want.size].cpu().numpy()
            assert (got == want.reshape(-1)).all(), f"image {i} differs from the restatement"
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
        try:
            Image.open(io.BytesIO(data)).load()
        except OSError:
            return None  # (a form PIL does not read)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": w * h / 1e6 / statistics.median(ms) * 1e3}


def time_serial_core(datas, w, h):
    """{form: one bmp_decode_serial}: a process that decodes the file twice, less one that decodes it once."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bmp_core_demo")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cxx", "bmp_core_demo.cpp"), "-o", exe], check=True)
        for form, data in datas.items():
            path = os.path.join(tmp, "f.bmp")
            open(path, "wb").write(data)
            t = []
            for k in (1, 2):
                open(os.path.join(tmp, "list.txt"), "w").write((path + "\n") * k)
                best = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    subprocess.run([exe, "decode", os.path.join(tmp, "list.txt"), os.path.join(tmp, "out.bin")], check=True,
                                   stdout=subprocess.DEVNULL)
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                t.append(best)
            ms = max(t[1] - t[0], 1e-3)
            out[form] = {"ms": ms, "mp_per_s": w * h / 1e6 / ms * 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8, help="generated pictures; each image is one with its rows rotated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bmp_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    res = {"read": {}, "write": {}, "targa_same_session": {}, "cpu_one_core": {"pil": {}}}
    host_first = {}
    forms = {"raw24": lambda: raw_files(24, n, s, a.distinct), "pal8": lambda: raw_files(8, n, s, a.distinct),
             "mono1": lambda: raw_files(1, n, s, a.distinct),
             "rgb565": lambda: raw_files(16, n, s, a.distinct, comp=3, masks=B.M565),
             "bitfields32": lambda: raw_files(32, n, s, a.distinct, hs=108, comp=3, masks=B.M8888),
             "rle8_photo_runs": lambda: rle8_files("photo_runs", n, s, a.distinct),
             "rle8_photo_literal": lambda: rle8_files("photo_literal", n, s, a.distinct),
             "rle8_flat": lambda: rle8_files("flat", n, s, a.distinct)}
    for form, make in forms.items():
        files = make()
        host_first[form] = files[0]
        blob, stride, sizes = upload(torch, dev, files)
        r = time_batch(torch, dev, icx.BmpBatch, icx.BMP_OK, ctx, blob, stride, sizes, n, s, s, a.warmup, a.reps, files)
        if not form.startswith("rle8"):
            d = B.probe(files[0])[3]
            moved = float(np.sum(sizes)) + n * s * s * float(d)
            r["raw_stage_bytes_moved"] = moved
            r["raw_stage_share_of_hbm_peak"] = moved / (r["stage_ms_last_repeat"]["raw"] * 1e-3) / HBM_PEAK
        pil = time_pil(files[0], s, s)
        if pil:
            res["cpu_one_core"]["pil"][form] = pil
        res["read"][form] = r
        print(form, json.dumps(r), flush=True)
        del blob, files
    res["cpu_one_core"]["serial_core"] = time_serial_core(host_first, s, s)
    print("serial_core", json.dumps(res["cpu_one_core"]["serial_core"]), flush=True)

    # the write, and the Targa reads of the same session (raw d = 3 from the same pixels)
    for d in (3, 4):
        base = [torch.randint(0, 256, (s, s * d), dtype=torch.uint8, device=dev) for _ in range(min(a.distinct, n))]
        srcs = [torch.roll(base[i % len(base)], 7 * (i // len(base)), 0).reshape(-1).contiguous() for i in range(n)]
        stride = (icx.bmp_encode_bound(s, s, d) + 255) & ~255
        files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
        status = torch.full((n,), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ms = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            rc = ctx.bmp_encode_device_batch([t.data_ptr() for t in srcs], [s] * n, [s] * n, d, files.data_ptr(), stride,
                                             sizes.data_ptr(), status.data_ptr())  # (synchronises)
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == icx.BMP_OK
        assert (status.cpu().numpy() == icx.BMP_OK).all()
        assert bytes(files[:int(sizes[0])].cpu().numpy()) == B.encode(srcs[0].cpu().numpy().reshape(s, s, d))
        res["write"][f"d{d}"] = rate(n * s * s / 1e6, ms)
        print(f"write_d{d}", json.dumps(res["write"][f"d{d}"]), flush=True)
        if d == 3:
            tstride = (icx.tga_encode_bound(s, s, 3) + 255) & ~255
            tfiles = torch.zeros(n * tstride, dtype=torch.uint8, device=dev)
            rc = ctx.tga_encode_device_batch([t.data_ptr() for t in srcs], [s] * n, [s] * n, 3, False, tfiles.data_ptr(),
                                             tstride, sizes.data_ptr(), status.data_ptr())
            assert rc == icx.TGA_OK and (status.cpu().numpy() == icx.TGA_OK).all()
            tsizes = sizes.cpu().numpy()
            for rep in (1, 2):
                r = time_batch(torch, dev, icx.TgaBatch, icx.TGA_OK, ctx, tfiles, tstride, tsizes, n, s, s, a.warmup, a.reps)
                res["targa_same_session"][f"raw24_repeat{rep}"] = r
                print(f"tga_raw24_{rep}", json.dumps(r), flush=True)
            del tfiles
        del files, srcs, base
    runs = [np.ascontiguousarray(P.synth_rgba(40 + k, s, s) & 0xE0) for k in range(min(a.distinct, n))]
    base = [torch.from_numpy(px.reshape(s, s * 4)).to(dev) for px in runs]
    srcs = [torch.roll(base[i % len(base)], 7 * (i // len(base)), 0).reshape(-1).contiguous() for i in range(n)]
    tstride = (icx.tga_encode_bound(s, s, 4) + 255) & ~255
    tfiles = torch.zeros(n * tstride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = ctx.tga_encode_device_batch([t.data_ptr() for t in srcs], [s] * n, [s] * n, 4, True, tfiles.data_ptr(), tstride,
                                     sizes.data_ptr(), status.data_ptr())
    assert rc == icx.TGA_OK and (status.cpu().numpy() == icx.TGA_OK).all()
    for rep in (1, 2):
        r = time_batch(torch, dev, icx.TgaBatch, icx.TGA_OK, ctx, tfiles, tstride, sizes.cpu().numpy(), n, s, s, a.warmup, a.reps)
        res["targa_same_session"][f"runs_rle_repeat{rep}"] = r
        print(f"tga_rle_{rep}", json.dumps(r), flush=True)

    t = res["targa_same_session"]
    spread = abs(t["raw24_repeat1"]["ms_median"] - t["raw24_repeat2"]["ms_median"])
    tga = min(t["raw24_repeat1"]["ms_median"], t["raw24_repeat2"]["ms_median"])
    bmp = res["read"]["raw24"]["ms_median"]
    res["bmp24_vs_tga_raw"] = {"bmp_ms_median": bmp, "tga_ms_median_best_of_two": tga, "session_spread_ms": spread,
                               "bmp_slower_by_more_than_the_spread": bool(bmp - tga > spread)}
    res["rle8_beside_tga_rle"] = {"bmp_rle8_flat_mp_per_s": res["read"]["rle8_flat"]["mp_per_s_median"],
                                  "bmp_rle8_photo_runs_mp_per_s": res["read"]["rle8_photo_runs"]["mp_per_s_median"],
                                  "tga_runs_rle_mp_per_s": [t[f"runs_rle_repeat{k}"]["mp_per_s_median"] for k in (1, 2)]}
    print("summary", json.dumps({k: res[k] for k in ("bmp24_vs_tga_raw", "rle8_beside_tga_rle")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
