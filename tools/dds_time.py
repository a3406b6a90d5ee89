#!/usr/bin/env python3
"""Timing aid (GPU box): the DDS read and write, beside the BMP and Targa paths of the same session.

  * N files of S x S per form, built on the host (tests/ddsutil.py) and left in HBM, read through
    DdsBatch.decode_device: megapixels per second over warm-up + repeats (median, min, max), the
    per-stage split of the last repeat, and the bytes the bounding stage moves (file in, pixels out)
    as a share of the HBM peak. Forms: DXT1, DXT5, BC4 (ATI1), BC5 (ATI2), 24-bit B,G,R and 32-bit
    B,G,R,A. The blocks and rasters are random bytes: neither path looks at them. --distinct payloads
    are generated and every file is one of them rotated.
  * The write from random pixels in HBM (Context.dds_encode_device_batch): RAW and BC for d = 3 and 4.
  * The yardsticks in the same session: the 24-bit BMP read, the raw Targa read and the BMP write
    (d = 3, 4). Everything is timed in two rounds, the forms alternating; the difference of a form's
    two medians is its run-to-run spread.
  * "bc1_read_vs_bmp24_read" and "bc_write_d3_vs_bmp_write_d3" compare pixel rates and say whether DDS
    is slower by more than the spread.
  * One core of the same machine: PIL, and the serial core (tests/cxx/dds_core_demo.cpp built with
    g++ -O2; a process that handles the file twice, less one that handles it once).

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream (icx_dds_batch_stage_times). Image 0 and the last image of every form are checked
against the restatement. --out writes the figures as JSON."""
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
import ddsutil as D  # noqa: E402
import bmputil as B  # noqa: E402
from bmp_time import HBM_PEAK, rate, raw_files, upload  # noqa: E402

RGB24 = (0xFF0000, 0xFF00, 0xFF, 0)
BGRA32 = (0xFF0000, 0xFF00, 0xFF, 0xFF000000)


def dds_files(form, n, s, distinct):
    """n files of one form: `distinct` random payloads, each file one of them rotated by whole rows."""
    if form in ("dxt1", "dxt5", "bc4", "bc5"):
        first = D.block_file(1, {"dxt1": b"DXT1", "dxt5": b"DXT5", "bc4": b"ATI1", "bc5": b"ATI2"}[form], s, s)
    else:
        first = D.masked_file(1, s, s, 24 if form == "rgb24" else 32, RGB24 if form == "rgb24" else BGRA32)
    rows = (s + 3) // 4 if form in ("dxt1", "dxt5", "bc4", "bc5") else s
    body = (len(first) - 128) // rows
    base = [np.random.default_rng(700 + k).integers(0, 256, (rows, body), dtype=np.uint8) for k in range(min(distinct, n))]
    return [first[:128] + np.roll(base[i % len(base)], 7 * (i // len(base)), 0).tobytes() for i in range(n)]


def time_read(torch, dev, make_batch, ok, ndims, blob, stride, sizes, n, w, h, warmup, reps, decode, check):
    d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int64)).to(dev)
    out_stride = 4 * w * h
    out = torch.zeros(n * out_stride, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros((n, ndims), dtype=torch.int32, device=dev)
    b = make_batch(n, w, h)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        b.decode_device(n, blob.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), out.data_ptr(), out_stride, st.data_ptr(),
                        dims.data_ptr())
        torch.cuda.synchronize(dev)
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    stages = b.stage_times()
    assert (st.cpu().numpy() == ok).all(), st.cpu().numpy()
    moved = float(np.sum(sizes))
    for i in (0, n - 1):  # against the restatement
        want = decode(check[i])
        got = out[i * out_stride:i * out_stride + want.size].cpu().numpy()
        assert (got == want.reshape(-1)).all(), f"image {i} differs from the restatement"
        if i == 0:
            moved += n * float(want.size)
    b.close()
    top = max(stages, key=stages.get)
    res = {"images": n, "width": w, "height": h, "file_bytes_mean": float(np.mean(sizes)), "stage_ms_last_repeat": stages,
           "bounding_stage": top, "bytes_moved": moved, "bounding_stage_share_of_hbm_peak": moved / (stages[top] * 1e-3) / HBM_PEAK}
    res.update(rate(n * w * h / 1e6, ms))
    res["bytes_moved_per_s_median"] = moved / (res["ms_median"] * 1e-3)
    return res


def time_write(torch, dev, encode, bound, srcs, n, s, d, warmup, reps, want_first):
    stride = (bound + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        rc = encode([t.data_ptr() for t in srcs], [s] * n, [s] * n, files.data_ptr(), stride, sizes.data_ptr(), status.data_ptr())
        if k >= warmup:  # (the call synchronises)
            ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0
    assert (status.cpu().numpy() == 0).all()
    assert bytes(files[:int(sizes[0])].cpu().numpy()) == want_first, "image 0 differs from the restatement"
    res = rate(n * s * s / 1e6, ms)
    res["bytes_moved"] = float(n) * (s * s * d + bound)
    res["bytes_moved_per_s_median"] = res["bytes_moved"] / (res["ms_median"] * 1e-3)
    res["share_of_hbm_peak"] = res["bytes_moved_per_s_median"] / HBM_PEAK
    return res


def time_pil_read(data, w, h, reps=3):
    from PIL import Image
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        Image.open(io.BytesIO(data)).load()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": w * h / 1e6 / statistics.median(ms) * 1e3}


def time_pil_write(px, pixel_format, reps=3):
    from PIL import Image
    im = Image.fromarray(px)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        try:
            im.save(io.BytesIO(), "DDS", **({"pixel_format": pixel_format} if pixel_format else {}))
        except (KeyError, OSError, ValueError, TypeError):
            return None  # (a PIL that does not write this form)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": px.shape[0] * px.shape[1] / 1e6 / statistics.median(ms) * 1e3}


def time_serial_core(reads, writes, s):
    """{form: one dds_decode_serial / dds_encode_serial}: a process that does it twice, less one that does it once."""
    out = {"read": {}, "write": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "dds_core_demo")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cxx", "dds_core_demo.cpp"), "-o", exe], check=True)

        def twice_less_once(args_for):
            t = []
            for k in (1, 2):
                args = args_for(k)
                best = 1e9
                for _ in range(3):
                    t0 = time.perf_counter()
                    subprocess.run([exe, *args], check=True, stdout=subprocess.DEVNULL)
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                t.append(best)
            ms = max(t[1] - t[0], 1e-3)
            return {"ms": ms, "mp_per_s": s * s / 1e6 / ms * 1e3}

        lst = os.path.join(tmp, "list.txt")
        for form, data in reads.items():
            path = os.path.join(tmp, "f.dds")
            open(path, "wb").write(data)

            def args_for(k):
                open(lst, "w").write((path + "\n") * k)
                return ["decode", lst, os.path.join(tmp, "out.bin")]
            out["read"][form] = twice_less_once(args_for)
        for form, (px, fmt) in writes.items():
            path = os.path.join(tmp, "px.bin")
            open(path, "wb").write(px.tobytes())

            def args_for(k):
                open(lst, "w").write(f"{path} {s} {s} {px.shape[2]} {fmt} {os.path.join(tmp, 'w.dds')}\n" * k)
                return ["write", lst]
            out["write"][form] = twice_less_once(args_for)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8, help="generated payloads; each image is one of them rotated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dds_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    res = {"read": {}, "write": {}, "yardsticks_same_session": {}, "cpu_one_core": {"pil": {"read": {}, "write": {}}}}

    # the files of every read form, resident for both rounds
    reads = {}
    for form in ("dxt1", "dxt5", "bc4", "bc5", "rgb24", "bgra32"):
        files = dds_files(form, n, s, a.distinct)
        reads[form] = ("dds", files[0], files[-1], *upload(torch, dev, files))
    bmp = raw_files(24, n, s, a.distinct)
    reads["bmp24"] = ("bmp", bmp[0], bmp[-1], *upload(torch, dev, bmp))
    px3 = [torch.randint(0, 256, (s, s * 3), dtype=torch.uint8, device=dev) for _ in range(min(a.distinct, n))]
    srcs3 = [torch.roll(px3[i % len(px3)], 7 * (i // len(px3)), 0).reshape(-1).contiguous() for i in range(n)]
    px4 = [torch.randint(0, 256, (s, s * 4), dtype=torch.uint8, device=dev) for _ in range(min(a.distinct, n))]
    srcs4 = [torch.roll(px4[i % len(px4)], 7 * (i // len(px4)), 0).reshape(-1).contiguous() for i in range(n)]
    tstride = (icx.tga_encode_bound(s, s, 3) + 255) & ~255
    tfiles = torch.zeros(n * tstride, dtype=torch.uint8, device=dev)
    tsz = torch.zeros((n,), dtype=torch.int64, device=dev)
    tst = torch.full((n,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rc = ctx.tga_encode_device_batch([t.data_ptr() for t in srcs3], [s] * n, [s] * n, 3, False, tfiles.data_ptr(), tstride,
                                     tsz.data_ptr(), tst.data_ptr())
    assert rc == icx.TGA_OK and (tst.cpu().numpy() == icx.TGA_OK).all()
    tsizes = tsz.cpu().numpy()
    first3, last3 = (srcs3[i].cpu().numpy().reshape(s, s, 3) for i in (0, n - 1))
    first4 = srcs4[0].cpu().numpy().reshape(s, s, 4)

    for rnd in (1, 2):
        for form, (kind, f0, f1, blob, stride, sizes) in reads.items():
            if kind == "dds":
                r = time_read(torch, dev, lambda *x: icx.DdsBatch(ctx, *x), icx.DDS_OK, 4, blob, stride, sizes, n, s, s, a.warmup,
                              a.reps, lambda f: D.decode(f)[5], {0: f0, n - 1: f1})
                res["read"].setdefault(form, {})[f"round{rnd}"] = r
            else:
                r = time_read(torch, dev, lambda *x: icx.BmpBatch(ctx, *x), icx.BMP_OK, 3, blob, stride, sizes, n, s, s, a.warmup,
                              a.reps, lambda f: B.decode(f)[4], {0: f0, n - 1: f1})
                res["yardsticks_same_session"].setdefault("bmp24_read", {})[f"round{rnd}"] = r
            print(form, rnd, json.dumps(r), flush=True)
        r = time_read(torch, dev, lambda *x: icx.TgaBatch(ctx, *x), icx.TGA_OK, 3, tfiles, tstride, tsizes, n, s, s, a.warmup, a.reps,
                      lambda px: px, {0: first3, n - 1: last3})
        res["yardsticks_same_session"].setdefault("tga_raw24_read", {})[f"round{rnd}"] = r
        print("tga_raw24", rnd, json.dumps(r), flush=True)
        for d, srcs, first in ((3, srcs3, first3), (4, srcs4, first4)):
            for name, fmt in (("raw", icx.DDS_RAW), ("bc", icx.DDS_BC)):
                r = time_write(torch, dev, lambda p, w, h, *rest: ctx.dds_encode_device_batch(p, w, h, d, fmt, *rest),
                               icx.dds_encode_bound(s, s, d, fmt), srcs, n, s, d, a.warmup, a.reps, D.encode(first, fmt))
                res["write"].setdefault(f"{name}_d{d}", {})[f"round{rnd}"] = r
                print(f"write_{name}_d{d}", rnd, json.dumps(r), flush=True)
            r = time_write(torch, dev, lambda p, w, h, *rest: ctx.bmp_encode_device_batch(p, w, h, d, *rest),
                           icx.bmp_encode_bound(s, s, d), srcs, n, s, d, a.warmup, a.reps, B.encode(first))
            res["yardsticks_same_session"].setdefault(f"bmp_write_d{d}", {})[f"round{rnd}"] = r
            print(f"bmp_write_d{d}", rnd, json.dumps(r), flush=True)

    def two(entry):  # the better median of the two rounds, and their difference
        m = [entry[f"round{k}"]["ms_median"] for k in (1, 2)]
        return min(m), abs(m[0] - m[1])

    def versus(ours, yard):
        (o, so), (y, sy) = two(ours), two(yard)
        return {"dds_ms_median_best_of_two": o, "yardstick_ms_median_best_of_two": y, "spread_ms": max(so, sy),
                "dds_slower_by_more_than_the_spread": bool(o - y > max(so, sy))}

    y = res["yardsticks_same_session"]
    res["bc1_read_vs_bmp24_read"] = versus(res["read"]["dxt1"], y["bmp24_read"])
    res["rgb24_read_vs_bmp24_read"] = versus(res["read"]["rgb24"], y["bmp24_read"])
    res["bc_write_d3_vs_bmp_write_d3"] = versus(res["write"]["bc_d3"], y["bmp_write_d3"])
    res["raw_write_d3_vs_bmp_write_d3"] = versus(res["write"]["raw_d3"], y["bmp_write_d3"])
    print("summary", json.dumps({k: v for k, v in res.items() if "_vs_" in k}), flush=True)

    # one core of this machine
    for form, (kind, f0, *_rest) in reads.items():
        if kind == "dds":
            res["cpu_one_core"]["pil"]["read"][form] = time_pil_read(f0, s, s)
    for name, px, pf in (("raw_d3", first3, None), ("bc_d3", first3, "DXT1"), ("raw_d4", first4, None), ("bc_d4", first4, "DXT5")):
        r = time_pil_write(px, pf)
        if r:
            res["cpu_one_core"]["pil"]["write"][name] = r
    res["cpu_one_core"]["serial_core"] = time_serial_core(
        {form: v[1] for form, v in reads.items() if v[0] == "dds"},
        {"raw_d3": (first3, D.RAW), "bc_d3": (first3, D.BC), "raw_d4": (first4, D.RAW), "bc_d4": (first4, D.BC)}, s)
    print("cpu_one_core", json.dumps(res["cpu_one_core"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
