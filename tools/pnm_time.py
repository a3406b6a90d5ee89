#!/usr/bin/env python3
"""Timing aid (GPU box): the Netpbm read and write.

  * N images of S x S (--distinct random pictures; every image of the batch is one of them with its
    rows rotated by a different amount, so each has its own N-th of the input in HBM and no two files
    are equal) are written on the box by Context.pnm_encode_device_batch as P6, P5, P4 and PF, left in
    HBM and read back through PnmBatch.decode_device. P3 text (one row per line, "%d" samples) is
    made on the host for the distinct pictures and rotated line-wise on the device. Each result has
    megapixels per second over warm-up + repeats (median, min, max), the per-stage split of the last
    repeat (icx_pnm_batch_stage_times) and, for the stage that does the work, the bytes the algorithm
    must move (file in, pixels out) over the stage time as a share of the 8 TB/s HBM peak. The P3 read
    is also given in GB/s of text.
  * The comparison line: the P6 read and write stream the same bytes as the raw Targa paths, so
    TgaBatch's raw read and the raw Targa write of the same pictures are timed in the same session,
    the two alternating call by call; "spread" is (max - min) / median of the repeats of one call.
  * CPU, one core of the same machine: PIL for each form it reads, and the serial core
    (tests/cxx/pnm_core_demo.cpp built with g++ -O2; the time of a second decode in one process).

Times are a host clock around the call and a device synchronise; the stages are HIP events on the
launch stream. --out writes the figures as JSON."""
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
import imagecodecs_amd as icx  # noqa: E402

HBM_PEAK = 8e12  # bytes per second (MI355X specification)
FORMS = {"P6": (icx.PNM_P6, 3, icx.PNM_UBYTE), "P5": (icx.PNM_P5, 1, icx.PNM_UBYTE), "P4": (icx.PNM_P4, 1, icx.PNM_UBYTE),
         "PF": (icx.PNM_PF, 3, icx.PNM_FLOAT)}


def rate(mp, ms):
    med = statistics.median(ms)
    return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
            "mp_per_s_median": mp / med * 1e3, "mp_per_s_min": mp / max(ms) * 1e3, "mp_per_s_max": mp / min(ms) * 1e3}


def timed(torch, dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


class PnmWrite:
    def __init__(self, torch, dev, ctx, srcs, s, form):
        self.fmt, self.d, self.typ = FORMS[form]
        self.n, self.s, self.ctx = len(srcs), s, ctx
        self.stride = (icx.pnm_encode_bound(s, s, self.d, self.typ, self.fmt) + 255) & ~255
        self.files = torch.zeros(self.n * self.stride, dtype=torch.uint8, device=dev)
        self.sizes = torch.zeros((self.n,), dtype=torch.int64, device=dev)
        self.status = torch.full((self.n,), -9, dtype=torch.int32, device=dev)
        self.ptrs = [x.data_ptr() for x in srcs]

    def __call__(self):
        rc = self.ctx.pnm_encode_device_batch(self.ptrs, [self.s] * self.n, [self.s] * self.n, self.d, self.typ, self.fmt,
                                              self.files.data_ptr(), self.stride, self.sizes.data_ptr(), self.status.data_ptr())
        assert rc == icx.PNM_OK


class PnmRead:
    def __init__(self, torch, dev, ctx, files, offsets, sizes, n, s, out_bytes):
        self.files = files
        self.d_off = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev)
        self.d_sz = torch.from_numpy(np.asarray(sizes, np.int64)).to(dev)
        self.n, self.out_stride = n, (out_bytes + 15) & ~15
        self.out = torch.zeros(n * self.out_stride, dtype=torch.uint8, device=dev)
        self.st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        self.dims = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        self.b = icx.PnmBatch(ctx, n, s, s)

    def __call__(self):
        rc = self.b.decode_device(self.n, self.files.data_ptr(), self.d_off.data_ptr(), self.d_sz.data_ptr(), self.out.data_ptr(),
                                  self.out_stride, self.st.data_ptr(), self.dims.data_ptr())
        assert rc == icx.PNM_OK


class TgaWrite:
    def __init__(self, torch, dev, ctx, srcs, s):
        self.n, self.s, self.ctx = len(srcs), s, ctx
        self.stride = (icx.tga_encode_bound(s, s, 3) + 255) & ~255
        self.files = torch.zeros(self.n * self.stride, dtype=torch.uint8, device=dev)
        self.sizes = torch.zeros((self.n,), dtype=torch.int64, device=dev)
        self.status = torch.full((self.n,), -9, dtype=torch.int32, device=dev)
        self.ptrs = [x.data_ptr() for x in srcs]

    def __call__(self):
        rc = self.ctx.tga_encode_device_batch(self.ptrs, [self.s] * self.n, [self.s] * self.n, 3, False, self.files.data_ptr(),
                                              self.stride, self.sizes.data_ptr(), self.status.data_ptr())
        assert rc == icx.TGA_OK


class TgaRead:
    def __init__(self, torch, dev, ctx, w, n, s):
        self.w, self.n = w, n
        self.d_off = torch.from_numpy(np.arange(n, dtype=np.int64) * w.stride).to(dev)
        self.out_stride = 4 * s * s
        self.out = torch.zeros(n * self.out_stride, dtype=torch.uint8, device=dev)
        self.st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        self.dims = torch.zeros((n, 3), dtype=torch.int32, device=dev)
        self.b = icx.TgaBatch(ctx, n, s, s)

    def __call__(self):
        self.b.decode_device(self.n, self.w.files.data_ptr(), self.d_off.data_ptr(), self.w.sizes.data_ptr(), self.out.data_ptr(),
                             self.out_stride, self.st.data_ptr(), self.dims.data_ptr())


def alternate(torch, dev, calls, warmup, reps):
    """{name: [ms]}: the calls take turns, so drift of the machine falls on all of them alike."""
    ms = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            t = timed(torch, dev, fn)
            if r >= warmup:
                ms[k].append(t)
    return ms


def p3_text(px):
    """uint8 (s, s, 3) -> (header, raster text, the offset of every line in the raster)."""
    lines = [(" ".join(map(str, row.reshape(-1).tolist())) + "\n").encode() for row in px]
    offs = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])])
    return b"P3\n%d %d\n255\n" % (px.shape[1], px.shape[0]), b"".join(lines), offs


def time_pil(data, reps=3):
    try:
        from PIL import Image
    except ImportError:
        return None
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        im = Image.open(io.BytesIO(data))
        im.load()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "mp_per_s_median": im.size[0] * im.size[1] / 1e6 / statistics.median(ms) * 1e3}


def time_serial_core(datas):
    """{form: ms of one pnm_decode_serial}: a process that decodes the file twice, less one that decodes it once."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pnm_core_demo")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "imagecodecs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cxx", "pnm_core_demo.cpp"), "-o", exe], check=True)
        res = {}
        for form, data in datas.items():
            src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
            open(src, "wb").write(data)
            t = []
            for k in (1, 2):
                open(os.path.join(tmp, "jobs"), "w").write(f"decode {src} {dst}\n" * k)
                runs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    subprocess.run([exe, os.path.join(tmp, "jobs")], check=True, capture_output=True)
                    runs.append((time.perf_counter() - t0) * 1e3)
                t.append(statistics.median(runs))
            res[form] = {"ms": max(t[1] - t[0], 1e-3)}
        return res


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
        sys.exit("pnm_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s, nd = a.images, a.size, min(a.distinct, a.images)
    mp = n * s * s / 1e6
    res = {"images": n, "size": s, "hbm_peak_bytes_per_s": HBM_PEAK}
    g = torch.Generator(device=dev).manual_seed(7)
    shift = [7 * (i // nd) % s for i in range(n)]
    host_files = {}

    def sources(d, dtype):
        if dtype == torch.float32:
            base = [torch.randn((s, s * d), generator=g, device=dev) for _ in range(nd)]
        else:
            base = [torch.randint(0, 256, (s, s * d), generator=g, device=dev, dtype=torch.uint8) for _ in range(nd)]
        return base, [torch.roll(base[i % nd], shift[i], 0).reshape(-1).contiguous() for i in range(n)]

    for form, (fmt, d, typ) in FORMS.items():
        base, srcs = sources(d, torch.float32 if typ == icx.PNM_FLOAT else torch.uint8)
        if form == "P4":
            srcs = [torch.where(x > 127, 255, 0).to(torch.uint8) for x in srcs]
        w = PnmWrite(torch, dev, ctx, srcs, s, form)
        calls = {"write": w}
        if form == "P6":
            tw = TgaWrite(torch, dev, ctx, srcs, s)
            calls["tga_raw_write"] = tw
        ms = alternate(torch, dev, calls, a.warmup, a.reps)
        assert (w.status.cpu().numpy() == icx.PNM_OK).all()
        sizes = w.sizes.cpu().numpy()
        es = 4 if typ == icx.PNM_FLOAT else 1
        out_bytes = s * s * d * es
        r = PnmRead(torch, dev, ctx, w.files, np.arange(n, dtype=np.int64) * w.stride, sizes, n, s, out_bytes)
        calls = {"read": r}
        if form == "P6":
            tr = TgaRead(torch, dev, ctx, tw, n, s)
            calls["tga_raw_read"] = tr
        ms.update(alternate(torch, dev, calls, a.warmup, a.reps))
        stages = r.b.stage_times()
        assert (r.st.cpu().numpy() == icx.PNM_OK).all(), r.st.cpu().numpy()
        for i in range(n):  # the read gives back the writer's input, every image of the batch
            assert torch.equal(r.out[i * r.out_stride:i * r.out_stride + out_bytes], srcs[i].view(torch.uint8).reshape(-1)), (form, i)
        moved = float(np.sum(sizes)) + n * float(s * s * d * es)  # both directions move the file and the pixels once
        entry = {"file_bytes_mean": float(np.mean(sizes)), "bytes_per_pixel_moved": moved / (n * s * s),
                 "read": rate(mp, ms["read"]), "write": rate(mp, ms["write"]), "read_stage_ms_last_repeat": stages}
        entry["read"]["stream_stage_share_of_hbm_peak"] = moved / (stages["stream"] * 1e-3) / HBM_PEAK
        entry["read"]["call_share_of_hbm_peak"] = moved / (entry["read"]["ms_median"] * 1e-3) / HBM_PEAK
        entry["write"]["call_share_of_hbm_peak"] = moved / (entry["write"]["ms_median"] * 1e-3) / HBM_PEAK
        if form == "P6":
            assert (tr.st.cpu().numpy() == icx.TGA_OK).all()
            entry["tga_raw_read"] = rate(mp, ms["tga_raw_read"])
            entry["tga_raw_read"]["stage_ms_last_repeat"] = tr.b.stage_times()
            entry["tga_raw_write"] = rate(mp, ms["tga_raw_write"])
            entry["read_over_tga_raw_read"] = entry["read"]["ms_median"] / entry["tga_raw_read"]["ms_median"]
            entry["write_over_tga_raw_write"] = entry["write"]["ms_median"] / entry["tga_raw_write"]["ms_median"]
            tr.b.close()
            del tr, tw
        host_files[form] = bytes(w.files[: int(sizes[0])].cpu().numpy())
        res[form] = entry
        print(form, json.dumps(entry), flush=True)
        r.b.close()
        if form == "P6":
            p3_base = [b.reshape(s, s, 3).cpu().numpy() for b in base]
        del r, w, srcs, base

    # P3: text of the distinct pictures from the host, rotated line-wise on the device
    texts = [p3_text(px) for px in p3_base]
    stride = (max(len(h) + len(t) for h, t, _ in texts) + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    d_text = [torch.from_numpy(np.frombuffer(t, np.uint8).copy()).to(dev) for _, t, _ in texts]
    sizes, expect = [], []
    for i in range(n):
        h, t, offs = texts[i % nd]
        k = (s - shift[i]) % s  # roll(rows, shift): the file starts with row s - shift
        files[i * stride:i * stride + len(h)] = torch.from_numpy(np.frombuffer(h, np.uint8).copy()).to(dev)
        files[i * stride + len(h):i * stride + len(h) + len(t)] = torch.roll(d_text[i % nd], -int(offs[k]))
        sizes.append(len(h) + len(t))
        expect.append(torch.roll(torch.from_numpy(p3_base[i % nd]).to(dev).reshape(s, s * 3), shift[i], 0).reshape(-1))
    r = PnmRead(torch, dev, ctx, files, np.arange(n, dtype=np.int64) * stride, sizes, n, s, s * s * 3)
    ms = alternate(torch, dev, {"read": r}, a.warmup, a.reps)
    stages = r.b.stage_times()
    assert (r.st.cpu().numpy() == icx.PNM_OK).all(), r.st.cpu().numpy()
    for i in range(n):
        assert torch.equal(r.out[i * r.out_stride:i * r.out_stride + s * s * 3], expect[i]), ("P3", i)
    text_bytes = float(np.sum(sizes))
    entry = {"file_bytes_mean": text_bytes / n, "text_bytes_per_pixel": text_bytes / (n * s * s),
             "read": rate(mp, ms["read"]), "read_stage_ms_last_repeat": stages}
    entry["read"]["text_gb_per_s_median"] = text_bytes / (entry["read"]["ms_median"] * 1e-3) / 1e9
    entry["read"]["gp_per_s_median"] = entry["read"]["mp_per_s_median"] / 1e3
    # the text is read twice (locate, text) and the samples written once
    entry["read"]["call_share_of_hbm_peak"] = (2 * text_bytes + n * s * s * 3.0) / (entry["read"]["ms_median"] * 1e-3) / HBM_PEAK
    host_files["P3"] = bytes(files[: sizes[0]].cpu().numpy())
    res["P3"] = entry
    print("P3", json.dumps(entry), flush=True)
    r.b.close()

    res["cpu_one_core"] = {"pil": {f: time_pil(d) for f, d in host_files.items() if f != "PF"},
                           "serial_core": time_serial_core(host_files)}
    for f, v in res["cpu_one_core"]["serial_core"].items():
        v["mp_per_s"] = s * s / 1e6 / v["ms"] * 1e3
    print("cpu", json.dumps(res["cpu_one_core"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
