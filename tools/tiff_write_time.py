#!/usr/bin/env python3
"""Timing aid (GPU box): the TIFF write, beside the TIFF read of the files just written and the BMP
write of the same session.

  * N sources of S x S RGB in HBM, written through Context.tiff_encode_device_batch in strips of
    --rows rows: compression 1; PackBits on flat graphics and on noise; LZW and Deflate with and
    without the predictor on a smooth picture; LZW and Deflate as one strip (the reference's layout).
    Megapixels per second over warm-up + repeats (median, min, max), in two rounds with the cases
    alternating: the difference of a case's two medians is its run-to-run spread.
  * The yardsticks, same session: TiffBatch.decode_device on the files each case just wrote (read
    back to the sources, which also checks every file), and the BMP write (d = 3).
  * Sizes: payload bytes over raw bytes per case, and the Deflate payload over zlib level 6, on
    tiffutil.smooth, on the reference's test.tif tiled to S x S and on noise.

Every call is queued on torch's current stream between two device events and ends in a synchronise:
"ms_*" / "mp_per_s_*" are the events' times, "host_ms_median" a host clock around the same call and
its synchronise. The first event is reached before the call has built its strip and segment tables
on the host, so the events' interval includes that host time as an idle stream, as the host clock
does: neither figure is kernel time alone. The read of the files is timed by the host clock: events
on the caller's stream did not bracket the batch read's work (they showed 0.03 ms for 256 images). --out writes JSON."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import imagecodecs_amd as icx  # noqa: E402
import tiffutil as T  # noqa: E402
import tiffwutil as W  # noqa: E402
from bmp_time import rate  # noqa: E402


def sources(torch, dev, kind, n, s, distinct, fixture):
    base = []
    for k in range(min(distinct, n)):
        if kind == "noise":
            a = T.noise(900 + k, s, s, 3)
        elif kind == "smooth":
            a = T.smooth(k, s, s, 3)
        elif kind == "flat":  # graphics: flat rectangles of a few colours
            rng = np.random.default_rng(k)
            a = np.repeat(np.repeat(rng.integers(0, 4, (s // 32, s // 64, 1)) * 80, 32, 0), 64, 1).astype(np.uint8) * np.ones((1, 1, 3), np.uint8)
        else:
            reps = (-(-s // fixture.shape[0]), -(-s // fixture.shape[1]), 1)
            a = np.roll(np.tile(fixture, reps)[:s, :s], 13 * k, 1)
        base.append(torch.from_numpy(np.ascontiguousarray(a).reshape(s, s * 3)).to(dev))
    return [torch.roll(base[i % len(base)], 7 * (i // len(base)), 0).reshape(-1).contiguous() for i in range(n)]


def timed(torch, dev, mp, warmup, reps, call, by_host=False):
    """call(stream) queued between two events, synchronised; -> rate() of the events' ms + the host's
    median. by_host: rate() of the host clock's ms (the batch read, whose work events on the caller's
    stream did not bracket) + the events' median."""
    import statistics
    stream = torch.cuda.current_stream(dev)
    ev, host = [], []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        call(stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        if k >= warmup:
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    r = rate(mp, host if by_host else ev)
    r["event_ms_median" if by_host else "host_ms_median"] = statistics.median(ev if by_host else host)
    return r


def time_case(torch, dev, ctx, srcs, n, s, comp, pred, rps, warmup, reps):
    bound = icx.tiff_encode_bound(s, s, 3, comp, pred, rps)
    stride = (bound + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    ptrs = [t.data_ptr() for t in srcs]
    torch.cuda.synchronize(dev)

    def write(stream):
        rc = ctx.tiff_encode_device_batch(ptrs, [s] * n, [s] * n, 3, comp, pred, rps, files.data_ptr(), stride, sizes.data_ptr(),
                                          status.data_ptr(), stream)
        assert rc == icx.TIFF_OK
    res = {"write": timed(torch, dev, n * s * s / 1e6, warmup, reps, write)}
    assert (status.cpu().numpy() == icx.TIFF_OK).all()
    hs = sizes.cpu().numpy()
    res["file_bytes_over_raw"] = float(hs.mean()) / (s * s * 3)
    # the read of the same files, back to the sources
    tb = icx.TiffBatch(ctx, n, s, s)
    pstride = 4 * s * s
    pix = torch.zeros(n * pstride, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -9, dtype=torch.int32, device=dev)
    dims = torch.zeros(3 * n, dtype=torch.int32, device=dev)
    offs = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
    torch.cuda.synchronize(dev)
    read = timed(torch, dev, n * s * s / 1e6, warmup, reps,
                 lambda stream: tb.decode_device(n, files.data_ptr(), offs.data_ptr(), sizes.data_ptr(), pix.data_ptr(), pstride,
                                                 st.data_ptr(), dims.data_ptr(), stream), by_host=True)
    assert (st.cpu().numpy() == icx.TIFF_OK).all()
    for i in (0, n - 1):
        assert torch.equal(pix[i * pstride:i * pstride + 3 * s * s], srcs[i]), f"image {i} does not read back"
    tb.close()
    res["read_of_the_same_files"] = read
    first = bytes(files[:int(hs[0])].cpu().numpy())
    return res, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tiff_write_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    fixture = ctx.tiff_decode(open(os.path.join(ROOT, "tests", "golden", "tiff", "test.tif"), "rb").read())[4]
    src = {k: sources(torch, dev, k, n, s, a.distinct, fixture) for k in ("noise", "smooth", "flat", "fixture")}
    cases = [("none", "noise", 1, 1, a.rows), ("packbits_flat", "flat", 32773, 1, a.rows), ("packbits_noise", "noise", 32773, 1, a.rows),
             ("lzw", "smooth", 5, 1, a.rows), ("lzw_pred2", "smooth", 5, 2, a.rows),
             ("deflate", "smooth", 8, 1, a.rows), ("deflate_pred2", "smooth", 8, 2, a.rows),
             ("lzw_one_strip", "smooth", 5, 1, 0), ("deflate_one_strip", "smooth", 8, 1, 0)]
    res = {"images": n, "size": s, "rows_per_strip": a.rows, "cases": {}, "yardsticks_same_session": {}, "sizes": {}}
    for rnd in (1, 2):
        for name, kind, comp, pred, rps in cases:
            r, _ = time_case(torch, dev, ctx, src[kind], n, s, comp, pred, rps, a.warmup, a.reps)
            res["cases"].setdefault(name, {})[f"round{rnd}"] = r
            print(name, rnd, json.dumps(r), flush=True)
        bound = icx.bmp_encode_bound(s, s, 3)
        stride = (bound + 255) & ~255
        files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
        status = torch.full((n,), -9, dtype=torch.int32, device=dev)
        ptrs = [t.data_ptr() for t in src["noise"]]
        torch.cuda.synchronize(dev)

        def bmp_write(stream):
            rc = ctx.bmp_encode_device_batch(ptrs, [s] * n, [s] * n, 3, files.data_ptr(), stride, sizes.data_ptr(), status.data_ptr(), stream)
            assert rc == icx.BMP_OK
        res["yardsticks_same_session"].setdefault("bmp_write_d3", {})[f"round{rnd}"] = timed(torch, dev, n * s * s / 1e6, a.warmup, a.reps, bmp_write)
        del files
        print("bmp_write_d3", rnd, json.dumps(res["yardsticks_same_session"]["bmp_write_d3"][f"round{rnd}"]), flush=True)
    for name in res["cases"]:
        m = [res["cases"][name][f"round{k}"]["write"]["ms_median"] for k in (1, 2)]
        res["cases"][name]["spread_ms_between_rounds"] = abs(m[0] - m[1])
    # sizes: one image of each content, 64-row strips
    for kind in ("smooth", "fixture", "noise"):
        one = src[kind][:1]
        px = one[0].cpu().numpy().reshape(s, s, 3)
        out = {}
        for cname, comp, pred in (("packbits", 32773, 1), ("lzw", 5, 1), ("lzw_pred2", 5, 2), ("deflate", 8, 1), ("deflate_pred2", 8, 2)):
            _, f = time_case(torch, dev, ctx, one, 1, s, comp, pred, a.rows, 0, 1)
            pays = W.file_strips(f)[1]
            ours = sum(len(p) for p in pays)
            out[cname] = {"payload_over_raw": ours / px.size}
            if comp == 8:
                z6 = sum(len(zlib.compress(r, 6)) for r in W.strips_raw(px, pred, a.rows))
                out[cname]["payload_over_zlib6"] = ours / z6
        res["sizes"][kind] = out
        print("sizes", kind, json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
