#!/usr/bin/env python3
"""Timing aid (GPU box): the GIF write, beside the TIFF LZW write and the GIF read of the same session.

  * N sources of S x S in HBM, written through Context.gif_encode_device_batch: 256-colour
    photograph-like indices (tools/gif_time.py's content, d = 1), flat graphics (16 levels, d = 1),
    an RGB source of more than 256 colours through the cube with and without ordered dithering; a
    sweep of segment_pixels over 4096, 16384, 65536 and -1 (one segment) on the first two; and for
    every sweep value one call with a single image, whose latency is what the cut is for: its time
    over S*S pixels at one segment is the chain's cost per index.
    Megapixels per second over warm-up + repeats (median, min, max), in two rounds with the cases
    alternating: the difference of a case's two medians is its run-to-run spread.
  * The yardsticks, same session: the TIFF LZW write (d = 1, the photograph-like content) at 64-row
    strips and as one strip per image, and GifBatch.decode_device on the files each case just wrote.
  * Read-back: every file of every case is decoded by the batch read and compared on the device with
    what the contract says it holds (the source's own colours, or the cube's).
  * Sizes: the payload over the one-segment payload per sweep value and content, and over PIL's GIF
    of the same indices (reported, not asserted).

Every call is queued on torch's current stream between two device events and ends in a synchronise;
the events' interval includes the host's building of the job table, as the host clock does. The read
is timed by the host clock (tools/tiff_write_time.py says why). --out writes JSON."""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import imagecodecs_amd as icx  # noqa: E402
import gifutil as G  # noqa: E402
from gif_time import pictures  # noqa: E402
from tiff_write_time import timed  # noqa: E402

SWEEP = (4096, 16384, 65536, -1)
B4 = [[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]


def sources(torch, dev, kind, n, s, distinct):
    base = []
    for k, a in enumerate(pictures("photo" if kind != "flat" else "flat", min(distinct, n), s)):
        if kind == "flat":
            a = a * 17
        if kind == "rgb":  # more than 256 colours: three differently rolled copies of the picture
            a = np.stack([a, np.roll(a, 31, 0), np.roll(a, 57, 1)], axis=2)
        base.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return [torch.roll(base[i % len(base)], (13 * (i // len(base)), 29 * (i // len(base))), (0, 1)).contiguous() for i in range(n)]


def expected(torch, src, dither):
    """What the file of src holds, as (s, s, 3) on the device: grey as it is, RGB through the cube."""
    if src.dim() == 2:
        return src[:, :, None].expand(-1, -1, 3)
    s = src.shape[0]
    c = src.to(torch.int64)
    if dither:
        t = torch.tensor(B4, device=src.device, dtype=torch.int64).repeat(s // 4 + 1, s // 4 + 1)[:s, :s] * 2 + 1
    else:
        t = torch.full((s, s), 16, device=src.device, dtype=torch.int64)
    out = []
    for ch, L in enumerate((6, 7, 6)):
        k = (32 * c[:, :, ch] * (L - 1) + 255 * t) // 8160
        out.append((255 * k + (L - 1) // 2) // (L - 1))
    return torch.stack(out, 2).to(torch.uint8)


def time_case(torch, dev, ctx, srcs, s, seg, dither, warmup, reps, check=True):
    n, d = len(srcs), 1 if srcs[0].dim() == 2 else 3
    stride = (icx.gif_encode_bound(s, s, seg) + 255) & ~255
    files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
    status = torch.full((n,), -9, dtype=torch.int32, device=dev)
    ptrs = [t.data_ptr() for t in srcs]
    torch.cuda.synchronize(dev)

    def write(stream):
        rc = ctx.gif_encode_device_batch(ptrs, [s] * n, [s] * n, d, seg, dither, icx.GIF_PALETTE_AUTO, files.data_ptr(), stride,
                                         sizes.data_ptr(), status.data_ptr(), stream)
        assert rc == icx.GIF_OK
    res = {"write": timed(torch, dev, n * s * s / 1e6, warmup, reps, write)}
    assert (status.cpu().numpy() == icx.GIF_OK).all()
    hs = sizes.cpu().numpy()
    res["file_bytes_mean"] = float(hs.mean())
    if check:
        gb = icx.GifBatch(ctx, n, s, s)
        pstride = 3 * s * s
        pix = torch.zeros(n * pstride, dtype=torch.uint8, device=dev)
        st = torch.full((n,), -9, dtype=torch.int32, device=dev)
        dims = torch.zeros(3 * n, dtype=torch.int32, device=dev)
        offs = torch.from_numpy(np.arange(n, dtype=np.int64) * stride).to(dev)
        torch.cuda.synchronize(dev)
        res["read_of_the_same_files"] = timed(
            torch, dev, n * s * s / 1e6, warmup, reps,
            lambda stream: gb.decode_device(n, files.data_ptr(), offs.data_ptr(), sizes.data_ptr(), pix.data_ptr(), pstride,
                                            st.data_ptr(), dims.data_ptr(), stream), by_host=True)
        assert (st.cpu().numpy() == icx.GIF_OK).all()
        for i in range(n):
            assert torch.equal(pix[i * pstride:(i + 1) * pstride].view(s, s, 3), expected(torch, srcs[i], dither)), f"image {i} does not read back"
        gb.close()
    first = bytes(files[:int(hs[0])].cpu().numpy())
    return res, first


def payload_bytes(f):
    code, F = G.parse(f)
    assert code == G.OK and F["has_image"]
    return len(G.data_stream(f, F["data_at"])[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        sys.exit("gif_write_time: no GPU (a rate is only measured on one)")
    dev = torch.device("cuda", 0)
    ctx = icx.Context(0)
    n, s = a.images, a.size
    src = {k: sources(torch, dev, k, n, s, a.distinct) for k in ("photo", "flat", "rgb")}
    cases = [("photo256", "photo", 0, 0), ("flat16", "flat", 0, 0), ("cube", "rgb", 0, 0), ("cube_dither", "rgb", 0, 1)]
    cases += [(f"{kind}_seg{seg}", kind, seg, 0) for kind in ("photo", "flat") for seg in SWEEP]
    res = {"images": n, "size": s, "default_segment_pixels": 65536, "cases": {}, "single_image": {}, "yardsticks_same_session": {}, "sizes": {}}
    firsts = {}
    for rnd in (1, 2):
        for name, kind, seg, dither in cases:
            r, f = time_case(torch, dev, ctx, src[kind], s, seg, dither, a.warmup, a.reps, check=rnd == 1)
            res["cases"].setdefault(name, {})[f"round{rnd}"] = r
            firsts[name] = f
            print(name, rnd, json.dumps(r), flush=True)
        for kind in ("photo", "flat"):
            for seg in SWEEP:
                r, _ = time_case(torch, dev, ctx, src[kind][:1], s, seg, 0, a.warmup, a.reps, check=rnd == 1)
                r["ns_per_pixel"] = r["write"]["ms_median"] * 1e6 / (s * s)
                res["single_image"].setdefault(f"{kind}_seg{seg}", {})[f"round{rnd}"] = r
                print("single", kind, seg, rnd, json.dumps(r), flush=True)
        # the TIFF LZW write of the photograph-like content, d = 1
        for yname, rps in (("tiff_lzw_64_rows", 64), ("tiff_lzw_one_strip", 0)):
            stride = (icx.tiff_encode_bound(s, s, 1, 5, 1, rps) + 255) & ~255
            files = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
            sizes = torch.zeros((n,), dtype=torch.int64, device=dev)
            status = torch.full((n,), -9, dtype=torch.int32, device=dev)
            ptrs = [t.data_ptr() for t in src["photo"]]
            torch.cuda.synchronize(dev)

            def tiff_write(stream):
                rc = ctx.tiff_encode_device_batch(ptrs, [s] * n, [s] * n, 1, 5, 1, rps, files.data_ptr(), stride, sizes.data_ptr(),
                                                  status.data_ptr(), stream)
                assert rc == icx.TIFF_OK
            r = timed(torch, dev, n * s * s / 1e6, a.warmup, a.reps, tiff_write)
            if rps == 0:
                r["ns_per_byte_per_wave"] = r["ms_median"] * 1e6 / (s * s)  # (n <= resident waves: every strip's chain runs at once)
            res["yardsticks_same_session"].setdefault(yname, {})[f"round{rnd}"] = r
            del files
            print(yname, rnd, json.dumps(r), flush=True)
    for group in ("cases", "single_image"):
        for name, v in res[group].items():
            m = [v[f"round{k}"]["write"]["ms_median"] for k in (1, 2)]
            v["spread_ms_between_rounds"] = abs(m[0] - m[1])
    pal = np.random.default_rng(5).integers(0, 256, 768, dtype=np.uint8).tobytes()
    for kind in ("photo", "flat"):
        one = payload_bytes(firsts[f"{kind}_seg-1"])
        px = src[kind][0].cpu().numpy()
        im = Image.fromarray(px // (17 if kind == "flat" else 1), "P")
        im.putpalette(pal)
        b = io.BytesIO()
        im.save(b, "GIF")
        pil = payload_bytes(b.getvalue())
        res["sizes"][kind] = {"one_segment_payload_bytes": one, "pil_payload_bytes": pil, "one_segment_over_pil": one / pil,
                              "payload_over_one_segment": {str(seg): payload_bytes(firsts[f"{kind}_seg{seg}"]) / one for seg in SWEEP}}
        print("sizes", kind, json.dumps(res["sizes"][kind]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
