// icx_gif.hip -- GIF read on gfx950: Image::readGif (codecs.cpp:507-542) over gd_open_gif /
// gd_get_frame / gd_render_frame (gif.cpp:43-524), with the contract and deviations of include/icx.h.
//
//   k_gif_parse   container walk (gif_parse), one lane per image -> descriptor record
//   k_gif_lzw     one wave per image, alone in its workgroup. The wave stages the file through an
//                 LDS window (16-byte loads bounded by the file's length), walks the sub-block chain
//                 there and packs the payload into an LDS ring of code bytes. 64 lanes then take 64
//                 codes at once: between two clear codes the k-th code's bit offset and width are a
//                 closed form (gif_code_offset / gif_code_width), and a ballot finds the first clear /
//                 stop / invalid / missing code. String lengths and first bytes of the codes before
//                 it come from the table, or -- for entries made by the same 64 codes -- by pointer
//                 doubling over the lanes; a wave scan gives every string its place in the index
//                 stream. The table is the classic prefix / suffix / length one (16 KiB + 4 KiB of
//                 first bytes): once the 64 codes' entries are in, the lanes walk their own chains
//                 back to front and store the indices into the image's index plane, which is laid out
//                 as the clipped frame rectangle (interlace map and clipping applied here, per row).
//                 The round from the 64 codes to the stored bytes is icx_lzw_wave.h.
//   k_gif_render  canvas rows: background, frame rectangle through the palette with the transparent
//                 skip; pixels the stream did not reach read as the background index. A row segment
//                 is assembled in LDS and leaves as 16-byte stores at the destination's alignment.
//   k_gif_finish  status and dims
// No stream is declined: there is no serial fallback kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_gif_core.h"
#include "icx_lzw_wave.h"

namespace icx {

constexpr int kGifWin = 2048;    // file bytes staged per window load (tests/test_gpu_gif.py names both)
constexpr int kGifRing = 2048;   // code bytes the ring holds (a power of two)
constexpr int kGifSeg = 1024;    // pixels per row segment of k_gif_render
enum { kGifEndNone = 0, kGifEndTerm = 1, kGifEndFile = 2 };

struct GifDesc {
    GifHead H;
    int64_t size;
    int32_t status;
    uint32_t produced;  // stream pixels the data reached (k_gif_lzw)
};

__global__ void k_gif_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ size, GifDesc* __restrict__ desc, int max_w, int max_h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GifDesc dd{};
    dd.size = (int64_t)size[i];
    dd.status = gif_parse(data + off[i], dd.size, &dd.H);
    if (dd.status == kGifOk && (dd.H.w > max_w || dd.H.h > max_h)) dd.status = kGifTooLarge;
    desc[i] = dd;
}

// One wave per image.
__global__ __launch_bounds__(64) void k_gif_lzw(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                GifDesc* __restrict__ desc, uint8_t* __restrict__ plane,
                                                uint64_t plane_stride) {
    __shared__ uint32_t tab[4096];  // the LZW table (icx_lzw_wave.h)
    __shared__ uint8_t first[4096];
    __shared__ __attribute__((aligned(16))) uint8_t win[kGifWin];
    __shared__ uint8_t ring[kGifRing];
    const int i = blockIdx.x, lane = threadIdx.x;
    GifDesc& dd = desc[i];
    if (dd.status != kGifOk || !dd.H.has_image) return;
    const GifHead H = dd.H;
    const uint8_t* d = data + off[i];
    const int64_t n = dd.size;
    uint8_t* pl = plane + (uint64_t)i * plane_stride;
    const int mcs = H.mcs, clear = 1 << mcs;
    const uint32_t fw = (uint32_t)H.fw, npix = fw * (uint32_t)H.fh;  // (< 2^32)
    const uint32_t cw = (uint32_t)min(H.fw, H.w - H.fx), ch = (uint32_t)min(H.fh, H.h - H.fy);

    // input: the sub-block chain -> ring
    int64_t p = H.data_at;              // the next sub-block's size byte
    int64_t wbase = INT64_MIN / 2;      // file offset of win[0]
    int ended = kGifEndNone;
    uint32_t wr = 0, rdbyte = 0, rdbit = 0;  // ring bytes written; read position (counters wrap; the ring's size divides 2^32)
    // decode state
    uint32_t t0 = 0;                    // the next code's number after the last clear
    LzwCarry C;                         // C.base: index bytes produced
    int status = kGifOk;

    while (C.base < npix) {
        while (ended == kGifEndNone && kGifRing - (wr - rdbyte) >= 255u) {
            if (p < wbase || p + 256 > wbase + kGifWin) {
                wbase = p - (int64_t)(reinterpret_cast<uintptr_t>(d + p) & 15);
                wave_sync();  // the window's readers are done
                fill_window(win, d, n, wbase, kGifWin, lane, 64);
                wave_sync();
            }
            if (p >= n) { ended = kGifEndFile; break; }
            const int sz = __builtin_amdgcn_readfirstlane((int)win[p - wbase]);
            if (sz == 0) { ended = kGifEndTerm; break; }
            const int avail = (int)min<int64_t>(sz, n - (p + 1));
            for (int j = lane; j < avail; j += 64) ring[(wr + j) & (kGifRing - 1)] = win[p + 1 + j - wbase];
            wr += avail;
            if (avail < sz) { ended = kGifEndFile; break; }
            p += 1 + sz;
        }
        wave_sync();

        // 64 codes at once
        const uint32_t availbits = (wr - rdbyte) * 8 - rdbit;
        const uint32_t t = t0 + lane;
        const uint32_t off0 = (uint32_t)gif_code_offset(mcs, t0);  // (a difference of two: the wrap cancels)
        const uint32_t rel = (uint32_t)gif_code_offset(mcs, t) - off0;
        const int width = gif_code_width(mcs, t);
        const bool has = rel + width <= availbits;
        const uint32_t bit = rdbit + rel, b0 = rdbyte + (bit >> 3);
        const uint32_t v = ring[b0 & (kGifRing - 1)] | ring[(b0 + 1) & (kGifRing - 1)] << 8 | ring[(b0 + 2) & (kGifRing - 1)] << 16;
        const int code = (int)((v >> (bit & 7)) & ((1u << width) - 1));
        const bool isclear = has && code == clear, isstop = has && code == clear + 1;
        const int j = code - (clear + 2);  // the code's entry was made from code number j and its successor
        const bool invalid = has && !isclear && !isstop && (t == 0 ? code >= clear : (j >= 0 && (uint32_t)j > t - 1));
        const uint64_t evmask = __ballot(!has || isclear || isstop || invalid);
        const int m0 = evmask ? __builtin_ctzll(evmask) : 64;
        const bool act = lane < m0;

        const LzwRound R = lzw_resolve(code, act, t0, clear, npix, C, tab, first, lane);
        lzw_enter(R, code, t, clear, C, tab, first, lane);
        if (R.need) {  // the index plane is the clipped frame rectangle: interlace map and clipping per row
            const uint32_t Lcut = R.cut();
            const uint32_t pe = C.base + R.excl + R.L - 1;  // (< 2^32: npix <= 65535^2, L < 4096)
            uint32_t y = pe / fw, x = pe - y * fw;
            uint32_t ym = H.interlace && y < (uint32_t)H.fh ? (uint32_t)gif_interlace_row(H.fh, (int)y) : y;
            lzw_walk(R, code, tab, [&](uint32_t k, int s) {
                if (k < Lcut && x < cw && ym < ch) pl[(uint64_t)ym * cw + x] = (uint8_t)s;
                if (k > 0 && x == 0) {  // on to the byte before
                    x = fw - 1;
                    --y;
                    ym = H.interlace && y < (uint32_t)H.fh ? (uint32_t)gif_interlace_row(H.fh, (int)y) : y;
                } else {
                    --x;
                }
            });
        }
        lzw_carry(C, R, code, npix);
        if (C.base >= npix) break;
        // (not complete: R.m == m0)
        uint32_t adv;
        if (m0 == 64) {
            adv = (uint32_t)gif_code_offset(mcs, t0 + 64) - off0;
            t0 += 64;
        } else {
            adv = __shfl(rel, m0);
            const bool e_has = __shfl((int)has, m0), e_clear = __shfl((int)isclear, m0), e_stop = __shfl((int)isstop, m0);
            if (!e_has) {
                if (ended == kGifEndNone) {
                    if (m0 == 0) { status = -1; break; }  // (the ring holds 64 codes whenever the data goes on)
                } else {
                    if (ended == kGifEndFile) status = kGifTruncated;
                    break;
                }
                t0 += m0;
            } else if (e_stop) {
                break;
            } else if (e_clear) {
                adv += __shfl(width, m0);
                t0 = 0;
            } else {
                status = kGifBadData;
                break;
            }
        }
        rdbit += adv;
        rdbyte += rdbit >> 3;
        rdbit &= 7;
    }
    if (lane == 0) {
        dd.produced = C.base;
        dd.status = status;
    }
}

// grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_gif_render(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                    const GifDesc* __restrict__ desc, const uint8_t* __restrict__ plane,
                                                    uint64_t plane_stride, uint8_t* __restrict__ out, uint64_t out_stride) {
    __shared__ uint32_t pal[256];
    __shared__ __attribute__((aligned(16))) uint8_t seg[kGifSeg * 3 + 16];
    const int i = blockIdx.y, tid = threadIdx.x;
    const GifDesc& dd = desc[i];
    if (dd.status != kGifOk) return;
    const GifHead H = dd.H;
    const uint8_t* file = data + off[i];
    const uint8_t* pl = plane + (uint64_t)i * plane_stride;
    uint8_t* dst = out + (uint64_t)i * out_stride;
    {
        uint32_t c = 0;
        if (H.has_image && tid < H.pal_size) {  // (the table lies inside the file: gif_parse)
            const uint8_t* e = file + H.pal_at + 3 * tid;
            c = e[0] | e[1] << 8 | e[2] << 16;
        }
        pal[tid] = c;
    }
    const int cw = H.has_image ? min(H.fw, H.w - H.fx) : 0, ch = H.has_image ? min(H.fh, H.h - H.fy) : 0;
    const uint32_t produced = dd.produced;
    for (int y = blockIdx.x; y < H.h; y += gridDim.x) {
        const int fr = y - H.fy;  // frame row
        const bool inrow = fr >= 0 && fr < ch;
        const uint32_t sr = inrow ? (uint32_t)(H.interlace ? gif_interlace_stream_row(H.fh, fr) : fr) : 0;
        for (int x0 = 0; x0 < H.w; x0 += kGifSeg) {
            const int nx = min(kGifSeg, H.w - x0);
            __syncthreads();  // the previous segment's readers are done (and pal is in)
            for (int x = tid; x < nx; x += 256) {
                uint32_t rgb = (uint32_t)H.bg_rgb;
                const int fc = x0 + x - H.fx;  // frame column
                if (inrow && fc >= 0 && fc < cw) {
                    const int idx = sr * (uint32_t)H.fw + (uint32_t)fc < produced ? pl[(uint64_t)fr * cw + fc] : H.bg_index;
                    if (idx != H.transparent) rgb = pal[idx];
                }
                seg[3 * x] = (uint8_t)rgb;
                seg[3 * x + 1] = (uint8_t)(rgb >> 8);
                seg[3 * x + 2] = (uint8_t)(rgb >> 16);
            }
            __syncthreads();
            store_segment(dst + ((int64_t)y * H.w + x0) * 3, nx * 3, tid, [&](int q) -> uint32_t { return seg[q]; });
        }
    }
}

__global__ void k_gif_finish(int n, const GifDesc* __restrict__ desc, int32_t* __restrict__ status,
                             int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GifDesc& dd = desc[i];
    const bool ok = dd.status == kGifOk;
    status[i] = dd.status;
    dims[3 * i + 0] = ok ? dd.H.w : 0;
    dims[3 * i + 1] = ok ? dd.H.h : 0;
    dims[3 * i + 2] = ok ? 3 : 0;
}

// ------------------------------------------------------------------------------- host
int gif_probe(const uint8_t* data, int64_t size, int* w, int* h) {
    GifHead H{};
    const int rc = gif_parse(data, size, &H);
    if (rc == kGifOk) { *w = H.w; *h = H.h; }
    return rc;
}

bool gif_ws_alloc(GifWs& ws, Blocks& mem, int max_images, int max_w, int max_h) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.plane_stride = ((int64_t)max_w * max_h + 15) & ~(int64_t)15;
    const size_t n = (size_t)max_images;
    return mem.alloc(ws.desc, n * sizeof(GifDesc)) && mem.alloc(ws.plane, n * (size_t)ws.plane_stride);
}

void launch_gif_decode(const GifWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    const int nb = (n + 63) / 64;
    S.begin(kStParse);
    hipLaunchKernelGGL(k_gif_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.max_w, ws.max_h);
    S.end(kStParse);
    S.begin(kStEntropy);
    hipLaunchKernelGGL(k_gif_lzw, dim3(n), dim3(64), 0, st, d_data, d_off, ws.desc, ws.plane, (uint64_t)ws.plane_stride);
    S.end(kStEntropy);
    S.begin(kStConvert);
    hipLaunchKernelGGL(k_gif_render, dim3(rows_grid(ws.max_h, n), n), dim3(256), 0, st,
                       d_data, d_off, ws.desc, ws.plane, (uint64_t)ws.plane_stride, d_out, out_stride);
    hipLaunchKernelGGL(k_gif_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    S.end(kStConvert);
}

}  // namespace icx
