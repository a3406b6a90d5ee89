// icx_pngd.hip -- PNG read on gfx950: Image::readPng (codecs.cpp:903-1020) -> 8-bit RGBA, rows
// top-down. The reference hands the file to libpng; the sample conversions here are the PNG
// specification's, which is what its libpng calls (:967-982) implement.
//
// A PNG is one zlib stream cut into IDAT chunks, so an image inflates on one wave and the
// throughput comes from the batch:
//   k_pngd_parse     one lane per image: the chunk walk (icx_pngd_core.h) into the descriptor
//   k_pngd_gather    the IDAT payloads of an image concatenated into one stream
//   k_pngd_inflate   one wave per image: exr_inflate_wave (icx_inflate_wave.h) into the image's
//                    scratch, exactly h * (1 + lb) filtered bytes or BAD_DATA
//   k_pngd_unfilter  one wave per image, bands of 64 rows on the anti-diagonal, in place
//   k_pngd_expand    samples -> RGBA8 (sub-byte unpack, palette, tRNS key, 16 -> 8 bits)
//   k_pngd_finish    status and dims per image
// Device-resident inputs, no host read-back, every launch on the caller's stream. A failed image
// leaves the others alone; its pixels are unspecified.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "icx_inflate_wave.h"
#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_pngd_core.h"

namespace icx {

struct PngdDesc {
    int32_t status, pad_;
    int64_t size;
    PngdInfo I;
};

__global__ void k_pngd_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                             const uint64_t* __restrict__ size, PngdDesc* __restrict__ desc, int max_w, int max_h,
                             int64_t zcap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PngdDesc& dd = desc[i];
    dd.size = (int64_t)size[i];
    int st = pngd_walk(data + off[i], dd.size, dd.I);
    if (st == kPngrOk && (dd.I.w > max_w || dd.I.h > max_h)) st = kPngrTooLarge;
    // (a stream longer than any deflate of the batch's largest image: it cannot inflate to h * (1 + lb))
    if (st == kPngrOk && dd.I.idat_bytes > zcap) st = kPngrBadData;
    dd.status = st;
}

// grid (x: pieces of the stream, y: image). Every workgroup walks the image's IDAT chain (a few
// bytes per chunk) and copies the part of each payload that falls into its piece of the stream.
// The stream starts at z + i * zcap, 16-byte aligned; InW::ld loads no byte past its end.
__global__ __launch_bounds__(256) void k_pngd_gather(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                     const PngdDesc* __restrict__ desc, uint8_t* __restrict__ z,
                                                     int64_t zcap) {
    const int i = blockIdx.y;
    const PngdDesc& dd = desc[i];
    if (dd.status != kPngrOk) return;
    const uint8_t* d = data + off[i];
    const int64_t n = dd.size, total = dd.I.idat_bytes;
    const int64_t per = ((total + gridDim.x - 1) / gridDim.x + 255) & ~(int64_t)255;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = min<int64_t>(total, lo + per);
    if (lo >= hi) return;
    uint8_t* zi = z + (int64_t)i * zcap;
    int64_t acc = 0;
    for (int64_t p = dd.I.first_idat; p >= 0 && acc < hi; p = pngd_idat_next(d, n, p)) {
        const int64_t len = (int64_t)pngd_be32(d + p);
        const int64_t a = max<int64_t>(acc, lo), b = min<int64_t>(acc + len, hi);  // (acc + len <= total <= zcap)
        for (int64_t k = a + threadIdx.x; k < b; k += blockDim.x) zi[k] = d[p + 8 + (k - acc)];
        acc += len;
    }
}

constexpr int kPngdWin = 16384;  // the inflate's LDS ring (matches farther back come from the flushed output)
__global__ __launch_bounds__(64) void k_pngd_inflate(PngdDesc* __restrict__ desc, const uint8_t* __restrict__ z, int64_t zcap,
                                                     uint8_t* __restrict__ scr, int64_t scap) {
    __shared__ InfState st;
    __shared__ __attribute__((aligned(16))) uint8_t win[kPngdWin];
    const int i = blockIdx.x;
    PngdDesc& dd = desc[i];
    if (dd.status != kPngrOk) return;
    const int64_t want = (int64_t)dd.I.h * (1 + (int64_t)dd.I.lb);  // (<= scap: w <= max_w, h <= max_h)
    int64_t m = 0;
    const bool ok = exr_inflate_wave<kPngdWin>(z + (int64_t)i * zcap, dd.I.idat_bytes, scr + (int64_t)i * scap, want, &m, st, win);
    // (more than `want` bytes fail inside the inflate, before a byte past `want` is stored)
    if (threadIdx.x == 0 && (!ok || m != want)) dd.status = kPngrBadData;
}

// ---------------------------------------------------------------------------- the un-filter
// Paeth and Average make a row serial along its filter units (bw bytes), and every row needs the
// row above: the parallelism is the anti-diagonal. One wave per image works through bands of 64
// rows; lane k owns row 64 * band + k and at step t reconstructs unit t - k. The unit above (b)
// is what lane k - 1 produced one step earlier (a lane shift), the unit above-left (c) is the b
// of the step before, the unit to the left (a) is the lane's own previous result: all three stay
// in registers. Lane 0's row above is the previous band's last row, which the same wave stored
// through memory: the band starts by waiting for those stores, and the row is then loaded 64
// units at a time (lane j: unit t + j, every 64 steps) with agent-scope loads, which do not
// return a line the L1 held from before the stores; lane 0 takes unit t from lane t mod 64.
template <int BW>
struct PngdUnit {
    using T = typename std::conditional<(BW > 4), uint64_t, uint32_t>::type;
};
template <int BW>
__device__ __forceinline__ typename PngdUnit<BW>::T pngd_ld_unit(const uint8_t* p) {
    typename PngdUnit<BW>::T v = 0;
#pragma unroll
    for (int j = 0; j < BW; ++j) v |= (typename PngdUnit<BW>::T)p[j] << (8 * j);
    return v;
}
template <int BW>
__device__ __forceinline__ typename PngdUnit<BW>::T pngd_ld_unit_fresh(uint8_t* p) {
    typename PngdUnit<BW>::T v = 0;
#pragma unroll
    for (int j = 0; j < BW; ++j)
        v |= (typename PngdUnit<BW>::T)__hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << (8 * j);
    return v;
}
// Reconstruction of one unit (PNG spec 9.2-9.4), byte by byte; ft is the row's filter type, 0..4.
template <int BW>
__device__ __forceinline__ typename PngdUnit<BW>::T pngd_recon(int ft, typename PngdUnit<BW>::T x, typename PngdUnit<BW>::T a,
                                                               typename PngdUnit<BW>::T b, typename PngdUnit<BW>::T c) {
    typename PngdUnit<BW>::T r = 0;
#pragma unroll
    for (int j = 0; j < BW; ++j) {
        const int xa = (int)((a >> (8 * j)) & 255u), xb = (int)((b >> (8 * j)) & 255u), xc = (int)((c >> (8 * j)) & 255u);
        const int pa = abs(xb - xc), pb = abs(xa - xc), pc = abs(xa + xb - 2 * xc);
        const int paeth = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        const int pred = ft == 1 ? xa : ft == 2 ? xb : ft == 3 ? (xa + xb) >> 1 : ft == 4 ? paeth : 0;
        r |= (typename PngdUnit<BW>::T)(((int)((x >> (8 * j)) & 255u) + pred) & 255) << (8 * j);
    }
    return r;
}
// The h rows of 1 + lb bytes at s, in place. false: a filter byte above 4.
template <int BW>
__device__ bool pngd_unfilter_image(uint8_t* s, int h, int lb) {
    using U = typename PngdUnit<BW>::T;
    const int lane = (int)__lane_id();
    const int nu = lb / BW;  // (lb is a multiple of bw; at least 1)
    const int64_t stride = 1 + (int64_t)lb;
    bool bad = false;
    for (int y0 = 0; y0 < h; y0 += 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (row y0 - 1: the previous band's stores)
        const int rows = min(64, h - y0);
        const bool live = lane < rows;
        uint8_t* rp = s + (int64_t)(y0 + (live ? lane : 0)) * stride + 1;
        int ft = live ? (int)rp[-1] : 0;
        if (ft > 4) {
            bad = true;
            ft = 0;
        }
        uint8_t* up = y0 > 0 ? s + (int64_t)(y0 - 1) * stride + 1 : nullptr;  // (row 0's prior is zero)
        U a = 0, bp = 0, res = 0, above = 0;
        U x = live && lane == 0 ? pngd_ld_unit<BW>(rp) : (U)0;
        const int steps = nu + rows - 1;
        for (int t = 0; t < steps; ++t) {
            if ((t & 63) == 0) {
                const int ua = t + lane;
                above = up && ua < nu ? pngd_ld_unit_fresh<BW>(up + (int64_t)ua * BW) : (U)0;
            }
            const int u = t - lane;
            const bool act = live && u >= 0 && u < nu;
            // (the next step's unit is loaded before this step's result is stored: other bytes)
            const U xn = live && u + 1 >= 0 && u + 1 < nu ? pngd_ld_unit<BW>(rp + (int64_t)(u + 1) * BW) : (U)0;
            U b = __shfl_up(res, 1);
            const U b0 = __shfl(above, t & 63);
            if (lane == 0) b = b0;
            if (act) {
                res = pngd_recon<BW>(ft, x, a, b, bp);
                uint8_t* q = rp + (int64_t)u * BW;
#pragma unroll
                for (int j = 0; j < BW; ++j) q[j] = (uint8_t)(res >> (8 * j));
                a = res;
                bp = b;
            } else {
                res = 0;
                a = 0;
                bp = 0;
            }
            x = xn;
        }
    }
    return !__any(bad);
}

__global__ __launch_bounds__(64) void k_pngd_unfilter(PngdDesc* __restrict__ desc, uint8_t* __restrict__ scr, int64_t scap) {
    const int i = blockIdx.x;
    PngdDesc& dd = desc[i];
    if (dd.status != kPngrOk) return;
    uint8_t* s = scr + (int64_t)i * scap;
    const int h = dd.I.h, lb = dd.I.lb;
    bool ok = true;
    switch (dd.I.bw) {  // (wave-uniform)
        case 1: ok = pngd_unfilter_image<1>(s, h, lb); break;
        case 2: ok = pngd_unfilter_image<2>(s, h, lb); break;
        case 3: ok = pngd_unfilter_image<3>(s, h, lb); break;
        case 4: ok = pngd_unfilter_image<4>(s, h, lb); break;
        case 6: ok = pngd_unfilter_image<6>(s, h, lb); break;
        default: ok = pngd_unfilter_image<8>(s, h, lb); break;
    }
    if (threadIdx.x == 0 && !ok) dd.status = kPngrBadData;
}

// ---------------------------------------------------------------------------- samples -> RGBA8
// Pixel x of an un-filtered row as R | G << 8 | B << 16 | A << 24:
//   16-bit samples keep the high byte (png_set_strip_16); grey of 1 / 2 / 4 bits is scaled by
//   255 / (2^bd - 1); a palette index takes PLTE's colour and tRNS's alpha (pal[]: 255 without
//   one, (0, 0, 0, 255) past PLTE); grey is replicated; alpha is the file's for colour types 4
//   and 6, and for 0 and 2 with a tRNS key 0 where the samples at file precision equal the key.
__device__ __forceinline__ uint32_t pngd_pixel(int ct, int bd, bool has_key, uint32_t k0, uint32_t k1, uint32_t k2,
                                               const uint32_t* pal, const uint8_t* row, int x) {
    if (bd < 8) {  // colour types 0 and 3
        const int bit = x * bd;
        const uint32_t v = ((uint32_t)row[bit >> 3] >> (8 - bd - (bit & 7))) & ((1u << bd) - 1u);
        if (ct == 3) return pal[v];
        const uint32_t g = v * (255u / ((1u << bd) - 1u));
        return g * 0x010101u | (has_key && v == k0 ? 0u : 0xFF000000u);
    }
    const int sb = bd >> 3;  // bytes per sample
    auto full = [&](int k) { return sb == 1 ? (uint32_t)row[k] : (uint32_t)row[2 * k] << 8 | row[2 * k + 1]; };
    auto hi = [&](uint32_t v) { return sb == 1 ? v : v >> 8; };
    switch (ct) {
        case 0: {
            const uint32_t v = full(x);
            return hi(v) * 0x010101u | (has_key && v == k0 ? 0u : 0xFF000000u);
        }
        case 2: {
            const uint32_t r = full(3 * x), g = full(3 * x + 1), b = full(3 * x + 2);
            return hi(r) | hi(g) << 8 | hi(b) << 16 | (has_key && r == k0 && g == k1 && b == k2 ? 0u : 0xFF000000u);
        }
        case 3: return pal[row[x]];
        case 4: return hi(full(2 * x)) * 0x010101u | hi(full(2 * x + 1)) << 24;
        default: return hi(full(4 * x)) | hi(full(4 * x + 1)) << 8 | hi(full(4 * x + 2)) << 16 | hi(full(4 * x + 3)) << 24;
    }
}

// grid (x: pixel chunks, y: image). The image as a flat run of w * h pixels, four per lane: one
// 16-byte store where the image's output is 16-byte aligned, else four 4-byte stores.
__global__ __launch_bounds__(256) void k_pngd_expand(const PngdDesc* __restrict__ desc, const uint8_t* __restrict__ scr,
                                                     int64_t scap, uint8_t* __restrict__ out, uint64_t out_stride) {
    __shared__ uint32_t pal[256];
    const int i = blockIdx.y;
    const PngdDesc& dd = desc[i];
    if (dd.status != kPngrOk) return;
    pal[threadIdx.x] = dd.I.pal[threadIdx.x];
    __syncthreads();
    const int w = dd.I.w, ct = dd.I.ct, bd = dd.I.bd;
    const bool has_key = dd.I.has_key != 0;
    const uint32_t k0 = dd.I.key[0], k1 = dd.I.key[1], k2 = dd.I.key[2];
    const uint32_t npx = (uint32_t)w * (uint32_t)dd.I.h;  // (<= 2^24)
    const int64_t stride = 1 + (int64_t)dd.I.lb;
    const uint8_t* s = scr + (int64_t)i * scap;
    uint8_t* o = out + (uint64_t)i * out_stride;
    const bool vec = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; 4u * q < npx; q += gridDim.x * blockDim.x) {
        const uint32_t p0 = 4u * q;
        int y = (int)(p0 / (uint32_t)w), x = (int)(p0 - (uint32_t)y * (uint32_t)w);
        uint32_t v[4] = {0, 0, 0, 0};
        const int cnt = (int)min(4u, npx - p0);
        for (int k = 0; k < cnt; ++k) {
            v[k] = pngd_pixel(ct, bd, has_key, k0, k1, k2, pal, s + (int64_t)y * stride + 1, x);
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<uint4*>(o + 4ull * p0) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < cnt; ++k) *reinterpret_cast<uint32_t*>(o + 4ull * (p0 + k)) = v[k];
        }
    }
}

__global__ void k_pngd_finish(int n, const PngdDesc* __restrict__ desc, int32_t* __restrict__ status, int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PngdDesc& dd = desc[i];
    const bool ok = dd.status == kPngrOk;
    status[i] = dd.status;
    dims[3 * i + 0] = ok ? dd.I.w : 0;
    dims[3 * i + 1] = ok ? dd.I.h : 0;
    dims[3 * i + 2] = ok ? 4 : 0;
}

// ------------------------------------------------------------------------------- host
int pngd_probe(const uint8_t* data, int64_t size, int* w, int* h) {
    PngdInfo I;
    const int rc = pngd_walk(data, size, I);
    *w = rc == kPngrOk ? I.w : 0;
    *h = rc == kPngrOk ? I.h : 0;
    return rc;
}

// Per image: the filtered bytes (up to 8 bytes per pixel and one filter byte per row), and the
// gathered zlib stream (stored blocks add 5 bytes per 64 KiB; room for a writer with shorter ones).
bool pngd_ws_alloc(PngdWs& ws, Blocks& mem, int max_images, int max_w, int max_h) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    const int64_t raw = (int64_t)max_h * (1 + 8 * (int64_t)max_w);
    ws.scap = (raw + 15) & ~(int64_t)15;
    ws.zcap = (raw + raw / 256 + 1024 + 15) & ~(int64_t)15;
    const size_t n = (size_t)max_images;
    return mem.alloc(ws.desc, n * sizeof(PngdDesc)) && mem.alloc(ws.scr, n * (size_t)ws.scap) &&
           mem.alloc(ws.z, n * (size_t)ws.zcap);
}

void launch_pngd_decode(const PngdWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                        uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                        StageHook* hook) {
    if (n <= 0) return;
    auto B = [&](Stage s) { if (hook) hook->begin(s, st); };
    auto E = [&](Stage s) { if (hook) hook->end(s, st); };
    const int nb = (n + 63) / 64;
    const int per = std::max(1, 16384 / n);  // workgroups per image at most
    B(kStParse);
    hipLaunchKernelGGL(k_pngd_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.max_w, ws.max_h, ws.zcap);
    E(kStParse);
    B(kStUnstuff);  // gather
    const int gz = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(per, 64), ws.zcap / 65536));
    hipLaunchKernelGGL(k_pngd_gather, dim3(gz, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.z, ws.zcap);
    E(kStUnstuff);
    B(kStEntropy);  // inflate
    hipLaunchKernelGGL(k_pngd_inflate, dim3(n), dim3(64), 0, st, ws.desc, ws.z, ws.zcap, ws.scr, ws.scap);
    E(kStEntropy);
    B(kStIdct);  // un-filter
    hipLaunchKernelGGL(k_pngd_unfilter, dim3(n), dim3(64), 0, st, ws.desc, ws.scr, ws.scap);
    E(kStIdct);
    B(kStConvert);  // expand
    const int64_t quads = ((int64_t)ws.max_w * ws.max_h + 3) / 4;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(per, (quads + 255) / 256));
    hipLaunchKernelGGL(k_pngd_expand, dim3(gx, n), dim3(256), 0, st, ws.desc, ws.scr, ws.scap, d_out, out_stride);
    hipLaunchKernelGGL(k_pngd_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    E(kStConvert);
}

}  // namespace icx
