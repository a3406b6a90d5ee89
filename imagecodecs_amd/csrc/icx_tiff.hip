// icx_tiff.hip -- TIFF read on gfx950: Image::readTiff (codecs.cpp:1439-1484, libtiff's
// TIFFReadRGBAImage), with the contract and deviations of include/icx.h.
//
//   k_tiff_parse   IFD walk (tiff_parse), one lane per image -> descriptor record and chunk count
//   k_tiff_scan    exclusive scan of the chunk counts over the batch: item j of the work list is
//                  chunk j - first[i] of the image i with first[i] <= j < first[i + 1]
//   k_tiff_unpack  a fixed grid (sized from the CU count: the host does not know the chunk counts),
//                  one wave per workgroup; each wave takes the next item of the work list from a
//                  counter (chunks differ in cost, and more workgroups are launched than are
//                  resident) and decompresses one strip or tile at a time into the chunk's room of
//                  the image's scratch:
//                    zlib      exr_inflate_wave (icx_inflate_wave.h), unchanged
//                    LZW       64 codes at once as in k_gif_lzw: between two Clears the k-th code's
//                              bit offset and width are a closed form (tiff_code_offset /
//                              tiff_code_width), a ballot finds the first Clear / EOI / invalid /
//                              missing code, lengths and first bytes of entries born in the same 64
//                              come by pointer doubling, a wave scan places every string, and the
//                              lanes walk their chains back to front. Codes are MSB first and read
//                              from an LDS window staged straight from the chunk's bytes.
//                    PackBits  the wave walks the packet headers, all lanes copy or fill
//                    none      only the extent check; k_tiff_render reads the file's bytes
//   k_tiff_render  a workgroup per image row: predictor 2 undone as a packed per-channel running sum
//                  (thread-local, then a workgroup scan, then the carry of the row so far; it
//                  restarts at every chunk row), MinIsWhite / ColorMap, tile clipping; a row segment
//                  is assembled in LDS and leaves as 16-byte stores at the destination's alignment.
//   k_tiff_finish  status (the lowest failing chunk's code) and dims
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_tiff_core.h"
#include "icx_inflate_wave.h"
#include "icx_wave.h"

namespace icx {

constexpr int kTiffWin = 2048;       // chunk bytes staged per window load of the LZW wave (tests/test_gpu_tiff.py names it)
constexpr int kTiffWinNeed = 128;    // bytes one round of 64 codes can touch (64 * 12 bits, 7 bits of phase, 2 bytes of slack)
constexpr int kTiffSeg = 1024;       // pixels per row segment of k_tiff_render
constexpr int kTiffInfWin = 16384;   // the inflate's LDS ring
constexpr uint32_t kTiffNoFail = 0xFFFFFFFFu;

struct TiffDesc {
    TiffHead H;
    int64_t size;
    int32_t status;  // of the parse
    uint32_t fail;   // min over failing chunks of chunk << 8 | code (k_tiff_unpack)
};

__global__ void k_tiff_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                             const uint64_t* __restrict__ size, TiffDesc* __restrict__ desc, int32_t* __restrict__ count,
                             int max_w, int max_h, uint64_t slot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TiffDesc dd{};
    dd.size = (int64_t)size[i];
    dd.fail = kTiffNoFail;
    dd.status = tiff_parse(data + off[i], dd.size, &dd.H);
    if (dd.status == kTiffOk && (dd.H.w > max_w || dd.H.h > max_h || tiff_scratch_need(dd.H) > slot)) dd.status = kTiffTooLarge;
    desc[i] = dd;
    count[i] = dd.status == kTiffOk ? dd.H.nchunks : 0;
}

// One workgroup of 256: first[0] = 0, first[i + 1] = first[i] + count[i].
__global__ __launch_bounds__(256) void k_tiff_scan(int n, const int32_t* __restrict__ count, int32_t* __restrict__ first,
                                                   uint32_t* __restrict__ next) {
    __shared__ int32_t sc[256];
    const int tid = threadIdx.x;
    int32_t carry = 0;
    if (tid == 0) {
        first[0] = 0;
        *next = 0;  // k_tiff_unpack's work counter
    }
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int32_t v = i < n ? count[i] : 0;
        sc[tid] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int32_t t = tid >= s ? sc[tid - s] : 0;
            __syncthreads();
            sc[tid] += t;
            __syncthreads();
        }
        if (i < n) first[i + 1] = carry + sc[tid];
        carry += sc[255];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------- chunk decoders (one wave)
__device__ __forceinline__ int tiff_lzw_wave(const uint8_t* __restrict__ s, int64_t cnt, uint8_t* __restrict__ dst, uint32_t want,
                                             uint32_t* tab, uint8_t* first, uint8_t* win, int lane) {
    if (tiff_lzw_old_style(s, cnt)) return kTiffUnsupported;
    const uint64_t nbits = (uint64_t)cnt * 8;
    if (nbits < 9 || tiff_msb_bits(s, cnt, 0, 9) != 256) return kTiffBadData;  // the first code is a Clear
    uint64_t rd = 9;                    // bit position of code t0
    int64_t wbase = INT64_MIN / 2;      // chunk offset of win[0]
    uint32_t t0 = 0, base = 0;          // the next code's number after the last Clear; bytes produced
    int prev_code = 0, prev_F = 0;      // of code t0 - 1 (t0 > 0)
    uint32_t prev_L = 0;
    constexpr int clear = 256;

    while (base < want) {
        const int64_t b_lo = (int64_t)(rd >> 3);
        if (b_lo < wbase || b_lo + kTiffWinNeed > wbase + kTiffWin) {
            wbase = b_lo - (int64_t)(reinterpret_cast<uintptr_t>(s + b_lo) & 15);
            wave_sync();  // the window's readers are done
            fill_window(win, s, cnt, wbase, kTiffWin, lane, 64);
            wave_sync();
        }
        // 64 codes at once
        const uint32_t t = t0 + lane;
        const uint64_t off0 = tiff_code_offset(t0);
        const uint32_t rel = (uint32_t)(tiff_code_offset(t) - off0);
        const int width = tiff_code_width(t);
        const uint64_t bit = rd + rel;
        const bool has = bit + width <= nbits;
        const uint32_t wb = (uint32_t)((int64_t)(bit >> 3) - wbase);  // (+ 2 < kTiffWin)
        const uint32_t v = (uint32_t)win[wb] << 16 | (uint32_t)win[wb + 1] << 8 | win[wb + 2];
        const int code = (int)((v >> (24 - (int)(bit & 7) - width)) & ((1u << width) - 1));
        const bool isclear = has && code == clear, isstop = has && code == clear + 1;
        const int j = code - (clear + 2);  // the code's entry was made from code number j and its successor
        const bool invalid = has && !isclear && !isstop &&
                             (t == 0 ? code >= clear : ((j >= 0 && (uint32_t)j > t - 1) || t > (uint32_t)kTiffLzwLastT));
        const uint64_t evmask = __ballot(!has || isclear || isstop || invalid);
        const int m0 = evmask ? __builtin_ctzll(evmask) : 64;
        const bool act = lane < m0;

        // (icx_lzw_wave.h's round written out: shared, it moved this kernel's deflate path by 1.1 %)
        // string length L and first byte F of every code before the event
        uint32_t A = 0;
        int D = -1, F = 0;
        if (act) {
            if (code < clear) { A = 1; F = code; }
            else if ((uint32_t)j >= t0) { A = 1; D = (int)((uint32_t)j - t0); }  // made by this round's codes: a lower lane
            else if ((uint32_t)j + 1 == t0) { A = prev_L + 1; F = prev_F; }        // made by lane 0 of this round
            else { A = tab[code] >> 20; F = first[code]; }
        }
        while (__any(D >= 0)) {
            const int src = D < 0 ? lane : D;
            const uint32_t a2 = __shfl(A, src);
            const int f2 = __shfl(F, src), d2 = __shfl(D, src);
            if (D >= 0) { A += a2; F = f2; D = d2; }
        }
        const uint32_t L = A;
        const uint32_t incl = wave_sum_scan(L, lane), excl = incl - L;
        const uint32_t rem = want - base;
        const bool need = act && excl < rem;  // the code starts before the last byte: a prefix of the lanes
        const int m = __popcll(__ballot(need));

        // their table entries: code t >= 1 makes entry 257 + t from code t - 1 and its own first byte
        int pc = __shfl_up(code, 1), pF = __shfl_up(F, 1);
        uint32_t pL = __shfl_up(L, 1);
        if (lane == 0) { pc = prev_code; pF = prev_F; pL = prev_L; }
        if (need && t >= 1 && (uint32_t)clear + 1 + t < 4096u) {
            tab[clear + 1 + t] = (uint32_t)pc | (uint32_t)(F & 255) << 12 | (pL + 1) << 20;
            first[clear + 1 + t] = (uint8_t)pF;
        }
        wave_sync();

        // every lane walks its own string back to front
        if (need) {
            const uint32_t Lcut = min(L, rem - excl);
            uint8_t* o = dst + base + excl;
            int c = code;
            for (uint32_t k = L - 1;; --k) {
                int b = c;
                if (k > 0) {
                    const uint32_t e = tab[c];
                    b = (e >> 12) & 255;
                    c = e & 0xFFF;
                }
                if (k < Lcut) o[k] = (uint8_t)b;
                if (k == 0) break;
            }
        }
        wave_sync();  // the table is read before the next round's entries go in

        if (m > 0) {
            const uint32_t total = __shfl(incl, m - 1);
            base = total >= rem ? want : base + total;
            prev_code = __shfl(code, m - 1);
            prev_F = __shfl(F, m - 1);
            prev_L = __shfl(L, m - 1);
        }
        if (base >= want) break;
        // (not complete: m == m0)
        if (m0 == 64) {
            rd += tiff_code_offset(t0 + 64) - off0;
            t0 += 64;
        } else {
            const bool e_clear = __shfl((int)isclear, m0);
            if (!e_clear) return kTiffBadData;  // the data ends, an EOI before the last byte, or an invalid code
            rd += __shfl(rel, m0) + (uint32_t)__shfl(width, m0);
            t0 = 0;
        }
    }
    return kTiffOk;
}

__device__ __forceinline__ int tiff_packbits_wave(const uint8_t* __restrict__ s, int64_t cnt, uint8_t* __restrict__ dst, uint32_t want,
                                                  int lane) {
    int64_t p = 0;
    uint32_t out = 0;
    while (out < want) {
        if (p >= cnt) return kTiffBadData;
        const int hb = __builtin_amdgcn_readfirstlane((int)s[p]);
        if (hb == 128) { ++p; continue; }
        const uint32_t m = hb < 128 ? (uint32_t)hb + 1u : 257u - (uint32_t)hb;
        const int64_t need = hb < 128 ? 1 + (int64_t)m : 2;
        if (p + need > cnt) return kTiffBadData;
        const uint32_t mm = min(m, want - out);
        if (hb < 128) {
            for (uint32_t k = lane; k < mm; k += 64) dst[out + k] = s[p + 1 + k];
        } else {
            const uint8_t b = s[p + 1];
            for (uint32_t k = lane; k < mm; k += 64) dst[out + k] = b;
        }
        out += mm;
        p += need;
    }
    return kTiffOk;
}

// The LDS of one wave: the LZW table, first bytes and window, or the inflate's state and ring.
constexpr int kTiffLds = 4096 * 4 + 4096 + kTiffWin;
static_assert(kTiffLds >= kTiffInfWin + (int)sizeof(InfState), "the inflate's ring and tables fit");

__global__ __launch_bounds__(64) void k_tiff_unpack(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                    TiffDesc* __restrict__ desc, const int32_t* __restrict__ first,
                                                    uint32_t* __restrict__ next, uint8_t* __restrict__ scratch, uint64_t slot) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTiffLds];
    const int lane = threadIdx.x;
    const uint32_t total = (uint32_t)first[n];
    for (;;) {
        uint32_t taken = 0;
        if (lane == 0) taken = atomicAdd(next, 1u);  // (at most total + gridDim.x increments: no wrap)
        const uint32_t item = __builtin_amdgcn_readfirstlane(taken);
        if (item >= total) break;
        int lo = 0, hi = n - 1;  // the last image with first[i] <= item
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((uint32_t)first[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const int i = lo, k = (int)item - first[i];
        TiffDesc& dd = desc[i];
        const TiffHead& H = dd.H;
        const uint8_t* f = data + off[i];
        const TiffChunk c = tiff_chunk(H, k);
        const int64_t coff = tiff_elem(f, H.off_at, H.off_type, H.be, k), cnt = tiff_elem(f, H.cnt_at, H.cnt_type, H.be, k);
        uint8_t* dst = scratch + (uint64_t)i * slot + (uint64_t)k * tiff_chunk_room(H);
        const int comp = H.comp;
        int rc = kTiffOk;
        if (coff + cnt > dd.size) {
            rc = kTiffTruncated;
        } else if (comp == 1) {
            if (cnt < (int64_t)c.want) rc = kTiffBadData;
        } else if (comp == 5) {
            wave_sync();  // the previous item's LDS readers are done
            rc = tiff_lzw_wave(f + coff, cnt, dst, c.want, reinterpret_cast<uint32_t*>(lds), lds + 4096 * 4, lds + 4096 * 5, lane);
        } else if (comp == 32773) {
            rc = tiff_packbits_wave(f + coff, cnt, dst, c.want, lane);
        } else {
            wave_sync();
            int64_t m = 0;
            const bool ok = exr_inflate_wave<kTiffInfWin>(f + coff, cnt, dst, (int64_t)c.want, &m, *reinterpret_cast<InfState*>(lds + kTiffInfWin),
                                                          lds);
            // (more than `want` bytes fail inside the inflate, before a byte past `want` is stored)
            if (!ok || m != (int64_t)c.want) rc = kTiffBadData;
        }
        if (rc != kTiffOk && lane == 0) atomicMin(&dd.fail, (uint32_t)k << 8 | (uint32_t)rc);
    }
}

// ---------------------------------------------------------------------------- render
__device__ __forceinline__ uint32_t tiff_padd(uint32_t a, uint32_t b) {  // four byte sums mod 256
    return (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu) | (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u);
}

// grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_tiff_render(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                     const TiffDesc* __restrict__ desc, const uint8_t* __restrict__ scratch,
                                                     uint64_t slot, uint8_t* __restrict__ out, uint64_t out_stride) {
    __shared__ uint32_t pal[256];
    __shared__ uint32_t sc[256];
    __shared__ __attribute__((aligned(16))) uint8_t seg[kTiffSeg * 4 + 16];
    const int i = blockIdx.y, tid = threadIdx.x;
    const TiffDesc& dd = desc[i];
    if (dd.status != kTiffOk || dd.fail != kTiffNoFail) return;
    const TiffHead H = dd.H;
    const uint8_t* f = data + off[i];
    const uint8_t* scr = scratch + (uint64_t)i * slot;
    uint8_t* dst = out + (uint64_t)i * out_stride;
    const int spp = H.spp, d = H.d;
    if (H.photo == 3) {  // (the ColorMap lies inside the file: tiff_parse)
        const uint8_t* cm = f + H.cmap_at;
        pal[tid] = (tiff_u16(cm + 2 * tid, H.be) >> 8) | (tiff_u16(cm + 2 * (256 + tid), H.be) >> 8) << 8 |
                   (tiff_u16(cm + 2 * (512 + tid), H.be) >> 8) << 16;
    }
    const uint32_t room = tiff_chunk_room(H);
    for (int y = blockIdx.x; y < H.h; y += gridDim.x) {
        const int cy = y / H.ch;
        for (int cx = 0; cx < H.across; ++cx) {
            const int k = cy * H.across + cx;
            const TiffChunk c = tiff_chunk(H, k);
            const uint8_t* row = (H.comp == 1 ? f + tiff_elem(f, H.off_at, H.off_type, H.be, k) : scr + (uint64_t)k * room) +
                                 (uint64_t)(y - c.y0) * c.row_bytes;
            uint32_t carry = 0;
            for (int xs = 0; xs < c.cols; xs += kTiffSeg) {
                const int nx = min(kTiffSeg, c.cols - xs);
                uint32_t px[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p = 4 * tid + q;
                    uint32_t v = 0;
                    if (p < nx) {
                        const uint8_t* s = row + (int64_t)(xs + p) * spp;
                        v = s[0];
                        if (spp >= 3) v |= (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
                        if (spp == 4) v |= (uint32_t)s[3] << 24;
                    }
                    px[q] = v;
                }
                __syncthreads();  // the previous segment's readers are done (and pal is in)
                if (H.pred == 2) {
                    px[1] = tiff_padd(px[1], px[0]);
                    px[2] = tiff_padd(px[2], px[1]);
                    px[3] = tiff_padd(px[3], px[2]);
                    sc[tid] = px[3];
                    __syncthreads();
                    for (int s = 1; s < 256; s <<= 1) {
                        const uint32_t t = tid >= s ? sc[tid - s] : 0;
                        __syncthreads();
                        sc[tid] = tiff_padd(sc[tid], t);
                        __syncthreads();
                    }
                    const uint32_t add = tiff_padd(carry, tid ? sc[tid - 1] : 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) px[q] = tiff_padd(px[q], add);
                    carry = tiff_padd(carry, sc[255]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p = 4 * tid + q;
                    if (p >= nx) break;
                    uint32_t v = px[q];
                    if (H.photo == 0) v = 255u - (v & 255u);
                    else if (H.photo == 3) v = pal[v & 255u];
                    seg[d * p] = (uint8_t)v;
                    if (d >= 3) { seg[d * p + 1] = (uint8_t)(v >> 8); seg[d * p + 2] = (uint8_t)(v >> 16); }
                    if (d == 4) seg[d * p + 3] = (uint8_t)(v >> 24);
                }
                __syncthreads();
                store_segment(dst + ((int64_t)y * H.w + c.x0 + xs) * d, nx * d, tid, [&](int q) -> uint32_t { return seg[q]; });
            }
        }
    }
}

__global__ void k_tiff_finish(int n, const TiffDesc* __restrict__ desc, int32_t* __restrict__ status,
                              int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TiffDesc& dd = desc[i];
    const int code = dd.status != kTiffOk ? dd.status : dd.fail != kTiffNoFail ? (int)(dd.fail & 255u) : kTiffOk;
    const bool ok = code == kTiffOk;
    status[i] = code;
    dims[3 * i + 0] = ok ? dd.H.w : 0;
    dims[3 * i + 1] = ok ? dd.H.h : 0;
    dims[3 * i + 2] = ok ? dd.H.d : 0;
}

// ------------------------------------------------------------------------------- host
int tiff_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* pw, int* ph) {
    TiffHead H{};
    const int rc = tiff_parse(data, size, &H);
    if (rc == kTiffOk) {
        *w = H.w;
        *h = H.h;
        *d = H.d;
        *pw = H.across * H.cw;  // (the padded size: at most 2^30 pixels)
        *ph = H.down * H.ch;
    }
    return rc;
}

bool tiff_ws_alloc(TiffWs& ws, Blocks& mem, int device, int max_images, int max_w, int max_h) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.slot = (int64_t)tiff_scratch_slot(max_w, max_h);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return false;
    ws.unpack_grid = cus * 8;
    const size_t n = (size_t)max_images;
    return mem.alloc(ws.desc, n * sizeof(TiffDesc)) && mem.alloc(ws.count, n * sizeof(int32_t)) &&
           mem.alloc(ws.first, (n + 1) * sizeof(int32_t)) && mem.alloc(ws.next, sizeof(uint32_t)) && mem.alloc(ws.scratch, n * (size_t)ws.slot);
}

void launch_tiff_decode(const TiffWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                        uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                        StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    const int nb = (n + 63) / 64;
    S.begin(kStParse);
    hipLaunchKernelGGL(k_tiff_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.count, ws.max_w, ws.max_h,
                       (uint64_t)ws.slot);
    hipLaunchKernelGGL(k_tiff_scan, dim3(1), dim3(256), 0, st, n, ws.count, ws.first, ws.next);
    S.end(kStParse);
    S.begin(kStEntropy);
    hipLaunchKernelGGL(k_tiff_unpack, dim3(ws.unpack_grid), dim3(64), 0, st, n, d_data, d_off, ws.desc, ws.first, ws.next, ws.scratch,
                       (uint64_t)ws.slot);
    S.end(kStEntropy);
    S.begin(kStConvert);
    hipLaunchKernelGGL(k_tiff_render, dim3(rows_grid(ws.max_h, n), n), dim3(256), 0, st,
                       d_data, d_off, ws.desc, ws.scratch, (uint64_t)ws.slot, d_out, out_stride);
    hipLaunchKernelGGL(k_tiff_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    S.end(kStConvert);
}

}  // namespace icx
