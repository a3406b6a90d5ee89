// icx_dds.hip -- DDS read and write on gfx950 (Image::readDds / writeDds), with the contract of
// include/icx.h and the arithmetic of icx_dds_core.h.
//
// Read. A block-compressed top level is 4 x 4 blocks that decode independently, and the masked and
// copied forms are rows of fixed-size pixels: nothing has to be located, so the read is a header
// walk and one streaming pass.
//   k_dds_parse    header walk (dds_parse), one lane per image; it also settles TOO_LARGE against
//                  the batch's maxima and the slot, and writes the status and the dims
//   k_dds_blocks   BC1 .. BC5: a workgroup takes a row of blocks in segments of 256 blocks, one
//                  block per lane. The segment's bytes go to LDS by aligned 16-byte loads whatever
//                  the file's offset; a lane decodes its block and writes its four 4-pixel pieces
//                  (12 bytes each for BC1) into four staged pixel rows in LDS; wave r then stores
//                  pixel row r, 16 bytes per lane at consecutive addresses along the image row,
//                  single bytes at the ragged ends. The body is a template on the format; one
//                  kernel switches between its instances, so a batch costs one launch, not five
//   k_dds_raw      masked and copied forms, in the manner of k_bmp_raw: row segments through LDS,
//                  out by 16-byte stores at the destination's alignment. Files whose channels are
//                  whole bytes of the stored pixel (24-bit B,G,R, 32-bit B,G,R,A and the like, and
//                  the copied forms as one-byte pixels) move bytes; other masks go through
//                  bmp_field8 per field
// Write. k_ddsw_head writes each file's 128-byte header from its device-side job; k_ddsw_rows
// streams RAW rows (B,G,R(,A), or as they are for d < 3); k_ddsw_blocks mirrors k_dds_blocks: four
// pixel rows of a segment to LDS, one block per lane encoded by dds_encode_block, the blocks staged
// in LDS and stored as one contiguous run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_dds_core.h"
#include "icx_wave.h"

namespace icx {

constexpr int kDdsSegBlocks = 256;             // blocks per segment of a block row: one per lane of the workgroup
constexpr int kDdsSeg = 4 * kDdsSegBlocks;     // pixels per row segment (tests/test_gpu_dds.py names it)
constexpr int kDdsWin = kDdsSeg * 4 + 48;      // a segment's bytes at 4 per pixel (or 256 blocks of 16), misalignment, slack

struct DdsDesc {
    DdsHead H;
    int64_t size;
    int32_t status, pad_;
};

__global__ void k_dds_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ size, DdsDesc* __restrict__ desc, int max_w, int max_h,
                            uint64_t out_stride, int32_t* __restrict__ status, int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DdsDesc dd{};
    dd.size = (int64_t)size[i];
    dd.status = dds_parse(data + off[i], dd.size, &dd.H);
    if (dd.status == kDdsOk && (dd.H.w > max_w || dd.H.h > max_h || (uint64_t)dds_out_bytes(dd.H) > out_stride))
        dd.status = kDdsTooLarge;
    desc[i] = dd;
    const bool ok = dd.status == kDdsOk;
    status[i] = dd.status;
    dims[4 * i + 0] = ok ? dd.H.w : 0;
    dims[4 * i + 1] = ok ? dd.H.h : 0;
    dims[4 * i + 2] = ok ? dd.H.d : 0;
    dims[4 * i + 3] = ok ? dd.H.type : 0;
}

// The 4 bytes at byte `at` of the 4-byte aligned LDS array `base` (8 bytes from at & ~3 are read).
__device__ __forceinline__ uint32_t lds_u32(const uint8_t* base, int at) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(base + (at & ~3));
    return (uint32_t)((q[0] | (uint64_t)q[1] << 32) >> (8 * (at & 3)));
}

// optr[0, nb) = src[0, nb) by lanes tid of nthreads: src is a 4-byte aligned LDS array with 20
// readable bytes past nb. Single bytes up to optr's 16-byte boundary, 16-byte stores, single
// bytes after.
__device__ __forceinline__ void store_from_lds(uint8_t* optr, const uint8_t* src, int nb, int tid, int nthreads) {
    const int head = min(nb, (int)((16 - (reinterpret_cast<uintptr_t>(optr) & 15)) & 15));
    const int nv = (nb - head) / 16;
    for (int v = tid; v < nv; v += nthreads) {
        const int a = head + 16 * v;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src + (a & ~3));
        const int sh = 8 * (a & 3);
        const uint32_t t0 = q[0], t1 = q[1], t2 = q[2], t3 = q[3], t4 = q[4];
        const uint4 o = make_uint4((uint32_t)((t0 | (uint64_t)t1 << 32) >> sh), (uint32_t)((t1 | (uint64_t)t2 << 32) >> sh),
                                   (uint32_t)((t2 | (uint64_t)t3 << 32) >> sh), (uint32_t)((t3 | (uint64_t)t4 << 32) >> sh));
        *reinterpret_cast<uint4*>(optr + a) = o;
    }
    const int tail0 = head + 16 * nv;
    for (int b = tid; b < head + (nb - tail0); b += nthreads) {
        const int q = b < head ? b : tail0 + (b - head);
        optr[q] = src[q];
    }
}

template <int KIND>
__device__ __forceinline__ void dds_block_rows(const DdsHead& H, const uint8_t* file, int64_t fsize, uint8_t* dst, uint8_t* win,
                                               uint8_t* stage) {
    constexpr int BS = KIND == kDdsBc1 || KIND == kDdsBc4 ? 8 : 16;
    constexpr int D = KIND == kDdsBc1 ? 3 : KIND == kDdsBc4 ? 1 : KIND == kDdsBc5 ? 2 : 4;
    constexpr int RS = kDdsSeg * D + 32;  // bytes of a staged pixel row (a multiple of 16)
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int bw = (H.w + 3) / 4, bh = (H.h + 3) / 4;
    for (int by = blockIdx.x; by < bh; by += gridDim.x) {
        for (int bx0 = 0; bx0 < bw; bx0 += kDdsSegBlocks) {
            const int nblk = min(kDdsSegBlocks, bw - bx0);
            const int64_t s0 = H.ds + ((int64_t)by * bw + bx0) * BS;
            const int mis = (int)(reinterpret_cast<uintptr_t>(file + s0) & 15);
            __syncthreads();  // the previous segment's readers are done
            fill_window(win, file, fsize, s0 - mis, (mis + nblk * BS + 8 + 15) & ~15, tid, 256);
            __syncthreads();
            if (tid < nblk) {
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < BS / 4; ++k) w[k] = lds_u32(win, mis + tid * BS + 4 * k);
                DdsBlockPal P{};
                dds_block_setup(KIND, w, &P);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t p[4];
#pragma unroll
                    for (int x = 0; x < 4; ++x) p[x] = dds_block_pixel(KIND, w, P, 4 * r + x);
                    uint8_t* o = stage + r * RS + tid * 4 * D;
                    if (D == 4) {
                        *reinterpret_cast<uint4*>(o) = make_uint4(p[0], p[1], p[2], p[3]);
                    } else if (D == 3) {
                        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
                        o4[0] = p[0] | p[1] << 24;
                        o4[1] = p[1] >> 8 | p[2] << 16;
                        o4[2] = p[2] >> 16 | p[3] << 8;
                    } else if (D == 2) {
                        *reinterpret_cast<uint2*>(o) = make_uint2(p[0] | p[1] << 16, p[2] | p[3] << 16);
                    } else {
                        *reinterpret_cast<uint32_t*>(o) = p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24;
                    }
                }
            }
            __syncthreads();
            const int y = 4 * by + wv, x0 = 4 * bx0;  // wave wv stores pixel row wv of the block row
            if (y < H.h) store_from_lds(dst + ((int64_t)y * H.w + x0) * D, stage + wv * RS, min(4 * nblk, H.w - x0) * D, lane, 64);
        }
    }
}

// grid (x: block rows, y: image)
__global__ __launch_bounds__(256) void k_dds_blocks(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                    const DdsDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                    uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kDdsWin];
    __shared__ __attribute__((aligned(16))) uint8_t stage[4 * (kDdsSeg * 4 + 32)];
    const int i = blockIdx.y;
    const DdsDesc& dd = desc[i];
    if (dd.status != kDdsOk || dd.H.kind > kDdsBc5) return;
    const DdsHead H = dd.H;
    const uint8_t* file = data + off[i];
    uint8_t* dst = out + (uint64_t)i * out_stride;
    switch (H.kind) {
    case kDdsBc1: dds_block_rows<kDdsBc1>(H, file, dd.size, dst, win, stage); break;
    case kDdsBc2: dds_block_rows<kDdsBc2>(H, file, dd.size, dst, win, stage); break;
    case kDdsBc3: dds_block_rows<kDdsBc3>(H, file, dd.size, dst, win, stage); break;
    case kDdsBc4: dds_block_rows<kDdsBc4>(H, file, dd.size, dst, win, stage); break;
    case kDdsBc5: dds_block_rows<kDdsBc5>(H, file, dd.size, dst, win, stage); break;
    }
}

// Rows of `roww` stored pixels of bpp bytes -> D output bytes each. BYTEWISE: output channel c is
// byte (at >> 8c) & 255 of the stored pixel; otherwise the fields of H.mask.
template <int D, bool BYTEWISE>
__device__ __forceinline__ void dds_raw_rows(const DdsHead& H, int bpp, uint32_t at, int64_t roww, const uint8_t* file,
                                             int64_t fsize, uint8_t* dst, uint8_t* win) {
    const int tid = threadIdx.x;
    auto pixel = [&](const uint8_t* seg, int x) -> uint32_t {
        uint32_t v = 0;
        for (int b = 0; b < bpp; ++b) v |= (uint32_t)seg[x * bpp + b] << (8 * b);
        return dds_masked_pixel(H, v);
    };
    for (int y = blockIdx.x; y < H.h; y += gridDim.x) {
        for (int64_t x0 = 0; x0 < roww; x0 += kDdsSeg) {
            const int nx = (int)min<int64_t>(kDdsSeg, roww - x0);
            const int64_t s0 = H.ds + ((int64_t)y * roww + x0) * bpp;
            const int mis = (int)(reinterpret_cast<uintptr_t>(file + s0) & 15);
            __syncthreads();  // the previous segment's readers are done
            fill_window(win, file, fsize, s0 - mis, (mis + nx * bpp + 15) & ~15, tid, 256);
            __syncthreads();
            const uint8_t* seg = win + mis;
            uint8_t* optr = dst + ((int64_t)y * roww + x0) * D;
            const int nb = nx * D;
            const int head = min(nb, (int)((16 - (reinterpret_cast<uintptr_t>(optr) & 15)) & 15));
            const int nv = (nb - head) / 16;
            for (int v = tid; v < nv; v += 256) {
                const int b0 = head + 16 * v;
                int x = b0 / D, c = b0 - x * D;
                uint32_t wd[4] = {0, 0, 0, 0};
                if (BYTEWISE) {  // one LDS byte per output byte
#pragma unroll
                    for (int b = 0; b < 16; ++b) {
                        wd[b >> 2] |= (uint32_t)seg[x * bpp + (at >> (8 * c) & 255u)] << (8 * (b & 3));
                        if (++c == D) { c = 0; ++x; }
                    }
                } else {
                    uint32_t px = pixel(seg, x);
#pragma unroll
                    for (int b = 0; b < 16; ++b) {
                        wd[b >> 2] |= ((px >> (8 * c)) & 255u) << (8 * (b & 3));
                        if (++c == D) {
                            c = 0;
                            ++x;
                            px = x < nx ? pixel(seg, x) : 0;
                        }
                    }
                }
                *reinterpret_cast<uint4*>(optr + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
            const int tail0 = head + 16 * nv;
            for (int b = tid; b < head + (nb - tail0); b += 256) {
                const int q = b < head ? b : tail0 + (b - head);
                const int x = q / D, c = q - x * D;
                optr[q] = BYTEWISE ? seg[x * bpp + (at >> (8 * c) & 255u)] : (uint8_t)(pixel(seg, x) >> (8 * c));
            }
        }
    }
}

// grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_dds_raw(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                 const DdsDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                 uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kDdsWin];
    const int i = blockIdx.y;
    const DdsDesc& dd = desc[i];
    if (dd.status != kDdsOk || dd.H.kind <= kDdsBc5) return;
    const DdsHead H = dd.H;
    const uint8_t* file = data + off[i];
    uint8_t* dst = out + (uint64_t)i * out_stride;
    if (H.kind == kDdsCopy) {  // the samples as they are: pixels of one byte
        dds_raw_rows<1, true>(H, 1, 0, (int64_t)H.w * H.bpp, file, dd.size, dst, win);
        return;
    }
    switch (H.d * 2 + H.bytewise) {
    case 2: dds_raw_rows<1, false>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 3: dds_raw_rows<1, true>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 4: dds_raw_rows<2, false>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 5: dds_raw_rows<2, true>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 6: dds_raw_rows<3, false>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 7: dds_raw_rows<3, true>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 8: dds_raw_rows<4, false>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    case 9: dds_raw_rows<4, true>(H, H.bpp, H.at, H.w, file, dd.size, dst, win); break;
    }
}

// ------------------------------------------------------------------------------- write
struct DdsJob {
    const uint8_t* src;
    int32_t w, h;
    int32_t status, pad_;
};

// One wave per image: the file's size and status, and its header built in LDS and copied out.
__global__ __launch_bounds__(64) void k_ddsw_head(DdsJob* __restrict__ jobs, int d, int format, uint8_t* __restrict__ out,
                                                  uint64_t out_stride, uint64_t* __restrict__ sizes,
                                                  int32_t* __restrict__ status) {
    __shared__ uint8_t s_head[128];
    const int i = blockIdx.x, lane = threadIdx.x;
    DdsJob& J = jobs[i];
    if (J.status != kDdsOk) {
        if (lane == 0) { sizes[i] = 0; status[i] = J.status; }
        return;
    }
    const uint64_t total = dds_encode_bound(J.w, J.h, d, format);
    const bool fits = total <= out_stride;
    if (fits && lane == 0) dds_write_header(s_head, J.w, J.h, d, format);
    __syncthreads();
    if (fits) {
        uint8_t* o = out + (uint64_t)i * out_stride;
        for (int b = lane; b < 128; b += 64) o[b] = s_head[b];
    }
    __syncthreads();  // every lane has read J.status before lane 0 may change it
    if (lane == 0) {
        sizes[i] = total;
        status[i] = fits ? kDdsOk : kDdsTooLarge;
        if (!fits) J.status = kDdsTooLarge;  // the row and block kernels skip it
    }
}

template <int D>
__device__ __forceinline__ void ddsw_raw_rows(const DdsJob& J, uint8_t* dst, uint8_t* win) {
    const int w = J.w, h = J.h, tid = threadIdx.x;
    const int64_t src_size = (int64_t)w * h * D;
    for (int r = blockIdx.x; r < h; r += gridDim.x) {
        for (int x0 = 0; x0 < w; x0 += kDdsSeg) {
            const int nx = min(kDdsSeg, w - x0);
            const int64_t s0 = ((int64_t)r * w + x0) * D;
            const int mis = (int)(reinterpret_cast<uintptr_t>(J.src + s0) & 15);
            __syncthreads();  // the previous segment's readers are done
            fill_window(win, J.src, src_size, s0 - mis, (mis + nx * D + 15) & ~15, tid, 256);
            __syncthreads();
            const uint8_t* seg = win + mis;
            store_segment(dst + s0, nx * D, tid, [&](int q) -> uint32_t { return seg[dds_raw_source(q, D)]; });
        }
    }
}

// grid (x: rows, y: image): RAW files, rows top-down and unpadded.
__global__ __launch_bounds__(256) void k_ddsw_rows(const DdsJob* __restrict__ jobs, int d, uint8_t* __restrict__ out,
                                                   uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kDdsWin];
    const DdsJob& J = jobs[blockIdx.y];
    if (J.status != kDdsOk) return;
    uint8_t* dst = out + (uint64_t)blockIdx.y * out_stride + 128;
    switch (d) {
    case 1: ddsw_raw_rows<1>(J, dst, win); break;
    case 2: ddsw_raw_rows<2>(J, dst, win); break;
    case 3: ddsw_raw_rows<3>(J, dst, win); break;
    case 4: ddsw_raw_rows<4>(J, dst, win); break;
    }
}

template <int D>
__device__ __forceinline__ void ddsw_block_rows(const DdsJob& J, uint8_t* dst, uint8_t (*win)[kDdsWin], uint8_t* stage) {
    constexpr int BS = D == 1 || D == 3 ? 8 : 16;
    constexpr uint32_t kMask = D == 4 ? 0xFFFFFFFFu : (1u << (8 * (D & 3))) - 1;
    const int w = J.w, h = J.h, tid = threadIdx.x;
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    const int64_t src_size = (int64_t)w * h * D;
    for (int by = blockIdx.x; by < bh; by += gridDim.x) {
        for (int bx0 = 0; bx0 < bw; bx0 += kDdsSegBlocks) {
            const int nblk = min(kDdsSegBlocks, bw - bx0), x0 = 4 * bx0, nx = min(kDdsSeg, w - x0);
            int mis[4];
            __syncthreads();  // the previous segment's readers are done
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // rows past the image's last repeat it
                const int64_t s0 = ((int64_t)min(4 * by + r, h - 1) * w + x0) * D;
                mis[r] = (int)(reinterpret_cast<uintptr_t>(J.src + s0) & 15);
                fill_window(win[r], J.src, src_size, s0 - mis[r], (mis[r] + nx * D + 8 + 15) & ~15, tid, 256);
            }
            __syncthreads();
            if (tid < nblk) {
                uint32_t px[16], wd[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 16; ++k) {  // columns past the image's last repeat it
                    const int x = min(4 * tid + (k & 3), nx - 1);
                    px[k] = lds_u32(win[k >> 2], mis[k >> 2] + x * D) & kMask;
                }
                dds_encode_block(D, px, wd);
                uint32_t* o = reinterpret_cast<uint32_t*>(stage + tid * BS);
#pragma unroll
                for (int k = 0; k < BS / 4; ++k) o[k] = wd[k];
            }
            __syncthreads();
            store_from_lds(dst + ((int64_t)by * bw + bx0) * BS, stage, nblk * BS, tid, 256);
        }
    }
}

// grid (x: block rows, y: image): BC files.
__global__ __launch_bounds__(256) void k_ddsw_blocks(const DdsJob* __restrict__ jobs, int d, uint8_t* __restrict__ out,
                                                     uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[4][kDdsWin];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kDdsSegBlocks * 16 + 32];
    const DdsJob& J = jobs[blockIdx.y];
    if (J.status != kDdsOk) return;
    uint8_t* dst = out + (uint64_t)blockIdx.y * out_stride + 128;
    switch (d) {
    case 1: ddsw_block_rows<1>(J, dst, win, stage); break;
    case 2: ddsw_block_rows<2>(J, dst, win, stage); break;
    case 3: ddsw_block_rows<3>(J, dst, win, stage); break;
    case 4: ddsw_block_rows<4>(J, dst, win, stage); break;
    }
}

// ------------------------------------------------------------------------------- host
int dds_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* type) {
    DdsHead H{};
    const int rc = dds_parse(data, size, &H);
    if (rc == kDdsOk) {
        *w = H.w;
        *h = H.h;
        *d = H.d;
        *type = H.type;
    }
    return rc;
}

bool dds_ws_alloc(DdsWs& ws, Blocks& mem, int max_images, int max_w, int max_h) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    return mem.alloc(ws.desc, (size_t)max_images * sizeof(DdsDesc));
}

void launch_dds_decode(const DdsWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    S.begin(kStParse);
    hipLaunchKernelGGL(k_dds_parse, dim3((n + 63) / 64), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.max_w, ws.max_h,
                       out_stride, d_status, d_dims);
    S.end(kStParse);
    S.begin(kStEntropy);  // block formats
    hipLaunchKernelGGL(k_dds_blocks, dim3(rows_grid((ws.max_h + 3) / 4, n), n), dim3(256), 0, st, d_data, d_off, ws.desc, d_out,
                       out_stride);
    S.end(kStEntropy);
    S.begin(kStConvert);  // masked and copied forms
    hipLaunchKernelGGL(k_dds_raw, dim3(rows_grid(ws.max_h, n), n), dim3(256), 0, st, d_data, d_off, ws.desc, d_out, out_stride);
    S.end(kStConvert);
}

struct DdswWs {
    Buf<DdsJob> jobs;
};
DdswWs* ddsw_ws_create() { return new DdswWs(); }
void ddsw_ws_destroy(DdswWs* w) { delete w; }

int dds_encode_batch(hipStream_t st, DdswWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int format, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err) {
    std::vector<DdsJob> jobs((size_t)n);
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        DdsJob& J = jobs[i];
        J = DdsJob{};
        J.src = d_src[i];
        J.w = widths[i];
        J.h = heights[i];
        J.status = J.src && dds_write_args_ok(J.w, J.h, d, format) ? kDdsOk : kDdsInvalidArgument;
        if (J.status == kDdsOk) max_h = std::max(max_h, J.h);
    }
    if (jobs_upload("dds_encode_batch", ws.jobs, jobs, st, err)) return -1;
    hipLaunchKernelGGL(k_ddsw_head, dim3(n), dim3(64), 0, st, ws.jobs.p, d, format, d_out, out_stride, d_sizes, d_status);
    if (format == kDdsRaw)
        hipLaunchKernelGGL(k_ddsw_rows, dim3(rows_grid(max_h, n), n), dim3(256), 0, st, ws.jobs.p, d, d_out, out_stride);
    else
        hipLaunchKernelGGL(k_ddsw_blocks, dim3(rows_grid((max_h + 3) / 4, n), n), dim3(256), 0, st, ws.jobs.p, d, d_out, out_stride);
    return encode_finish("dds_encode_batch", st, err);
}

}  // namespace icx
