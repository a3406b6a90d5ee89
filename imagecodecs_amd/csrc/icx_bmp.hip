// icx_bmp.hip -- BMP read and write on gfx950: Image::readBmp (codecs.cpp:255-320) and
// Image::writeBmp (:324-375), with the contract and deviations of include/icx.h.
//
// Read. Raw files (1, 4, 8, 16, 24, 32 bits) are one streaming kernel. A run-length stream (RLE8,
// RLE4) moves a two-dimensional cursor: where a packet starts and where its pixels land depend on
// every packet before it. It is cut into tiles of kBmpTile bytes and located without a serial
// walk over the packets:
//   k_bmp_parse    header walk (bmp_parse), one lane per image
//   k_bmp_tiles    one workgroup per tile: every even offset taken as a would-be packet gets its
//                  successor and its cursor transform (reset, dx, dy); pointer doubling in LDS then
//                  tells, for a chain entering the tile at any offset, where it leaves the tile (or
//                  that it ends, or meets a packet the file cuts short) and what it does to the cursor
//   k_bmp_chain    one workgroup per image: tile t+1's entry offset and entry cursor from tile t's
//                  summary (rows of summaries staged through LDS, 16 tiles per global round trip);
//                  finds the tile in which the walk ends, or that it is TRUNCATED
//   k_bmp_fill     palette entry 0 (or its grey value) over the whole image, 16-byte stores
//   k_bmp_expand   one wave per tile: the packets are walked from an LDS window, 256 visible packets
//                  at a time, into a table of packet starts, cursors and visible pixel counts; the
//                  lanes then take one pixel each (its packet by binary search), so neighbouring
//                  lanes store neighbouring pixels. The cursor only moves forward in (y, x) and
//                  clipped pixels are dropped, so no output byte is written by two packets
//   k_bmp_raw24 /
//   k_bmp_raw      rows of raw files (24 bits in a kernel of its own, the other depths share one): source row segment -> LDS by aligned 16-byte loads, expanded
//                  through the palette or the mask tables staged in LDS, out by 16-byte stores at the
//                  absolute address's alignment (bytes at the ragged ends), row flip on the way out
// No stream is declined: every packet chain goes through the tiles, so there is no serial walk.
//
// Write. k_bmpw_head writes each file's header (and grey palette) from its device-side job;
// k_bmpw_rows streams the rows bottom-up, B,G,R(,A) or grey, with their zero pad bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_bmp_core.h"
#include "icx_wave.h"

namespace icx {

constexpr int kBmpTile = 4096;            // stream bytes per tile (tests/test_gpu_bmp.py names it)
constexpr int kBmpSlots = kBmpTile / 2;   // would-be packets per tile: every even offset
constexpr int kBmpMaxPkt = 258;           // longest packet: 2 + 255 literal bytes + pad
constexpr int kBmpEntries = 132;          // entry slots 0 .. 128 of a tile, padded to a multiple of 4
constexpr int kBmpWin = kBmpTile + 288;   // expand window: a tile, its last packet's overhang, 16 for alignment
constexpr uint32_t kBmpEndCode = 0xFFFE, kBmpCutCode = 0xFFFF;
constexpr int kBmpChunk = 256;            // visible packets k_bmp_expand locates before it writes their pixels
constexpr int kBmpChainRows = 16;         // summary rows staged per round of k_bmp_chain
constexpr int kBmpSeg = 1024;             // pixels per row segment of the streaming kernels (a multiple of 8)

struct BmpDesc {
    BmpHead H;
    int64_t size;
    int32_t status;
    int32_t ntiles;    // RLE: tiles the chain may visit
    int32_t last;      // the tile in which the walk ends (k_bmp_chain)
    int32_t short_ws;  // the stream is longer than the workspace's tiles cover
};

__global__ void k_bmp_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ size, BmpDesc* __restrict__ desc, int max_w, int max_h,
                            int64_t tiles_cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    BmpDesc dd{};
    dd.size = (int64_t)size[i];
    dd.last = -1;
    dd.status = bmp_parse(data + off[i], dd.size, &dd.H);
    if (dd.status == kBmpOk) {
        if (dd.H.w > max_w || dd.H.h > max_h || (dd.H.rle && tiles_cap == 0)) {  // (0: a workspace for raw files)
            dd.status = kBmpTooLarge;
        } else if (dd.H.rle) {
            dd.status = kBmpPending;
            // (+ 1: a chain that leaves the stream's last tile enters one that holds its end)
            const int64_t need = (dd.size - dd.H.ds) / kBmpTile + 1;
            dd.ntiles = (int32_t)min(need, tiles_cap);
            dd.short_ws = need > tiles_cap;
        }
    }
    desc[i] = dd;
}

// A cursor transform in two words: reset << 31 | dx, dy (both at most kBmpFar).
__device__ __forceinline__ void bmp_move_join(uint32_t& rdx, uint32_t& dy, uint32_t b_rdx, uint32_t b_dy) {  // this, then b
    const BmpMove m = bmp_compose(BmpMove{(int32_t)(rdx >> 31), (int32_t)(rdx & 0x7FFFFFFFu), (int32_t)dy},
                                  BmpMove{(int32_t)(b_rdx >> 31), (int32_t)(b_rdx & 0x7FFFFFFFu), (int32_t)b_dy});
    rdx = (uint32_t)m.reset << 31 | (uint32_t)m.dx;
    dy = (uint32_t)m.dy;
}

// grid (x: tile, y: image)
__global__ __launch_bounds__(256) void k_bmp_tiles(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                   const BmpDesc* __restrict__ desc, uint4* __restrict__ summary,
                                                   int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kBmpTile + 32];
    __shared__ uint16_t s_nxt[kBmpSlots];
    __shared__ uint32_t s_rdx[kBmpSlots];
    __shared__ uint32_t s_dy[kBmpSlots];
    const int i = blockIdx.y, t = blockIdx.x;
    const BmpDesc& dd = desc[i];
    if (dd.status != kBmpPending || t >= dd.ntiles) return;
    const uint8_t* d = data + off[i];
    const int64_t n = dd.size, tile0 = dd.H.ds + (int64_t)t * kBmpTile;
    const int rle = dd.H.rle;
    const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
    fill_window(win, d, n, tile0 - mis, kBmpTile + 32, threadIdx.x, 256);
    __syncthreads();
    constexpr int kPer = kBmpSlots / 256;
    uint16_t nn[kPer];
    uint32_t rx[kPer], ry[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = threadIdx.x + 256 * q;
        const BmpPacket k = bmp_packet(win + mis + 2 * j, n - (tile0 + 2 * j), rle);
        // >= kBmpSlots: leaves the tile at slot nn - kBmpSlots of the next one
        nn[q] = k.kind == kBmpPkEnd ? kBmpEndCode : k.kind == kBmpPkCut ? kBmpCutCode : (uint16_t)(j + k.len / 2);
        rx[q] = (uint32_t)k.move.reset << 31 | (uint32_t)k.move.dx;
        ry[q] = (uint32_t)k.move.dy;
        s_nxt[j] = nn[q];
        s_rdx[j] = rx[q];
        s_dy[j] = ry[q];
    }
    __syncthreads();
    // a chain inside a tile has at most kBmpSlots packets: 11 doublings reach its end; long
    // packets need fewer, and the rounds stop once every chain has left the tile
    for (int round = 0; round < 12; ++round) {
        bool active = false;
#pragma unroll
        for (int q = 0; q < kPer; ++q) active |= nn[q] < kBmpSlots;
        if (!__syncthreads_or(active)) break;
#pragma unroll
        for (int q = 0; q < kPer; ++q)
            if (nn[q] < kBmpSlots) {
                const int a = nn[q];
                bmp_move_join(rx[q], ry[q], s_rdx[a], s_dy[a]);
                nn[q] = s_nxt[a];
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int j = threadIdx.x + 256 * q;
            s_nxt[j] = nn[q];
            s_rdx[j] = rx[q];
            s_dy[j] = ry[q];
        }
    }
    __syncthreads();
    uint4* S = summary + ((int64_t)i * tiles_cap + t) * kBmpEntries;
    for (int e = threadIdx.x; e < kBmpEntries; e += 256) {
        uint4 v = make_uint4(kBmpCutCode, 0, 0, 0);
        if (e <= kBmpMaxPkt / 2) {
            const uint32_t nx = s_nxt[e];
            // (nx < kBmpSlots cannot be left after the doublings; it would read as a failed chain)
            v = make_uint4(nx >= kBmpEndCode ? nx : nx < kBmpSlots ? kBmpCutCode : nx - kBmpSlots, s_rdx[e], s_dy[e], 0);
        }
        S[e] = v;
    }
}

// One workgroup per image.
__global__ __launch_bounds__(256) void k_bmp_chain(BmpDesc* __restrict__ desc, const uint4* __restrict__ summary,
                                                   int32_t* __restrict__ entry, int32_t* __restrict__ cur_x,
                                                   int32_t* __restrict__ cur_y, int64_t tiles_cap) {
    __shared__ uint4 rows[kBmpChainRows * kBmpEntries];
    __shared__ int s_done;
    const int i = blockIdx.x;
    BmpDesc& dd = desc[i];
    if (dd.status != kBmpPending) return;
    const int ntiles = dd.ntiles;
    const uint4* S = summary + (int64_t)i * tiles_cap * kBmpEntries;
    int32_t* E = entry + (int64_t)i * tiles_cap;
    int32_t* X = cur_x + (int64_t)i * tiles_cap;
    int32_t* Y = cur_y + (int64_t)i * tiles_cap;
    int e = 0;  // thread 0's state
    int32_t x = 0, y = 0;
    if (threadIdx.x == 0) s_done = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += kBmpChainRows) {
        const int nr = min(kBmpChainRows, ntiles - t0);
        for (int k = threadIdx.x; k < nr * kBmpEntries; k += 256) rows[k] = S[(int64_t)t0 * kBmpEntries + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int r = 0; r < nr; ++r) {
                const int t = t0 + r;
                E[t] = e;
                X[t] = x;
                Y[t] = y;
                const uint4 s = rows[r * kBmpEntries + e];
                if (s.x == kBmpCutCode) {  // a packet the file cuts short
                    dd.status = kBmpTruncated;
                    s_done = 1;
                    break;
                }
                if (s.x == kBmpEndCode) {  // end-of-bitmap, or fewer than 2 bytes remain
                    dd.last = t;
                    dd.status = kBmpOk;
                    s_done = 1;
                    break;
                }
                bmp_apply(BmpMove{(int32_t)(s.y >> 31), (int32_t)(s.y & 0x7FFFFFFFu), (int32_t)s.z}, &x, &y);
                e = (int)s.x;
            }
        }
        __syncthreads();
        if (s_done) return;
    }
    // (with every tile of the stream visited the walk has ended: only a short workspace gets here)
    if (threadIdx.x == 0) dd.status = dd.short_ws ? kBmpTooLarge : -1;
}

// grid (x: chunks, y: image): the d bytes of `bg` over the whole image.
__global__ __launch_bounds__(256) void k_bmp_fill(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                  const BmpDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                  uint64_t out_stride) {
    const int i = blockIdx.y;
    const BmpDesc& dd = desc[i];
    if (dd.status != kBmpOk || !dd.H.rle) return;
    const int d = dd.H.d;
    const uint32_t bg = bmp_pal_rgb(dd.H, data + off[i], 0);
    uint8_t* o = out + (int64_t)i * out_stride;
    const int64_t nb = (int64_t)dd.H.w * dd.H.h * d;
    const int64_t head = min<int64_t>(nb, (16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15);
    const int64_t nv = (nb - head) / 16;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t v = g; v < nv; v += step) {
        const int64_t b0 = head + 16 * v;
        int c = (int)(b0 % d);
        uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            wd[b >> 2] |= ((bg >> (8 * c)) & 255u) << (8 * (b & 3));
            if (++c == d) c = 0;
        }
        *reinterpret_cast<uint4*>(o + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    const int64_t tail0 = head + 16 * nv;
    for (int64_t b = g; b < head + (nb - tail0); b += step) {
        const int64_t q = b < head ? b : tail0 + (b - head);
        o[q] = (uint8_t)(bg >> (8 * (int)(q % d)));
    }
}

// grid (x: groups of 4 tiles, y: image); one wave per tile.
__global__ __launch_bounds__(256) void k_bmp_expand(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                    const BmpDesc* __restrict__ desc, const int32_t* __restrict__ entry,
                                                    const int32_t* __restrict__ cur_x, const int32_t* __restrict__ cur_y,
                                                    uint8_t* __restrict__ out, uint64_t out_stride, int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win_all[4][kBmpWin];
    __shared__ uint32_t s_pal[256];
    __shared__ uint16_t pk_pos_all[4][kBmpChunk];  // bit 15: a literal packet
    __shared__ uint32_t pk_end_all[4][kBmpChunk];
    __shared__ int32_t pk_x_all[4][kBmpChunk];
    __shared__ int32_t pk_row_all[4][kBmpChunk];
    const int i = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const BmpDesc& dd = desc[i];
    if (dd.status != kBmpOk || !dd.H.rle || (int)(blockIdx.x * 4) > dd.last) return;
    const BmpHead H = dd.H;
    const uint8_t* d = data + off[i];
    s_pal[threadIdx.x] = bmp_pal_rgb(H, d, threadIdx.x);
    __syncthreads();
    // (readfirstlane: what is the same in every lane of the wave is kept in scalar registers, so
    // the packet walk below issues scalar instructions)
    const int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    if (t > dd.last) return;
    uint8_t* o = out + (int64_t)i * out_stride;
    const int64_t n = dd.size, tile0 = H.ds + (int64_t)t * kBmpTile;
    uint8_t* win = win_all[wv];
    const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
    fill_window(win, d, n, tile0 - mis, kBmpWin, lane, 64);
    wave_sync();
    uint16_t* pk_pos = pk_pos_all[wv];
    uint32_t* pk_end = pk_end_all[wv];
    int32_t* pk_x = pk_x_all[wv];
    int32_t* pk_row = pk_row_all[wv];
    int pos = 2 * __builtin_amdgcn_readfirstlane(entry[(int64_t)i * tiles_cap + t]);
    int32_t x = __builtin_amdgcn_readfirstlane(cur_x[(int64_t)i * tiles_cap + t]);
    int32_t y = __builtin_amdgcn_readfirstlane(cur_y[(int64_t)i * tiles_cap + t]);
    const int64_t left0 = n - tile0;  // file bytes from the tile's start
    const int d_out = H.d, w = H.w, h = H.h, rle = H.rle;
    bool stop = false;
    while (!stop && pos < kBmpTile) {
        // the next kBmpChunk packets with visible pixels: every lane walks the same packets, lane 0
        // notes where each starts, its cursor and how many of the chunk's pixels end with it
        int np = 0;
        uint32_t cum = 0;
        while (np < kBmpChunk && pos < kBmpTile) {
            const uint8_t* p = win + mis + pos;
            const uint32_t lo = __builtin_amdgcn_readfirstlane(p[0] | p[1] << 8);
            const uint32_t hi = __builtin_amdgcn_readfirstlane(p[2] | p[3] << 8);
            const uint8_t four[4] = {(uint8_t)lo, (uint8_t)(lo >> 8), (uint8_t)hi, (uint8_t)(hi >> 8)};
            const BmpPacket k = bmp_packet(four, left0 - pos, rle);
            if (k.kind == kBmpPkEnd || k.kind == kBmpPkCut) { stop = true; break; }  // (Cut: k_bmp_chain never sends a tile here)
            const int vis = k.count > 0 && y < h && x < w ? min(k.count, w - x) : 0;
            if (vis > 0) {
                cum += vis;
                if (lane == 0) {
                    pk_pos[np] = (uint16_t)(pos | (k.kind == kBmpPkLiteral ? 0x8000 : 0));
                    pk_end[np] = cum;
                    pk_x[np] = x;
                    pk_row[np] = h - 1 - y;
                }
                ++np;
            }
            bmp_apply(k.move, &x, &y);
            pos += k.len;
        }
        wave_sync();
        // their pixels, one per lane: the packet of pixel q is the first whose end is past q
        for (uint32_t q = lane; q < cum; q += 64) {
            int lo = 0, hi = np - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pk_end[mid] > q) hi = mid;
                else lo = mid + 1;
            }
            const uint32_t first = lo ? pk_end[lo - 1] : 0;
            const int k = (int)(q - first);
            const uint32_t pp = pk_pos[lo];
            const uint32_t idx = bmp_packet_index(win + mis + (pp & 0x7FFF), (pp & 0x8000) ? kBmpPkLiteral : kBmpPkRun, rle, k);
            bmp_put(o + ((int64_t)pk_row[lo] * w + pk_x[lo] + k) * d_out, s_pal[idx], d_out);
        }
        wave_sync();  // the table is read before the next chunk overwrites it
    }
}

// Field tables of a 16- or 32-bit file: s_lut[c][v] = the 8-bit value of field c's (top) 8 bits v.
struct BmpFields {
    uint32_t mask[4];
    int32_t shift[4];  // the field's lowest bit, moved up for a field wider than 8 bits
};

// The segment's pixel x as R | G << 8 | B << 16 | A << 24.
template <int BITS>
__device__ __forceinline__ uint32_t bmp_seg_pixel(const uint8_t* seg, int x, const uint32_t* s_pal, const uint8_t (*s_lut)[256],
                                                  const BmpFields& F) {
    if (BITS == 1) return s_pal[(seg[x >> 3] >> (7 - (x & 7))) & 1];
    if (BITS == 4) return s_pal[(seg[x >> 1] >> ((x & 1) ? 0 : 4)) & 15];
    if (BITS == 8) return s_pal[seg[x]];
    if (BITS == 24) return seg[3 * x + 2] | (uint32_t)seg[3 * x + 1] << 8 | (uint32_t)seg[3 * x] << 16;
    const uint32_t v = BITS == 16 ? bmp_u16(seg + 2 * x) : bmp_u32(seg + 4 * x);
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) r |= (uint32_t)s_lut[c][((v & F.mask[c]) >> F.shift[c]) & 255u] << (8 * c);
    return r;
}

// The rows of one raw image, one workgroup per output row at a time, with the bit count and the
// channels as constants (the divisions by D below are then multiplications). A row goes in segments
// of kBmpSeg pixels through LDS; the segment's output bytes leave as 16-byte stores where the
// absolute address is aligned and as single bytes before and after.
template <int BITS, int D>
__device__ __forceinline__ void bmp_stream_rows(const BmpHead& H, const uint8_t* file, int64_t fsize, uint8_t* dst, uint8_t* win,
                                                const uint32_t* s_pal, const uint8_t (*s_lut)[256], const BmpFields& F) {
    const int tid = threadIdx.x;
    for (int y = blockIdx.x; y < H.h; y += gridDim.x) {
        const int fy = H.flip ? H.h - 1 - y : y;
        for (int x0 = 0; x0 < H.w; x0 += kBmpSeg) {
            const int nx = min(kBmpSeg, H.w - x0);
            const int ns = (nx * BITS + 7) >> 3;  // source bytes of the segment (x0 is a multiple of 8)
            const int64_t s0 = H.ds + (int64_t)fy * H.stride + ((int64_t)x0 * BITS >> 3);
            const int mis = (int)(reinterpret_cast<uintptr_t>(file + s0) & 15);
            __syncthreads();  // the previous segment's readers are done (and the tables are staged)
            fill_window(win, file, fsize, s0 - mis, (mis + ns + 15) & ~15, tid, 256);
            __syncthreads();
            const uint8_t* seg = win + mis;
            // (icx_wave.h's store_segment written out: x, c and the pixel are carried over the 16 bytes)
            uint8_t* optr = dst + ((int64_t)y * H.w + x0) * D;
            const int nb = nx * D;
            const int head = min(nb, (int)((16 - (reinterpret_cast<uintptr_t>(optr) & 15)) & 15));
            const int nv = (nb - head) / 16;
            for (int v = tid; v < nv; v += 256) {
                const int b0 = head + 16 * v;
                int x = b0 / D, c = b0 - x * D;
                if (BITS == 24) {  // one LDS byte per output byte: B <-> R
                    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int b = 0; b < 16; ++b) {
                        wd[b >> 2] |= (uint32_t)seg[3 * x + 2 - c] << (8 * (b & 3));
                        if (++c == 3) { c = 0; ++x; }
                    }
                    *reinterpret_cast<uint4*>(optr + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                    continue;
                }
                uint32_t px = bmp_seg_pixel<BITS>(seg, x, s_pal, s_lut, F);
                uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    wd[b >> 2] |= ((px >> (8 * c)) & 255u) << (8 * (b & 3));
                    if (++c == D) {
                        c = 0;
                        ++x;
                        px = x < nx ? bmp_seg_pixel<BITS>(seg, x, s_pal, s_lut, F) : 0;
                    }
                }
                *reinterpret_cast<uint4*>(optr + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
            const int tail0 = head + 16 * nv;
            for (int b = tid; b < head + (nb - tail0); b += 256) {
                const int q = b < head ? b : tail0 + (b - head);
                const int x = q / D;
                optr[q] = (uint8_t)(bmp_seg_pixel<BITS>(seg, x, s_pal, s_lut, F) >> (8 * (q - x * D)));
            }
        }
    }
}

// grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_bmp_raw(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                 const BmpDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                 uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kBmpSeg * 4 + 48];
    __shared__ uint32_t s_pal[256];
    __shared__ uint8_t s_lut[4][256];
    const int i = blockIdx.y;
    const BmpDesc& dd = desc[i];
    if (dd.status != kBmpOk || dd.H.rle || dd.H.bits == 24) return;  // (24 bits: k_bmp_raw24)
    const BmpHead H = dd.H;
    const uint8_t* file = data + off[i];
    const int64_t fsize = dd.size;
    uint8_t* dst = out + (int64_t)i * out_stride;
    const int tid = threadIdx.x;
    BmpFields F{};
    if (H.bits <= 8) {
        s_pal[tid] = bmp_pal_rgb(H, file, tid);
    } else if (H.bits != 24) {
        for (int c = 0; c < 4; ++c) {
            const int wd = H.width[c] > 8 ? 8 : H.width[c];
            F.mask[c] = H.mask[c];
            F.shift[c] = H.shift[c] + (H.width[c] - wd);
            s_lut[c][tid] = (uint8_t)bmp_field8((uint32_t)tid, wd ? (1u << wd) - 1 : 0, 0, wd);
        }
    }
    switch (H.bits * 8 + H.d) {  // (bmp_parse gives no other pair)
    case 1 * 8 + 3: bmp_stream_rows<1, 3>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 4 * 8 + 3: bmp_stream_rows<4, 3>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 8 * 8 + 3: bmp_stream_rows<8, 3>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 8 * 8 + 1: bmp_stream_rows<8, 1>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 16 * 8 + 3: bmp_stream_rows<16, 3>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 16 * 8 + 4: bmp_stream_rows<16, 4>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 32 * 8 + 3: bmp_stream_rows<32, 3>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    case 32 * 8 + 4: bmp_stream_rows<32, 4>(H, file, fsize, dst, win, s_pal, s_lut, F); break;
    }
}

// The same for 24-bit files, in a kernel of its own: its loop (one LDS byte per output byte,
// sixteen loads in flight) takes more registers than all the others together, and shared with them
// it measured 0.63 ms where this takes 0.40. grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_bmp_raw24(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                   const BmpDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                   uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kBmpSeg * 3 + 48];
    const int i = blockIdx.y;
    const BmpDesc& dd = desc[i];
    if (dd.status != kBmpOk || dd.H.rle || dd.H.bits != 24) return;
    const BmpHead H = dd.H;
    bmp_stream_rows<24, 3>(H, data + off[i], dd.size, out + (int64_t)i * out_stride, win, nullptr, nullptr, BmpFields{});
}

__global__ void k_bmp_finish(int n, const BmpDesc* __restrict__ desc, int32_t* __restrict__ status,
                             int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BmpDesc& dd = desc[i];
    // (a pending image that k_bmp_chain did not settle cannot be: reported as a failure of ours)
    const int32_t st = dd.status != kBmpPending ? dd.status : -1;
    const bool ok = st == kBmpOk;
    status[i] = st;
    dims[3 * i + 0] = ok ? dd.H.w : 0;
    dims[3 * i + 1] = ok ? dd.H.h : 0;
    dims[3 * i + 2] = ok ? dd.H.d : 0;
}

// ------------------------------------------------------------------------------- write
struct BmpJob {
    const uint8_t* src;
    int32_t w, h;
    int32_t status, pad_;
};

// One wave per image: the file's size and status, and its header built in LDS and copied out.
__global__ __launch_bounds__(64) void k_bmpw_head(BmpJob* __restrict__ jobs, int d, uint8_t* __restrict__ out,
                                                  uint64_t out_stride, uint64_t* __restrict__ sizes,
                                                  int32_t* __restrict__ status) {
    __shared__ uint8_t s_head[54 + 1024];
    const int i = blockIdx.x, lane = threadIdx.x;
    BmpJob& J = jobs[i];
    if (J.status != kBmpOk) {
        if (lane == 0) { sizes[i] = 0; status[i] = J.status; }
        return;
    }
    const uint64_t total = bmp_encode_bound(J.w, J.h, d);
    const bool fits = total <= out_stride;
    if (fits && lane == 0) bmp_write_header(s_head, J.w, J.h, d);
    __syncthreads();
    if (fits) {
        uint8_t* o = out + (uint64_t)i * out_stride;
        for (int b = lane; b < bmp_write_offbits(d); b += 64) o[b] = s_head[b];
    }
    __syncthreads();  // every lane has read J.status before lane 0 may change it
    if (lane == 0) {
        sizes[i] = total;
        status[i] = fits ? kBmpOk : kBmpTooLarge;
        if (!fits) J.status = kBmpTooLarge;  // k_bmpw_rows skips it
    }
}

// grid (x: rows, y: image): file row r is image row h - 1 - r, B,G,R(,A) or grey, zero padded to
// 4 bytes; segments through LDS, out by 16-byte stores where the absolute address is aligned.
__global__ __launch_bounds__(256) void k_bmpw_rows(const BmpJob* __restrict__ jobs, int d, uint8_t* __restrict__ out,
                                                   uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kBmpSeg * 4 + 32];
    const BmpJob& J = jobs[blockIdx.y];
    if (J.status != kBmpOk) return;
    const int w = J.w, h = J.h, tid = threadIdx.x;
    const int64_t stride = bmp_write_stride(w, d), src_size = (int64_t)w * h * d;
    uint8_t* dst = out + (uint64_t)blockIdx.y * out_stride + bmp_write_offbits(d);
    for (int r = blockIdx.x; r < h; r += gridDim.x) {
        for (int x0 = 0; x0 < w; x0 += kBmpSeg) {
            const int nx = min(kBmpSeg, w - x0);
            const int64_t s0 = ((int64_t)(h - 1 - r) * w + x0) * d;
            const int mis = (int)(reinterpret_cast<uintptr_t>(J.src + s0) & 15);
            __syncthreads();  // the previous segment's readers are done
            fill_window(win, J.src, src_size, s0 - mis, (mis + nx * d + 15) & ~15, tid, 256);
            __syncthreads();
            const uint8_t* seg = win + mis;
            auto byte_at = [&](int q) -> uint32_t {  // byte q of the segment's part of the file row
                if (q >= nx * d) return 0;  // the pad bytes
                if (d == 1) return seg[q];
                const int x = q / d, c = q - x * d;
                return c < 3 ? seg[x * d + 2 - c] : seg[x * d + 3];
            };
            const int nb = nx * d + (x0 + nx == w ? (int)(stride - (int64_t)w * d) : 0);
            store_segment(dst + (int64_t)r * stride + (int64_t)x0 * d, nb, tid, byte_at);
        }
    }
}

// ------------------------------------------------------------------------------- host
int bmp_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int64_t* stream) {
    BmpHead H{};
    const int rc = bmp_parse(data, size, &H);
    if (rc == kBmpOk) {
        *w = H.w;
        *h = H.h;
        *d = H.d;
        if (stream) *stream = H.rle ? size - H.ds + 1 : 0;
    }
    return rc;
}

int64_t bmp_stream_bound(int max_w, int max_h) { return 2 * (int64_t)max_w * max_h + 2 * (int64_t)max_h + 2; }

bool bmp_ws_alloc(BmpWs& ws, Blocks& mem, int max_images, int max_w, int max_h, int64_t stream_cap) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.tiles_cap = stream_cap > 0 ? stream_cap / kBmpTile + 1 : 0;
    const size_t n = (size_t)max_images, tiles = n * (size_t)ws.tiles_cap;
    if (!mem.alloc(ws.desc, n * sizeof(BmpDesc))) return false;
    return !tiles || (mem.alloc(ws.summary, tiles * kBmpEntries * 16) && mem.alloc(ws.entry, tiles * 4) &&
                      mem.alloc(ws.cur_x, tiles * 4) && mem.alloc(ws.cur_y, tiles * 4));
}

void launch_bmp_decode(const BmpWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    const int nb = (n + 63) / 64;
    const unsigned tiles = (unsigned)ws.tiles_cap;
    const int rows = rows_grid(ws.max_h, n);
    S.begin(kStParse);
    hipLaunchKernelGGL(k_bmp_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.max_w, ws.max_h,
                       ws.tiles_cap);
    S.end(kStParse);
    S.begin(kStUnstuff);  // locating the packets
    if (tiles) {
        hipLaunchKernelGGL(k_bmp_tiles, dim3(tiles, n), dim3(256), 0, st, d_data, d_off, ws.desc,
                           reinterpret_cast<uint4*>(ws.summary), ws.tiles_cap);
        hipLaunchKernelGGL(k_bmp_chain, dim3(n), dim3(256), 0, st, ws.desc, reinterpret_cast<const uint4*>(ws.summary),
                           ws.entry, ws.cur_x, ws.cur_y, ws.tiles_cap);
    }
    S.end(kStUnstuff);
    S.begin(kStWrite);  // the background of run-length coded images
    if (tiles) hipLaunchKernelGGL(k_bmp_fill, dim3(rows, n), dim3(256), 0, st, d_data, d_off, ws.desc, d_out, out_stride);
    S.end(kStWrite);
    S.begin(kStEntropy);  // run-length decoding
    if (tiles)
        hipLaunchKernelGGL(k_bmp_expand, dim3((tiles + 3) / 4, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.entry,
                           ws.cur_x, ws.cur_y, d_out, out_stride, ws.tiles_cap);
    S.end(kStEntropy);
    S.begin(kStConvert);  // raw files
    hipLaunchKernelGGL(k_bmp_raw24, dim3(rows, n), dim3(256), 0, st, d_data, d_off, ws.desc, d_out, out_stride);
    hipLaunchKernelGGL(k_bmp_raw, dim3(rows, n), dim3(256), 0, st, d_data, d_off, ws.desc, d_out, out_stride);
    hipLaunchKernelGGL(k_bmp_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    S.end(kStConvert);
}

struct BmpwWs {
    Buf<BmpJob> jobs;
};
BmpwWs* bmpw_ws_create() { return new BmpwWs(); }
void bmpw_ws_destroy(BmpwWs* w) { delete w; }

int bmp_encode_batch(hipStream_t st, BmpwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err) {
    std::vector<BmpJob> jobs((size_t)n);
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        BmpJob& J = jobs[i];
        J = BmpJob{};
        J.src = d_src[i];
        J.w = widths[i];
        J.h = heights[i];
        J.status = J.src && bmp_write_args_ok(J.w, J.h, d) ? kBmpOk : kBmpInvalidArgument;
        if (J.status == kBmpOk) max_h = std::max(max_h, J.h);
    }
    if (jobs_upload("bmp_encode_batch", ws.jobs, jobs, st, err)) return -1;
    const int gy = rows_grid(max_h, n);
    hipLaunchKernelGGL(k_bmpw_head, dim3(n), dim3(64), 0, st, ws.jobs.p, d, d_out, out_stride, d_sizes, d_status);
    hipLaunchKernelGGL(k_bmpw_rows, dim3(gy, n), dim3(256), 0, st, ws.jobs.p, d, d_out, out_stride);
    return encode_finish("bmp_encode_batch", st, err);
}

}  // namespace icx
