// icx_tga.hip -- Targa read and write on gfx950: Image::readTga (codecs.cpp:1304-1407) and
// Image::writeTga (:1410-1437), with the contract and deviations of include/icx.h.
//
// Read. Raw types (1, 2, 3) are one streaming kernel. A run-length stream (9, 10, 11) has no row
// markers: where a packet starts depends on every packet before it. It is cut into tiles of
// kTgaTile bytes and located without a serial walk over the packets:
//   k_tga_parse    header walk (tga_parse), one lane per image
//   k_tga_tiles    one workgroup per tile: every byte position taken as a would-be packet header
//                  gets its successor and pixel count; pointer doubling in LDS then tells, for a
//                  chain entering the tile at any offset, where it leaves the tile (or that it
//                  meets a packet the file cuts short) and with how many pixels
//   k_tga_chain    one workgroup per image: tile t+1's entry offset and pixel base from tile t's
//                  summary (rows of summaries staged through LDS, 16 tiles per global round trip);
//                  a chain that fails with pixels still missing is TRUNCATED here
//   k_tga_expand   one wave per tile: the packet headers are walked from an LDS window, 256 packets
//                  at a time, into a table of packet starts and pixel counts; the lanes then take
//                  one pixel each (its packet by binary search), so neighbouring lanes store
//                  neighbouring pixels (channel order, palette, row order applied on the way out).
//                  The tile in which the last pixel arrives decides OK or MALFORMED
//   k_tga_raw      rows of raw files: source row segment -> LDS by aligned 16-byte loads, out by
//                  16-byte stores at the absolute address's alignment (bytes at the ragged ends)
// No stream is declined: every packet chain goes through the tiles, so there is no serial
// fallback walk.
//
// Write. Uncompressed: the header and the same streaming kernel (R,G,B -> B,G,R is its own
// inverse). Run-length coded (C ABI extension): the greedy per-row rule of icx_tga_core.h's
// tga_pack_row in parallel form, a wave per row --
//   k_tgaw_rows    equality flags, run segments and literal regions by wave scans -> row bytes
//   k_tgaw_prefix  exclusive sum over an image's rows, its size, status and header
//   k_tgaw_emit    the same scans again, every packet's bytes stored by its own pixels
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_tga_core.h"
#include "icx_wave.h"

namespace icx {

constexpr int kTgaTile = 4096;     // stream bytes per tile (tests/test_gpu_tga.py names it)
constexpr int kTgaMaxPkt = 513;    // longest packet: header + 128 pixels of 4 bytes
constexpr int kTgaEntries = 516;   // entry offsets 0 .. 512 of a tile, padded to a multiple of 4
constexpr int kTgaWin = kTgaTile + 544;  // expand window: a tile, its last packet's overhang, 16 for alignment
constexpr uint32_t kTgaFailCode = 0xFFF;
constexpr int kTgaChunk = 256;     // packets k_tga_expand locates before it writes their pixels
constexpr int kTgaChainRows = 16;  // summary rows staged per round of k_tga_chain
constexpr int kTgaSeg = 1024;      // pixels per row segment of the streaming kernel

struct TgaDesc {
    TgaHead H;
    int64_t size;
    int32_t status;
    int32_t ntiles;  // RLE: tiles that can hold packets of this image
    int32_t last;    // the tile in which the last pixel arrives (k_tga_chain)
    int32_t verdict; // kTgaOk / kTgaMalformed from that tile's wave (k_tga_expand); status stays
                     // kTgaPending until k_tga_finish folds it in, so no kernel reads a field
                     // that another workgroup of the same launch writes
};

__global__ void k_tga_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ size, TgaDesc* __restrict__ desc, int max_w, int max_h,
                            int64_t tiles_cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TgaDesc dd{};
    dd.size = (int64_t)size[i];
    dd.last = -1;
    dd.verdict = kTgaPending;
    dd.status = tga_parse(data + off[i], dd.size, &dd.H);
    if (dd.status == kTgaOk) {
        if (dd.H.w > max_w || dd.H.h > max_h || (dd.H.rle && tiles_cap == 0)) {  // (0: a workspace for raw files)
            dd.status = kTgaTooLarge;
        } else if (dd.H.rle) {
            dd.status = kTgaPending;
            // no chain of packets that still misses a pixel is longer than npix * (bpp + 1) bytes
            const int64_t len = min(dd.size - dd.H.ds, (int64_t)dd.H.w * dd.H.h * (dd.H.bpp + 1));
            dd.ntiles = (int32_t)((len + kTgaTile - 1) / kTgaTile);
        }
    }
    desc[i] = dd;
}

// grid (x: tile, y: image)
__global__ __launch_bounds__(256) void k_tga_tiles(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                   const TgaDesc* __restrict__ desc, uint32_t* __restrict__ summary,
                                                   int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kTgaTile + 16];
    __shared__ uint16_t s_nxt[kTgaTile];
    __shared__ uint32_t s_cnt[kTgaTile];
    const int i = blockIdx.y, t = blockIdx.x;
    const TgaDesc& dd = desc[i];
    if (dd.status != kTgaPending || t >= dd.ntiles) return;
    const uint8_t* d = data + off[i];
    const int64_t n = dd.size, tile0 = dd.H.ds + (int64_t)t * kTgaTile;
    const int bpp = dd.H.bpp;
    const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
    fill_window(win, d, n, tile0 - mis, kTgaTile + 16, threadIdx.x, 256);
    __syncthreads();
    constexpr int kPer = kTgaTile / 256;
    constexpr uint16_t kFail = 0xFFFF;
    uint16_t nn[kPer];
    uint32_t cc[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = threadIdx.x + 256 * q;
        const int64_t pos = tile0 + j;
        const int hb = win[mis + j];
        const int count = (hb & 127) + 1;
        const int next = j + 1 + ((hb & 128) ? bpp : count * bpp);
        const bool ok = pos < n && tile0 + next <= n;
        nn[q] = ok ? (uint16_t)next : kFail;  // >= kTgaTile: leaves the tile at next - kTgaTile
        cc[q] = ok ? count : 0;
        s_nxt[j] = nn[q];
        s_cnt[j] = cc[q];
    }
    __syncthreads();
    // a chain inside a tile has at most kTgaTile / 2 packets: 11 doublings reach its end; long
    // packets need fewer, and the rounds stop once every chain has left the tile
    for (int round = 0; round < 12; ++round) {
        bool active = false;
#pragma unroll
        for (int q = 0; q < kPer; ++q) active |= nn[q] < kTgaTile;
        if (!__syncthreads_or(active)) break;
#pragma unroll
        for (int q = 0; q < kPer; ++q)
            if (nn[q] < kTgaTile) {
                const int a = nn[q];
                cc[q] += s_cnt[a];
                nn[q] = s_nxt[a];
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int j = threadIdx.x + 256 * q;
            s_nxt[j] = nn[q];
            s_cnt[j] = cc[q];
        }
    }
    __syncthreads();
    uint32_t* S = summary + ((int64_t)i * tiles_cap + t) * kTgaEntries;
    for (int e = threadIdx.x; e < kTgaEntries; e += 256) {
        uint32_t v = kTgaFailCode << 20;
        if (e < kTgaMaxPkt) {
            const uint32_t nx = s_nxt[e];
            // (nx < kTgaTile cannot be left after the doublings; it would read as a failed chain)
            const uint32_t code = nx == kFail || nx < kTgaTile ? kTgaFailCode : nx - kTgaTile;
            v = (code << 20) | s_cnt[e];
        }
        S[e] = v;
    }
}

// One workgroup per image.
__global__ __launch_bounds__(256) void k_tga_chain(TgaDesc* __restrict__ desc, const uint32_t* __restrict__ summary,
                                                   int32_t* __restrict__ entry, int32_t* __restrict__ pbase,
                                                   int64_t tiles_cap) {
    __shared__ uint32_t rows[kTgaChainRows * kTgaEntries];
    __shared__ int s_done;
    const int i = blockIdx.x;
    TgaDesc& dd = desc[i];
    if (dd.status != kTgaPending) return;
    const int ntiles = dd.ntiles;
    const int64_t npix = (int64_t)dd.H.w * dd.H.h;
    const uint32_t* S = summary + (int64_t)i * tiles_cap * kTgaEntries;
    int32_t* E = entry + (int64_t)i * tiles_cap;
    int32_t* B = pbase + (int64_t)i * tiles_cap;
    int e = 0;         // thread 0's state
    int64_t base = 0;
    if (threadIdx.x == 0) s_done = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += kTgaChainRows) {
        const int nr = min(kTgaChainRows, ntiles - t0);
        for (int k = threadIdx.x; k < nr * kTgaEntries; k += 256) rows[k] = S[(int64_t)t0 * kTgaEntries + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int r = 0; r < nr; ++r) {
                const int t = t0 + r;
                E[t] = e;
                B[t] = (int32_t)base;
                const uint32_t s = rows[r * kTgaEntries + e];
                const int64_t c = s & 0xFFFFFu;
                const uint32_t code = s >> 20;
                if (base + c >= npix) {  // the last pixel arrives in this tile: k_tga_expand decides
                    dd.last = t;
                    s_done = 1;
                    break;
                }
                if (code == kTgaFailCode) {  // a packet the file cuts short, pixels still missing
                    dd.status = kTgaTruncated;
                    s_done = 1;
                    break;
                }
                base += c;
                e = (int)code;
            }
        }
        __syncthreads();
        if (s_done) return;
    }
    if (threadIdx.x == 0) dd.status = kTgaTruncated;  // the next header byte is past the file's end
}

// grid (x: groups of 4 tiles, y: image); one wave per tile.
__global__ __launch_bounds__(256) void k_tga_expand(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                    TgaDesc* __restrict__ desc, const int32_t* __restrict__ entry,
                                                    const int32_t* __restrict__ pbase, uint8_t* __restrict__ out,
                                                    uint64_t out_stride, int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win_all[4][kTgaWin];
    __shared__ uint16_t pk_pos_all[4][kTgaChunk];
    __shared__ uint32_t pk_end_all[4][kTgaChunk];
    const int i = blockIdx.y, lane = threadIdx.x & 63;
    // (readfirstlane: what is the same in every lane of the wave is kept in scalar registers, so
    // the packet walk below issues scalar instructions)
    const int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    TgaDesc& dd = desc[i];
    if (dd.status != kTgaPending || dd.last < 0 || t > dd.last) return;
    const TgaHead H = dd.H;
    const uint8_t* d = data + off[i];
    const uint8_t* map = d + H.map_at;
    uint8_t* o = out + (int64_t)i * out_stride;
    const int64_t n = dd.size, tile0 = H.ds + (int64_t)t * kTgaTile, npix = (int64_t)H.w * H.h;
    uint8_t* win = win_all[threadIdx.x >> 6];
    const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
    fill_window(win, d, n, tile0 - mis, kTgaWin, lane, 64);
    wave_sync();
    uint16_t* pk_pos = pk_pos_all[threadIdx.x >> 6];
    uint32_t* pk_end = pk_end_all[threadIdx.x >> 6];
    int pos = __builtin_amdgcn_readfirstlane(entry[(int64_t)i * tiles_cap + t]);
    int64_t P = __builtin_amdgcn_readfirstlane(pbase[(int64_t)i * tiles_cap + t]);
    const int avail = (int)min<int64_t>(n - tile0, kTgaWin);  // file bytes from the tile's start
    bool over = false, stop = false;
    while (!stop && pos < kTgaTile && P < npix) {
        const uint32_t rem = (uint32_t)min<int64_t>(npix - P, 0x7FFFFFFF);  // pixels still missing
        // the next kTgaChunk packets: every lane walks the same headers, lane 0 notes where each
        // packet starts and how many of the chunk's pixels end with it
        int np = 0;
        uint32_t cum = 0;
        while (np < kTgaChunk && pos < kTgaTile && cum < rem) {
            const int hb = __builtin_amdgcn_readfirstlane(win[mis + pos]);
            const int count = (hb & 127) + 1;
            const int payload = (hb & 128) ? H.bpp : count * H.bpp;
            if (pos + 1 + payload > avail) { stop = true; break; }  // (k_tga_chain never sends a tile here)
            if ((uint32_t)count > rem - cum) { over = stop = true; break; }
            cum += count;
            if (lane == 0) {
                pk_pos[np] = (uint16_t)pos;
                pk_end[np] = cum;
            }
            ++np;
            pos += 1 + payload;
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
            const uint8_t* pk = win + mis + pk_pos[lo];
            const uint8_t* src = pk + 1 + ((pk[0] & 128) ? 0 : (q - first) * H.bpp);
            tga_store_px(H, map, src, o + tga_out_index(H, P + q) * H.d);
        }
        P += cum;
        wave_sync();  // the table is read before the next chunk overwrites it
    }
    if (t == dd.last && lane == 0) dd.verdict = over ? kTgaMalformed : P == npix ? kTgaOk : kTgaTruncated;
}

// Rows of h x w stored elements (file + ds, bpp bytes each) -> d bytes per pixel at dst, one
// workgroup per output row at a time. A row goes in segments of kTgaSeg pixels through LDS;
// the segment's output bytes leave as 16-byte stores where the absolute address is aligned and
// as single bytes before and after.
__device__ __forceinline__ void tga_stream_rows(const TgaHead& H, const uint8_t* file, int64_t fsize, uint8_t* dst,
                                                uint8_t* win) {
    const uint8_t* map = file + H.map_at;
    const int d = H.d, bpp = H.bpp, tid = threadIdx.x;
    auto byte_at = [&](const uint8_t* seg, int x, int c) -> uint32_t {  // channel c of the segment's pixel x
        const uint8_t* s = seg + x * bpp;
        if (H.pal) {
            const int idx = (bpp == 2 ? s[0] | s[1] << 8 : s[0]) - H.map_origin;
            if (idx < 0 || idx >= H.map_len) return 0;
            s = map + (int64_t)idx * d;
        }
        return d == 1 ? s[0] : c < 3 ? s[2 - c] : s[3];
    };
    for (int y = blockIdx.x; y < H.h; y += gridDim.x) {
        const int fy = H.topdown ? y : H.h - 1 - y;
        for (int x0 = 0; x0 < H.w; x0 += kTgaSeg) {
            const int nx = min(kTgaSeg, H.w - x0);
            const int64_t s0 = H.ds + ((int64_t)fy * H.w + x0) * bpp;
            const int mis = (int)(reinterpret_cast<uintptr_t>(file + s0) & 15);
            __syncthreads();  // the previous segment's readers are done
            fill_window(win, file, fsize, s0 - mis, (mis + nx * bpp + 15) & ~15, tid, 256);
            __syncthreads();
            const uint8_t* seg = win + mis;
            // (icx_wave.h's store_segment written out: b0 / d once per 16 bytes, not once per byte)
            uint8_t* optr = dst + ((int64_t)y * H.w + x0) * d;
            const int nb = nx * d;
            const int head = min(nb, (int)((16 - (reinterpret_cast<uintptr_t>(optr) & 15)) & 15));
            const int nv = (nb - head) / 16;
            for (int v = tid; v < nv; v += 256) {
                const int b0 = head + 16 * v;
                int x = b0 / d, c = b0 - x * d;
                uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    wd[b >> 2] |= byte_at(seg, x, c) << (8 * (b & 3));
                    if (++c == d) { c = 0; ++x; }
                }
                *reinterpret_cast<uint4*>(optr + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
            const int tail0 = head + 16 * nv;
            for (int b = tid; b < head + (nb - tail0); b += 256) {
                const int q = b < head ? b : tail0 + (b - head);
                const int x = q / d;
                optr[q] = (uint8_t)byte_at(seg, x, q - x * d);
            }
        }
    }
}

// grid (x: rows, y: image)
__global__ __launch_bounds__(256) void k_tga_raw(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                 const TgaDesc* __restrict__ desc, uint8_t* __restrict__ out,
                                                 uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kTgaSeg * 4 + 32];
    const int i = blockIdx.y;
    const TgaDesc& dd = desc[i];
    if (dd.status != kTgaOk || dd.H.rle) return;
    const TgaHead H = dd.H;
    tga_stream_rows(H, data + off[i], dd.size, out + (int64_t)i * out_stride, win);
}

__global__ void k_tga_finish(int n, const TgaDesc* __restrict__ desc, int32_t* __restrict__ status,
                             int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TgaDesc& dd = desc[i];
    // (a pending image whose last tile gave no verdict cannot be: reported as a failure of ours)
    const int32_t st = dd.status != kTgaPending ? dd.status : dd.verdict != kTgaPending ? dd.verdict : -1;
    const bool ok = st == kTgaOk;
    status[i] = st;
    dims[3 * i + 0] = ok ? dd.H.w : 0;
    dims[3 * i + 1] = ok ? dd.H.h : 0;
    dims[3 * i + 2] = ok ? dd.H.d : 0;
}

// ------------------------------------------------------------------------------- write
struct TgaJob {
    const uint8_t* src;
    int32_t w, h;
    int32_t status, pad_;
    uint64_t row0;  // the image's first row in TgawWs::rowoff
};

// tga_pack_row in parallel form, one wave per row, 64 pixels at a time. With o = a pixel's offset in
// its stretch of equal pixels and eq = "equals its right neighbour": a pixel is in a run packet
// when eq, or when it ends a stretch at o % 128 != 0; otherwise it is literal (a single pixel, or
// the 129th, 257th ... of a stretch). Run packets start at o % 128 == 0, literal packets every
// 128 pixels of a region of adjacent literal pixels. A packet's header byte (and a run's pixel)
// is stored by the packet's last pixel, which knows the count. Returns the row's bytes.
template <bool EMIT>
__device__ __forceinline__ uint32_t tga_rle_row(const uint8_t* row, int w, int d, uint8_t* out, int lane) {
    int s_carry = 0, ls_carry = -1, o_last = 0;
    uint32_t bytes = 0;
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int k = c0 + lane;
        const bool valid = k < w;
        const uint32_t v = valid ? tga_px_word(row, d, k) : 0;
        const bool eqm1 = valid && k > 0 && tga_px_word(row, d, k - 1) == v;
        const uint32_t vp1 = k + 1 < w ? tga_px_word(row, d, k + 1) : 0;
        const bool eq = k + 1 < w && v == vp1;
        const bool eqp1 = k + 2 < w && vp1 == tga_px_word(row, d, k + 2);
        const int s = max(wave_max_scan(valid && !eqm1 ? k : -1, lane), s_carry);
        const int o = k - s;
        int o_up = __shfl_up(o, 1);
        if (lane == 0) o_up = o_last;
        const int o_prev = eqm1 ? o - 1 : o_up;
        const bool run = eq || (o > 0 && (o & 127) != 0);
        const bool lit = valid && !run;
        const bool prev_lit = k > 0 && !eqm1 && (o_prev & 127) == 0;
        const int ls = max(wave_max_scan(lit && !prev_lit ? k : -1, lane), ls_carry);
        const int lo = k - ls;
        const uint32_t size = !valid ? 0 : run ? ((o & 127) == 0 ? 1 + d : 0) : d + ((lo & 127) == 0 ? 1 : 0);
        const uint32_t incl = wave_sum_scan(size, lane) + bytes;
        if (EMIT && valid) {
            if (run) {
                if ((o & 127) == 127 || !eq) {
                    uint8_t* p = out + (incl - (1 + d));
                    p[0] = (uint8_t)(0x80 | (o & 127));
                    tga_put_file_px(p + 1, v, d);
                }
            } else {
                tga_put_file_px(out + (incl - d), v, d);
                if ((lo & 127) == 127 || k + 1 >= w || eqp1) out[incl - ((lo & 127) + 1) * d - 1] = (uint8_t)(lo & 127);
            }
        }
        s_carry = __shfl(s, 63);
        ls_carry = __shfl(ls, 63);
        o_last = __shfl(o, 63);
        bytes = __shfl(incl, 63);
    }
    return bytes;
}

// grid (x: groups of 4 rows, y: image)
__global__ __launch_bounds__(256) void k_tgaw_rows(const TgaJob* __restrict__ jobs, int d, uint64_t* __restrict__ rowoff) {
    const TgaJob& J = jobs[blockIdx.y];
    if (J.status != kTgaOk) return;
    const int lane = threadIdx.x & 63;
    for (int y = blockIdx.x * 4 + (threadIdx.x >> 6); y < J.h; y += gridDim.x * 4) {
        const uint32_t b = tga_rle_row<false>(J.src + (int64_t)y * J.w * d, J.w, d, nullptr, lane);
        if (lane == 0) rowoff[J.row0 + y] = b;
    }
}

// One wave per image: row sizes -> row offsets in the file; size, status and header.
__global__ __launch_bounds__(64) void k_tgaw_prefix(TgaJob* __restrict__ jobs, int d, int rle, uint64_t* __restrict__ rowoff,
                                                    uint8_t* __restrict__ out, uint64_t out_stride,
                                                    uint64_t* __restrict__ sizes, int32_t* __restrict__ status) {
    const int i = blockIdx.x, lane = threadIdx.x;
    TgaJob& J = jobs[i];
    if (J.status != kTgaOk) {
        if (lane == 0) { sizes[i] = 0; status[i] = J.status; }
        return;
    }
    uint64_t total = (uint64_t)J.w * J.h * d;
    if (rle) {
        total = 0;
        for (int y0 = 0; y0 < J.h; y0 += 64) {
            const int y = y0 + lane;
            const uint64_t v = y < J.h ? rowoff[J.row0 + y] : 0, incl = wave_sum_scan(v, lane);
            if (y < J.h) rowoff[J.row0 + y] = 18 + total + incl - v;
            total += __shfl(incl, 63);
        }
    }
    if (lane == 0) {
        const bool fits = 18 + total <= out_stride;
        sizes[i] = 18 + total;
        status[i] = fits ? kTgaOk : kTgaTooLarge;
        if (fits) tga_write_header(out + (uint64_t)i * out_stride, J.w, J.h, d, rle);
        else J.status = kTgaTooLarge;  // k_tgaw_emit / k_tgaw_raw skip it
    }
}

__global__ __launch_bounds__(256) void k_tgaw_emit(const TgaJob* __restrict__ jobs, int d, const uint64_t* __restrict__ rowoff,
                                                   uint8_t* __restrict__ out, uint64_t out_stride) {
    const TgaJob& J = jobs[blockIdx.y];
    if (J.status != kTgaOk) return;
    const int lane = threadIdx.x & 63;
    uint8_t* o = out + (uint64_t)blockIdx.y * out_stride;
    for (int y = blockIdx.x * 4 + (threadIdx.x >> 6); y < J.h; y += gridDim.x * 4)
        tga_rle_row<true>(J.src + (int64_t)y * J.w * d, J.w, d, o + rowoff[J.row0 + y], lane);
}

// grid (x: rows, y: image): the uncompressed payload.
__global__ __launch_bounds__(256) void k_tgaw_raw(const TgaJob* __restrict__ jobs, int d, uint8_t* __restrict__ out,
                                                  uint64_t out_stride) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kTgaSeg * 4 + 32];
    const TgaJob& J = jobs[blockIdx.y];
    if (J.status != kTgaOk) return;
    TgaHead H{};
    H.w = J.w;
    H.h = J.h;
    H.d = H.bpp = d;
    H.topdown = 1;
    tga_stream_rows(H, J.src, (int64_t)J.w * J.h * d, out + (uint64_t)blockIdx.y * out_stride + 18, win);
}

// ------------------------------------------------------------------------------- host
int tga_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d) {
    TgaHead H{};
    const int rc = tga_parse(data, size, &H);
    if (rc == kTgaOk) { *w = H.w; *h = H.h; *d = H.d; }
    return rc;
}

bool tga_ws_alloc(TgaWs& ws, Blocks& mem, int max_images, int max_w, int max_h, bool rle) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.tiles_cap = rle ? ((int64_t)max_w * max_h * 5 + kTgaTile - 1) / kTgaTile + 1 : 0;
    const size_t n = (size_t)max_images, tiles = n * (size_t)ws.tiles_cap;
    if (!mem.alloc(ws.desc, n * sizeof(TgaDesc))) return false;
    return !rle || (mem.alloc(ws.summary, tiles * kTgaEntries * 4) && mem.alloc(ws.entry, tiles * 4) &&
                    mem.alloc(ws.pbase, tiles * 4));
}

void launch_tga_decode(const TgaWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    const int nb = (n + 63) / 64;
    const unsigned tiles = (unsigned)ws.tiles_cap;
    S.begin(kStParse);
    hipLaunchKernelGGL(k_tga_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, ws.max_w, ws.max_h,
                       ws.tiles_cap);
    S.end(kStParse);
    S.begin(kStUnstuff);  // locating the packets
    if (tiles) {
        hipLaunchKernelGGL(k_tga_tiles, dim3(tiles, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.summary, ws.tiles_cap);
        hipLaunchKernelGGL(k_tga_chain, dim3(n), dim3(256), 0, st, ws.desc, ws.summary, ws.entry, ws.pbase, ws.tiles_cap);
    }
    S.end(kStUnstuff);
    S.begin(kStEntropy);  // run-length decoding
    if (tiles)
        hipLaunchKernelGGL(k_tga_expand, dim3((tiles + 3) / 4, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.entry,
                           ws.pbase, d_out, out_stride, ws.tiles_cap);
    S.end(kStEntropy);
    S.begin(kStConvert);  // raw files
    hipLaunchKernelGGL(k_tga_raw, dim3(rows_grid(ws.max_h, n), n), dim3(256), 0, st,
                       d_data, d_off, ws.desc, d_out, out_stride);
    hipLaunchKernelGGL(k_tga_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    S.end(kStConvert);
}

struct TgawWs {
    Buf<TgaJob> jobs;
    Buf<uint64_t> rowoff;
};
TgawWs* tgaw_ws_create() { return new TgawWs(); }
void tgaw_ws_destroy(TgawWs* w) { delete w; }

int tga_encode_batch(hipStream_t st, TgawWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err) {
    std::vector<TgaJob> jobs((size_t)n);
    uint64_t rows = 0;
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        TgaJob& J = jobs[i];
        J = TgaJob{};
        J.src = d_src[i];
        J.w = widths[i];
        J.h = heights[i];
        J.row0 = rows;
        J.status = J.src && tga_write_args_ok(J.w, J.h, d) ? kTgaOk : kTgaInvalidArgument;
        if (J.status != kTgaOk) continue;
        rows += (uint64_t)J.h;
        max_h = std::max(max_h, J.h);
    }
    if (jobs_upload("tga_encode_batch", ws.jobs, jobs, st, err, ws.rowoff.reserve((rows + 1) * 8))) return -1;
    const int gy = rows_grid(max_h, n);
    if (rle) {
        const int gx = std::max(1, std::min((max_h + 3) / 4, 16384));
        hipLaunchKernelGGL(k_tgaw_rows, dim3(gx, n), dim3(256), 0, st, ws.jobs.p, d, ws.rowoff.p);
        hipLaunchKernelGGL(k_tgaw_prefix, dim3(n), dim3(64), 0, st, ws.jobs.p, d, 1, ws.rowoff.p, d_out, out_stride, d_sizes,
                           d_status);
        hipLaunchKernelGGL(k_tgaw_emit, dim3(gx, n), dim3(256), 0, st, ws.jobs.p, d, ws.rowoff.p, d_out, out_stride);
    } else {
        hipLaunchKernelGGL(k_tgaw_prefix, dim3(n), dim3(64), 0, st, ws.jobs.p, d, 0, ws.rowoff.p, d_out, out_stride, d_sizes,
                           d_status);
        hipLaunchKernelGGL(k_tgaw_raw, dim3(gy, n), dim3(256), 0, st, ws.jobs.p, d, d_out, out_stride);
    }
    return encode_finish("tga_encode_batch", st, err);
}

}  // namespace icx
