// icx_pnm.hip -- Netpbm read and write on gfx950: Image::readPbm (codecs.cpp:1034-1100) and
// Image::writePbm (:1102-1167) for P1 .. P6, Pf and PF, with the contract and deviations of
// include/icx.h.
//
// Read.
//   k_pnm_parse    header walk (pnm_check), one lane per image; for a binary type also the job of
//                  the streaming kernel
// The text of P1 / P2 / P3 has no fixed sample width: where sample k starts depends on every byte
// before it. It is cut into tiles of kPnmTile bytes, one wave per tile, 64 bytes per step:
//   k_pnm_tiles    whether a byte lies in a comment is decided from two ballots (the LF / CR bytes
//                  and the '#' bytes before it: the later of the two wins), with one bit carried from
//                  step to step. The bit a tile starts with is not known yet, and it matters only up to
//                  the tile's first LF / CR: the token starts and the first illegal byte are counted
//                  apart for that head (as if outside a comment) and for the rest
//   k_pnm_chain    one workgroup per image: the carried bit, the first sample index and the first
//                  illegal byte of every tile from the summaries (256 staged per round trip); the
//                  tile in which sample w*h*d starts, or that there are too few
//   k_pnm_convert  the same ballots with the carried bit known: a lane at a token start has rank
//                  base + popcount(starts below it), walks its digits (on into the next tiles if
//                  need be) and stores the sample; a value above maxval raises a flag, the lane of the
//                  last sample notes where its token starts
//   k_pnm_finish   BAD_DATA when an illegal byte lies before that position (by position, whichever
//                  kernel saw it) or the flag is up, else TRUNCATED when samples are missing
// Binary rasters and every write are one streaming kernel (pnm_stream_rows): a segment of a row's
// source bytes -> LDS by aligned 16-byte loads, out by 16-byte stores at the absolute address's
// alignment (single bytes at the ragged ends), each output byte fetched through the mode's index
// map: copy, 16- / 32-bit byte swap, 4 -> 3 samples per pixel, bits -> bytes, bytes -> bits; rows
// optionally in reverse order (PFM). Forms without row padding or reversal run as one long row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_pnm_core.h"
#include "icx_wave.h"

namespace icx {

constexpr int kPnmSeg = 4096;  // source and destination bytes per segment of the streaming kernel, at most

enum : int32_t { kPnmCopy = 0, kPnmSwap16, kPnmSwap32, kPnmDrop8, kPnmDrop16, kPnmUnpack, kPnmPack };

struct PnmStream {
    const uint8_t* src;  // readable at [0, src_size)
    int64_t src_size;
    int64_t src_off;     // the first source row
    uint8_t* dst;
    int64_t row_out, row_src;  // bytes of a row at the destination / the source
    int32_t nrows;
    int32_t flip;        // destination row y is source row nrows - 1 - y
    int32_t mode;
    int32_t go;          // 0: nothing to do
};

struct PnmDesc {
    PnmHead H;
    int64_t size;
    int32_t status;      // kPnmPending: an ASCII file whose text is being read (k_pnm_finish decides)
    int32_t ntiles;      // ASCII: tiles of text looked at
    int32_t clamped;     // ASCII: the text is longer than the workspace's tiles
    int32_t last;        // k_pnm_chain: the tile in which the last needed sample starts (too few: the last tile)
    int32_t missing;     // k_pnm_chain: fewer than w*h*d samples
    int32_t oversize;    // k_pnm_convert: a needed sample is above maxval
    int64_t firstbad;    // k_pnm_chain: file offset of the first illegal byte in tiles 0 .. last, or -1
    int64_t last_start;  // k_pnm_convert: file offset of the last needed sample's token
    PnmStream S;         // binary types
};

__global__ void k_pnm_parse(int n, const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ size, PnmDesc* __restrict__ desc, uint8_t* __restrict__ out,
                            uint64_t out_stride, int max_w, int max_h, int64_t tiles_cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PnmDesc dd{};
    dd.size = (int64_t)size[i];
    dd.last = -1;
    dd.firstbad = -1;
    dd.last_start = -1;
    const uint8_t* f = data + off[i];
    dd.status = pnm_check(f, dd.size, &dd.H);
    if (dd.status == kPnmOk) {
        const PnmHead& H = dd.H;
        if (H.w > max_w || H.h > max_h || (uint64_t)pnm_out_bytes(H) > out_stride || (H.ascii && tiles_cap == 0)) {
            dd.status = kPnmTooLarge;
        } else if (H.ascii) {
            dd.status = kPnmPending;
            const int64_t nt = (dd.size - H.rs + kPnmTile - 1) / kPnmTile;
            dd.clamped = nt > tiles_cap;
            dd.ntiles = (int32_t)min(nt, tiles_cap);
        } else {
            PnmStream& S = dd.S;
            S.src = f;
            S.src_size = dd.size;
            S.src_off = H.rs;
            S.dst = out + (uint64_t)i * out_stride;
            S.go = 1;
            if (H.kind == '4') {
                S.mode = kPnmUnpack;
                S.nrows = H.h;
                S.row_out = H.w;
                S.row_src = (H.w + 7) / 8;
            } else if (H.type == kPnmFloat) {
                S.mode = H.le ? kPnmCopy : kPnmSwap32;
                S.nrows = H.h;
                S.flip = 1;
                S.row_out = S.row_src = (int64_t)H.w * H.d * 4;
            } else {
                S.mode = H.type == kPnmUshort ? kPnmSwap16 : kPnmCopy;
                S.nrows = 1;
                S.row_out = S.row_src = pnm_out_bytes(H);
            }
        }
    }
    desc[i] = dd;
}

// ---------------------------------------------------------------------------- ASCII rasters
// What one step's 64 bytes are, given whether the step starts inside a comment (`carry`). Lane l
// looks at byte j of the tile; pc is the byte before it.
struct PnmStep {
    unsigned long long tok, bad, nl, hs, head;
};
__device__ __forceinline__ PnmStep pnm_step(int c, int pc, bool valid, bool p1, bool carry, bool seen_nl, int lane) {
    const bool is_nl = valid && pnm_is_eol(c), is_hs = valid && c == '#';
    PnmStep r;
    r.nl = __ballot(is_nl);
    r.hs = __ballot(is_hs);
    const unsigned long long below = (1ull << lane) - 1, nlb = r.nl & below, hsb = r.hs & below;
    // in a comment: a '#' stands between the byte and the last LF / CR before it (no byte is both,
    // so the mask with the higher top bit is the larger number); with neither before it, as carried
    const bool comment = hsb > nlb || (nlb == 0 && carry);
    const int cls = pnm_class(c, p1);
    r.tok = __ballot(valid && !comment && cls == kPnmClsDigit && (p1 || !pnm_is_digit(pc)));
    r.bad = __ballot(valid && !comment && cls == kPnmClsBad);
    r.head = __ballot(!seen_nl && nlb == 0);  // bytes up to the tile's first LF / CR
    return r;
}
__device__ __forceinline__ bool pnm_carry_out(const PnmStep& r, bool carry) {
    return r.nl ? r.hs > r.nl : (carry || r.hs != 0);
}

// grid (x: groups of 4 tiles, taken in turn, y: image); one wave per tile.
__global__ __launch_bounds__(256) void k_pnm_tiles(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                   const PnmDesc* __restrict__ desc, int4* __restrict__ summary,
                                                   int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win_all[4][kPnmTile + 32];
    const int i = blockIdx.y, lane = threadIdx.x & 63;
    const PnmDesc& dd = desc[i];
    if (dd.status != kPnmPending) return;
    const uint8_t* d = data + off[i];
    const int64_t n = dd.size;
    const bool p1 = dd.H.kind == '1';
    uint8_t* win = win_all[threadIdx.x >> 6];
    const int ntiles = dd.ntiles;
    for (int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); t < ntiles; t += gridDim.x * 4) {
        const int64_t tile0 = dd.H.rs + (int64_t)t * kPnmTile;
        const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
        wave_sync();  // the previous tile's readers are done
        fill_window(win, d, n, tile0 - mis, kPnmTile + 16, lane, 64);
        wave_sync();
        const int avail = (int)min<int64_t>(n - tile0, kPnmTile);
        const int prev0 = t > 0 ? d[tile0 - 1] : ' ';
        bool carry = false, seen_nl = false;  // as if the tile started outside a comment
        int cnt_head = 0, cnt_tail = 0, bad_head = -1, bad_tail = -1;
        for (int j0 = 0; j0 < avail; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j < avail;
            const int c = valid ? win[mis + j] : ' ';
            const int pc = j > 0 ? win[mis + j - 1] : prev0;
            const PnmStep r = pnm_step(c, pc, valid, p1, carry, seen_nl, lane);
            cnt_head += __popcll(r.tok & r.head);
            cnt_tail += __popcll(r.tok & ~r.head);
            if (bad_head < 0 && (r.bad & r.head)) bad_head = j0 + __ffsll((unsigned long long)(r.bad & r.head)) - 1;
            if (bad_tail < 0 && (r.bad & ~r.head)) bad_tail = j0 + __ffsll((unsigned long long)(r.bad & ~r.head)) - 1;
            carry = pnm_carry_out(r, carry);
            seen_nl = seen_nl || r.nl != 0;
        }
        // x: token starts in the head | in the rest << 16; y: the bit carried out for a tile entered
        // outside | inside << 1 a comment (inside: the head is all comment; it ends only at an LF / CR);
        // z, w: the first illegal byte of the head / the rest, -1 for none
        if (lane == 0)
            summary[(int64_t)i * tiles_cap + t] = make_int4(cnt_head | cnt_tail << 16, (carry ? 1 : 0) | ((seen_nl ? carry : true) ? 2 : 0),
                                                            bad_head, bad_tail);
    }
}

// One workgroup per image.
__global__ __launch_bounds__(256) void k_pnm_chain(PnmDesc* __restrict__ desc, const int4* __restrict__ summary,
                                                   int64_t* __restrict__ tbase, int64_t tiles_cap) {
    __shared__ int4 rows[256];
    __shared__ int s_done;
    const int i = blockIdx.x;
    PnmDesc& dd = desc[i];
    if (dd.status != kPnmPending) return;
    const int ntiles = dd.ntiles;
    const int64_t N = (int64_t)dd.H.w * dd.H.h * dd.H.d;
    const int4* S = summary + (int64_t)i * tiles_cap;
    int64_t* B = tbase + (int64_t)i * tiles_cap;
    int64_t base = 0, firstbad = -1;  // thread 0's state
    int in = 0;
    if (threadIdx.x == 0) s_done = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += 256) {
        const int nr = min(256, ntiles - t0);
        if ((int)threadIdx.x < nr) rows[threadIdx.x] = S[t0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int r = 0; r < nr; ++r) {
                const int t = t0 + r;
                const int4 s = rows[r];
                B[t] = base << 1 | in;  // the tile's first sample index and whether it starts in a comment
                const int64_t cnt = (s.x >> 16) + (in ? 0 : (s.x & 0xFFFF));
                const int bad = in ? s.w : (s.z >= 0 ? s.z : s.w);
                if (firstbad < 0 && bad >= 0) firstbad = dd.H.rs + (int64_t)t * kPnmTile + bad;
                if (base + cnt >= N) {  // the last needed sample starts in this tile
                    dd.last = t;
                    s_done = 1;
                    break;
                }
                base += cnt;
                in = (s.y >> in) & 1;
            }
        }
        __syncthreads();
        if (s_done) break;
    }
    if (threadIdx.x == 0) {
        dd.firstbad = firstbad;
        if (!s_done) {
            dd.missing = 1;
            dd.last = ntiles - 1;
            if (dd.clamped) dd.status = kPnmTooLarge;  // the text goes on past the workspace's tiles
        }
    }
}

// grid (x: groups of 4 tiles, taken in turn, y: image); one wave per tile.
__global__ __launch_bounds__(256) void k_pnm_convert(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                     PnmDesc* __restrict__ desc, const int64_t* __restrict__ tbase,
                                                     uint8_t* __restrict__ out, uint64_t out_stride, int64_t tiles_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t win_all[4][kPnmTile + 32];
    const int i = blockIdx.y, lane = threadIdx.x & 63;
    PnmDesc& dd = desc[i];
    if (dd.status != kPnmPending) return;
    const PnmHead H = dd.H;
    const uint8_t* d = data + off[i];
    uint8_t* o = out + (uint64_t)i * out_stride;
    const int64_t n = dd.size, N = (int64_t)H.w * H.h * H.d;
    const bool p1 = H.kind == '1';
    uint8_t* win = win_all[threadIdx.x >> 6];
    const int last = dd.last;
    bool over = false;
    for (int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); t <= last; t += gridDim.x * 4) {
        const int64_t tile0 = H.rs + (int64_t)t * kPnmTile;
        const int mis = (int)(reinterpret_cast<uintptr_t>(d + tile0) & 15);
        wave_sync();  // the previous tile's readers are done
        fill_window(win, d, n, tile0 - mis, kPnmTile + 32, lane, 64);
        wave_sync();
        const int avail = (int)min<int64_t>(n - tile0, kPnmTile);
        const int wlen = kPnmTile + 32 - mis;  // tile bytes [0, wlen) are in the window (zero past the file's end)
        const int prev0 = t > 0 ? d[tile0 - 1] : ' ';
        const int64_t b0 = tbase[(int64_t)i * tiles_cap + t];
        int64_t base = b0 >> 1;
        bool carry = b0 & 1;
        for (int j0 = 0; j0 < avail && base < N; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = j < avail;
            const int c = valid ? win[mis + j] : ' ';
            const int pc = j > 0 ? win[mis + j - 1] : prev0;
            const PnmStep r = pnm_step(c, pc, valid, p1, carry, true, lane);
            const int64_t idx = base + __popcll(r.tok & ((1ull << lane) - 1));
            if (((r.tok >> lane) & 1) && idx < N) {
                int32_t v;
                if (p1) {
                    v = c == '0' ? 255 : 0;
                } else {
                    v = c - '0';
                    for (int q = j + 1;; ++q) {  // the token's other digits; it may run past the tile
                        const int e = q < wlen ? win[mis + q] : (tile0 + q < n ? d[tile0 + q] : ' ');
                        if (!pnm_is_digit(e)) break;
                        v = v * 10 + (e - '0');
                        if (v > 65535) v = 65536;
                    }
                    over |= v > H.maxval;
                }
                if (H.type == kPnmUshort) reinterpret_cast<uint16_t*>(o)[idx] = (uint16_t)v;
                else o[idx] = (uint8_t)v;
                if (idx == N - 1) dd.last_start = tile0 + j;
            }
            base += __popcll(r.tok);
            carry = pnm_carry_out(r, carry);
        }
    }
    if (over) atomicOr(&dd.oversize, 1);
}

__global__ void k_pnm_finish(int n, const PnmDesc* __restrict__ desc, int32_t* __restrict__ status,
                             int32_t* __restrict__ dims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PnmDesc& dd = desc[i];
    int32_t st = dd.status;
    if (st == kPnmPending) {
        // (with every sample there, last_start is set: an unset one reads as a failure of ours)
        const bool bad = dd.firstbad >= 0 && (dd.missing || dd.firstbad < dd.last_start);
        st = bad || dd.oversize ? kPnmBadData : dd.missing ? kPnmTruncated : dd.last_start >= 0 ? kPnmOk : -1;
    }
    const bool ok = st == kPnmOk;
    status[i] = st;
    dims[5 * i + 0] = ok ? dd.H.w : 0;
    dims[5 * i + 1] = ok ? dd.H.h : 0;
    dims[5 * i + 2] = ok ? dd.H.d : 0;
    dims[5 * i + 3] = ok ? dd.H.type : 0;
    dims[5 * i + 4] = ok ? dd.H.maxval : 0;
}

// ------------------------------------------------------------------- the streaming kernel
// Destination byte q of a segment from the segment's source bytes (ns of them).
template <int MODE>
__device__ __forceinline__ uint32_t pnm_byte_at(const uint8_t* seg, int q, int ns) {
    if (MODE == kPnmCopy) return seg[q];
    if (MODE == kPnmSwap16) return seg[q ^ 1];
    if (MODE == kPnmSwap32) return seg[q ^ 3];
    if (MODE == kPnmDrop8) {  // R,G,B,A -> R,G,B
        const int p = q / 3;
        return seg[q + p];
    }
    if (MODE == kPnmDrop16) {  // the same for 16-bit samples, low byte first -> high byte first
        const int e = q >> 1, p = e / 3;
        return seg[((e + p) << 1) | ((q & 1) ^ 1)];
    }
    if (MODE == kPnmUnpack) return (seg[q >> 3] >> (7 - (q & 7))) & 1 ? 0 : 255;
    uint32_t b = 0;  // kPnmPack: bit = 1 exactly where the pixel byte is 0; a row's last byte is padded with 0
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (8 * q + k < ns) b |= (uint32_t)(seg[8 * q + k] == 0) << (7 - k);
    return b;
}
constexpr int kPnmAux = kPnmSeg / 8 + 16;  // a segment's packed bytes

template <int MODE, int UO, int US>
__device__ __forceinline__ void pnm_stream_mode(const PnmStream& J, uint8_t* win) {
    constexpr int kUnits = kPnmSeg / (UO > US ? UO : US), kSegOut = kUnits * UO, kSegSrc = kUnits * US;
    const int tid = threadIdx.x;
    const int64_t nseg = (J.row_out + kSegOut - 1) / kSegOut, items = nseg * J.nrows;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t y = it / nseg, sg = it - y * nseg, sy = J.flip ? J.nrows - 1 - y : y;
        const int nb = (int)min<int64_t>(kSegOut, J.row_out - sg * kSegOut);
        const int ns = (int)min<int64_t>(kSegSrc, J.row_src - sg * kSegSrc);
        const int64_t s0 = J.src_off + sy * J.row_src + sg * kSegSrc;
        const int mis = (int)(reinterpret_cast<uintptr_t>(J.src + s0) & 15);
        __syncthreads();  // the previous segment's readers are done
        fill_window(win, J.src, J.src_size, s0 - mis, (mis + ns + 15) & ~15, tid, 256);
        __syncthreads();
        const uint8_t* seg = win + mis;
        constexpr int kOut = MODE == kPnmPack ? kPnmCopy : MODE;
        if (MODE == kPnmPack) {  // every thread packs its bytes first; they leave like a copy
            uint8_t* aux = win + kPnmSeg + 32;
            for (int q = tid; q < nb; q += 256) aux[q] = (uint8_t)pnm_byte_at<kPnmPack>(seg, q, ns);
            __syncthreads();
            seg = aux;
        }
        store_segment(J.dst + y * J.row_out + sg * kSegOut, nb, tid, [&](int q) { return pnm_byte_at<kOut>(seg, q, ns); });
    }
}

// win: kPnmSeg + 32 + kPnmAux bytes, 16-byte aligned. One workgroup takes every gridDim.x-th segment.
__device__ __forceinline__ void pnm_stream_rows(const PnmStream& J, uint8_t* win) {
    switch (J.mode) {
        case kPnmCopy: pnm_stream_mode<kPnmCopy, 1, 1>(J, win); break;
        case kPnmSwap16: pnm_stream_mode<kPnmSwap16, 2, 2>(J, win); break;
        case kPnmSwap32: pnm_stream_mode<kPnmSwap32, 4, 4>(J, win); break;
        case kPnmDrop8: pnm_stream_mode<kPnmDrop8, 3, 4>(J, win); break;
        case kPnmDrop16: pnm_stream_mode<kPnmDrop16, 6, 8>(J, win); break;
        case kPnmUnpack: pnm_stream_mode<kPnmUnpack, 8, 1>(J, win); break;
        default: pnm_stream_mode<kPnmPack, 1, 8>(J, win); break;
    }
}

// grid (x: segments, y: image)
__global__ __launch_bounds__(256) void k_pnm_stream(const PnmDesc* __restrict__ desc) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPnmSeg + 32 + kPnmAux];
    const PnmDesc& dd = desc[blockIdx.y];
    if (dd.status != kPnmOk || !dd.S.go) return;
    const PnmStream J = dd.S;
    pnm_stream_rows(J, win);
}

// ------------------------------------------------------------------------------- write
struct PnmwJob {
    PnmStream S;
    uint64_t total;  // the file's length
    int32_t status, hdr_len;
    uint8_t hdr[kPnmMaxHeader];
};

__global__ void k_pnmw_head(int n, const PnmwJob* __restrict__ jobs, uint8_t* __restrict__ out, uint64_t out_stride,
                            uint64_t* __restrict__ sizes, int32_t* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PnmwJob& J = jobs[i];
    sizes[i] = J.total;
    status[i] = J.status;
    if (J.status != kPnmOk) return;
    uint8_t* o = out + (uint64_t)i * out_stride;
    for (int k = 0; k < J.hdr_len; ++k) o[k] = J.hdr[k];
}

__global__ __launch_bounds__(256) void k_pnmw_stream(const PnmwJob* __restrict__ jobs) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPnmSeg + 32 + kPnmAux];
    const PnmwJob& W = jobs[blockIdx.y];
    if (W.status != kPnmOk || !W.S.go) return;
    const PnmStream J = W.S;
    pnm_stream_rows(J, win);
}

// ------------------------------------------------------------------------------- host
int pnm_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* type, int* maxval, int64_t* raster_at) {
    PnmHead H{};
    const int rc = pnm_check(data, size, &H);
    if (rc == kPnmOk) {
        *w = H.w;
        *h = H.h;
        *d = H.d;
        *type = H.type;
        *maxval = H.maxval;
        *raster_at = H.ascii ? H.rs : -1;
    }
    return rc;
}

int64_t pnm_default_tiles(int max_w, int max_h) {
    // text of up to 8 bytes per sample of the largest RGB image the workspace takes
    return ((int64_t)max_w * max_h * 3 * 8 + kPnmTile - 1) / kPnmTile + 1;
}

bool pnm_ws_alloc(PnmWs& ws, Blocks& mem, int max_images, int max_w, int max_h, int64_t tiles_cap) {
    ws.max_images = max_images;
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.tiles_cap = tiles_cap;
    const size_t n = (size_t)max_images, tiles = n * (size_t)tiles_cap;
    if (!mem.alloc(ws.desc, n * sizeof(PnmDesc))) return false;
    return tiles_cap == 0 || (mem.alloc(ws.summary, tiles * sizeof(int4)) && mem.alloc(ws.tbase, tiles * 8));
}

// blocks per image of a streaming launch: every segment once, at most about 16384 blocks in all
static int pnm_stream_blocks(int64_t max_bytes, int n) {
    const int64_t segs = std::max<int64_t>(1, (max_bytes + 1023) / 1024);
    return (int)std::max<int64_t>(1, std::min<int64_t>(segs, 16384 / std::min(n, 16384)));
}

void launch_pnm_decode(const PnmWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook) {
    if (n <= 0) return;
    const Stages S{hook, st};
    const int nb = (n + 63) / 64;
    // (few images: a workgroup per 4 tiles; many: each workgroup takes several groups in turn, so
    // that a batch without text files does not pay for a grid of empty workgroups)
    const unsigned tiles = (unsigned)std::min<int64_t>((ws.tiles_cap + 3) / 4, 16384 / std::min(n, 16384));
    S.begin(kStParse);
    hipLaunchKernelGGL(k_pnm_parse, dim3(nb), dim3(64), 0, st, n, d_data, d_off, d_size, ws.desc, d_out, out_stride, ws.max_w,
                       ws.max_h, ws.tiles_cap);
    S.end(kStParse);
    S.begin(kStUnstuff);  // locating the samples of text files
    if (tiles) {
        hipLaunchKernelGGL(k_pnm_tiles, dim3(tiles, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.summary,
                           ws.tiles_cap);
        hipLaunchKernelGGL(k_pnm_chain, dim3(n), dim3(256), 0, st, ws.desc, ws.summary, ws.tbase, ws.tiles_cap);
    }
    S.end(kStUnstuff);
    S.begin(kStEntropy);  // text -> samples
    if (tiles)
        hipLaunchKernelGGL(k_pnm_convert, dim3(tiles, n), dim3(256), 0, st, d_data, d_off, ws.desc, ws.tbase, d_out,
                           out_stride, ws.tiles_cap);
    S.end(kStEntropy);
    S.begin(kStConvert);  // binary rasters
    hipLaunchKernelGGL(k_pnm_stream, dim3(pnm_stream_blocks((int64_t)ws.max_w * ws.max_h * 12, n), n), dim3(256), 0, st, ws.desc);
    hipLaunchKernelGGL(k_pnm_finish, dim3(nb), dim3(64), 0, st, n, ws.desc, d_status, d_dims);
    S.end(kStConvert);
}

struct PnmwWs {
    Buf<PnmwJob> jobs;
};
PnmwWs* pnmw_ws_create() { return new PnmwWs(); }
void pnmw_ws_destroy(PnmwWs* w) { delete w; }

int pnm_encode_batch(hipStream_t st, PnmwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int type, int format, uint8_t* d_out, uint64_t out_stride,
                     uint64_t* d_sizes, int32_t* d_status, std::string& err) {
    std::vector<PnmwJob> jobs((size_t)n);
    int64_t max_bytes = 1;
    for (int i = 0; i < n; ++i) {
        PnmwJob& J = jobs[i];
        J = PnmwJob{};
        const int w = widths[i], h = heights[i];
        if (!d_src[i] || !pnm_write_args_ok(w, h, d, type, format)) {
            J.status = kPnmInvalidArgument;
            continue;
        }
        J.hdr_len = pnm_write_header(J.hdr, w, h, d, type, format);
        const int64_t payload = pnm_payload_bytes(w, h, d, type, format);
        J.total = (uint64_t)J.hdr_len + (uint64_t)payload;
        if (J.total > out_stride) {
            J.status = kPnmTooLarge;
            continue;
        }
        const int es = pnm_elem_bytes(type);
        PnmStream& S = J.S;
        S.src = d_src[i];
        S.src_size = (int64_t)w * h * d * es;
        S.dst = d_out + (uint64_t)i * out_stride + J.hdr_len;
        S.go = 1;
        if (format == kPnmP4) {
            S.mode = kPnmPack;
            S.nrows = h;
            S.row_out = (w + 7) / 8;
            S.row_src = w;
        } else if (format == kPnmPF) {
            S.mode = kPnmCopy;
            S.nrows = h;
            S.flip = 1;
            S.row_out = S.row_src = (int64_t)w * d * 4;
        } else {
            S.mode = d == 4 ? (es == 2 ? kPnmDrop16 : kPnmDrop8) : (es == 2 ? kPnmSwap16 : kPnmCopy);
            S.nrows = 1;
            S.row_out = payload;
            S.row_src = S.src_size;
        }
        max_bytes = std::max(max_bytes, std::max(payload, S.src_size));
    }
    if (jobs_upload("pnm_encode_batch", ws.jobs, jobs, st, err)) return -1;
    hipLaunchKernelGGL(k_pnmw_head, dim3((n + 63) / 64), dim3(64), 0, st, n, ws.jobs.p, d_out, out_stride, d_sizes, d_status);
    hipLaunchKernelGGL(k_pnmw_stream, dim3(pnm_stream_blocks(max_bytes, n), n), dim3(256), 0, st, ws.jobs.p);
    return encode_finish("pnm_encode_batch", st, err);
}

}  // namespace icx
