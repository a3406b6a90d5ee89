// icx_tiffw.hip -- TIFF write on the MI355X: Image::writeTiff (codecs.cpp:1485-1513, libtiff with
// one Deflate strip) as strips of uncompressed, PackBits, LZW or Deflate data. Contract:
// include/icx.h "TIFF write"; the serial part and the bound: icx_tiffw_core.h. All strips of all
// images of a call go through each kernel in one launch.
//
//   none      k_tiffw_layout, k_tiffw_gather: every offset is known in advance, the gather copies
//             the pixel rows straight into the file
//   PackBits  k_tiffw_pb<false> one wave per row: packet sizes; k_tiffw_pb_scan: the rows' offsets
//             in their strip; k_tiffw_pb<true>: the packets
//   LZW       k_tiffw_lzw one wave per strip: greedy LZW is a serial chain per input byte, the
//             parallelism is the number of strips
//   Deflate   k_tiffw_pack, k_tiffw_lz77, k_tiffw_huff, k_tiffw_scan, k_tiffw_emit: the stages of
//             icx_exrw.hip over TIFF's view (distances 1, d, the row above; the segment hash), the
//             back end shared with it and icx_png.hip (icx_deflate_core.h, icx_deflate_wave.h)
//   all       k_tiffw_layout one workgroup per image: strip sizes -> offsets, the file's size,
//             TOO_LARGE, header, arrays and IFD; k_tiffw_gather: each payload to its place
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "icx_deflate_wave.h"
#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_tiffw_core.h"
#include "icx_wave.h"

namespace icx {

namespace tiffw {

using namespace deflate;

constexpr int kSeg = kTiffwSeg, kSlots = kSeg;  // (blocks of at most kTiffwBlockSegs segments: tiffw_deflate_blocks)
constexpr int kInternal = -1;
static_assert(kTiffwHdrBytes == kHdrWords * 4, "the bound's block header room is the header buffer");

struct Img {
    const uint8_t* src;
    uint8_t* out;
    TiffwGeom g;
    int32_t status;
    int32_t strip0;
    int64_t row0;  // its rows in the row-size table (PackBits)
};
struct Strip {
    int32_t img, y0, rows;
    uint32_t S;       // raw bytes
    int64_t at;       // its room in the payload (and predictor-byte) workspace, 16-byte aligned
    uint32_t room;    // payload bytes the room holds (the bound)
    int32_t seg0, nseg;  // deflate segments
    // written on the device
    uint32_t size;    // payload bytes
    uint32_t file_at;
    uint32_t adler;
};
struct Block {
    int32_t strip;
    int32_t seg0, nseg;
    int32_t last;
};

// ---------------------------------------------------------------------------- PackBits
// One wave per row, kPbTile positions per step, position p under lane p - p0; p == n is a virtual
// packet start that closes the row's last packet. Per position: the start of its run (a max scan
// of run starts, carried over tiles), from that its 128-byte piece and whether the piece is a
// repeat packet (3 or more: the two bytes after a piece's start decide it); literal stretches
// start after a repeat piece (a max scan again) and are cut every 128 bytes. A sum scan of the
// bytes each position adds gives its place in the output. A packet's header is written by the
// position that starts the next packet, which knows the length: the latest start before it, its
// output offset and its kind come from exclusive max scans.
// Five wave scans per tile instead of ballots: the cuts need the latest start *position*, which a
// ballot's mask gives only inside one tile, and the scans carry it across tiles as they are.
constexpr int kPbTile = 64;

__device__ __forceinline__ long long wave_max_scan64(long long v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long t = __shfl_up(v, s);
        if (lane >= s) v = max(v, t);
    }
    return v;
}

// grid (x: rows by turns of 4 waves, y: image)
template <bool STORE>
__global__ __launch_bounds__(256) void k_tiffw_pb(const Img* __restrict__ imgs, const Strip* __restrict__ strips,
                                                  uint32_t* __restrict__ rowsz, uint8_t* __restrict__ Z) {
    const Img& I = imgs[blockIdx.y];
    if (I.status != kTiffOk) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = I.g.rb;
    for (int r = blockIdx.x * 4 + wave; r < I.g.h; r += gridDim.x * 4) {  // (wave-uniform)
        const uint8_t* row = I.src + (int64_t)r * n;
        uint8_t* out = nullptr;
        if (STORE) out = Z + strips[I.strip0 + r / I.g.rps].at + rowsz[I.row0 + r];
        auto b = [&](int64_t q) -> int { return q >= 0 && q < n ? (int)row[q] : -1; };
        long long c_rs = -1, c_ls = -1, c_q = -1, c_ok = -1;  // carries: run start, stretch start, latest start, its offset * 2 + kind
        int c_rep = 0;                                        // the previous position was in a repeat piece
        unsigned long long c_o = 0;                           // output bytes before this tile
        for (int64_t p0 = 0; p0 <= n; p0 += kPbTile) {
            const int64_t p = p0 + lane;
            const bool live = p < n;
            // (the four loads hit the same cache lines; taking the neighbours' bytes by shuffles
            // instead measured 15.9 ms against 14.6 ms on 256 x 1024^2 RGB)
            const int v = b(p), vp = b(p - 1), v1 = b(p + 1), v2 = b(p + 2);
            const bool runstart = live && v != vp;
            const long long rs = max(c_rs, wave_max_scan64(runstart ? p : -1, lane));
            const int64_t inpiece = (p - rs) & 127;
            bool rep = false;
            if (live) rep = inpiece >= 2 || (inpiece == 1 ? v1 == v : (v1 == v && v2 == v));
            int prevrep = __shfl_up((int)rep, 1);
            if (lane == 0) prevrep = c_rep;
            const bool lit = live && !rep;
            const bool litstart = lit && (p == 0 || prevrep);
            const long long ls = max(c_ls, wave_max_scan64(litstart ? p : -1, lane));
            const bool start = p == n || (rep && inpiece == 0) || (lit && ((p - ls) & 127) == 0);
            const uint32_t add = !live ? 0u : rep ? (start ? 2u : 0u) : (start ? 2u : 1u);
            const uint32_t inc = wave_sum_scan(add, lane);
            const unsigned long long o = c_o + inc - add;
            // the latest start before p, its offset and kind
            const long long sq = wave_max_scan64(start && p <= n ? p : -1, lane);
            const long long sok = wave_max_scan64(start && live ? (long long)(o << 1 | (rep ? 1u : 0u)) : -1, lane);
            long long q = __shfl_up(sq, 1), ok = __shfl_up(sok, 1);
            if (lane == 0) { q = -1; ok = -1; }
            q = max(q, c_q);
            ok = max(ok, c_ok);
            if (STORE) {
                if (lit || (rep && start)) out[o + (start ? 1 : 0)] = (uint8_t)v;  // (a repeat piece's later bytes: nothing)
                if (start && p <= n && q >= 0) {
                    const int len = (int)(p - q);
                    out[ok >> 1] = (uint8_t)((ok & 1) ? 257 - len : len - 1);
                }
            }
            c_rs = __shfl(rs, 63);
            c_ls = __shfl(ls, 63);
            c_rep = __shfl((int)rep, 63);
            c_q = max(c_q, (long long)__shfl(sq, 63));
            c_ok = max(c_ok, (long long)__shfl(sok, 63));
            c_o += __shfl(inc, 63);
        }
        if (!STORE && lane == 0) rowsz[I.row0 + r] = (uint32_t)c_o;
    }
}

// One thread per strip: its rows' sizes into offsets, the strip's size.
__global__ void k_tiffw_pb_scan(const Img* __restrict__ imgs, Strip* __restrict__ strips, int64_t nstrips,
                                uint32_t* __restrict__ rowsz) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nstrips) return;
    Strip& s = strips[k];
    const Img& I = imgs[s.img];
    uint32_t run = 0;
    for (int r = 0; r < s.rows; ++r) {
        uint32_t& z = rowsz[I.row0 + s.y0 + r];
        const uint32_t v = z;
        z = run;
        run += v;
    }
    s.size = run;
}

// -------------------------------------------------------------------------------- LZW
// One wave per strip. The dictionary (icx_tiffw_core.h: 8192 words) is in LDS. Greedy LZW is a
// serial chain per input byte; every lane runs the same chain over the same bytes, so its state is
// wave-uniform, and lane 0 alone stores into the dictionary and the code list (a wave's LDS
// operations complete in order, so every lane's later probe sees them). The chain only appends
// (code, width) to an LDS list. Everything else is done by all lanes: staging kLzwIn input bytes
// (the predictor's gather from the pixels), freeing the dictionary after a Clear, and after each
// staged tile placing the codes -- a wave sum scan of the widths gives each code its bit, the lanes
// OR them MSB-first into an LDS image of the stream's words, whole bytes leave with one store per
// lane and the last partial byte is carried into the next tile's image.
// LDS: 32768 (dictionary) + 1024 (input) + 2064 (codes) + 2048 (words) = 37904 bytes per wave.
constexpr int kLzwIn = 1024;
constexpr int kLzwCodes = kLzwIn + 8;  // a tile's codes: one per byte at most, the leading Clear, a forced Clear, the last code, EOI
constexpr int kLzwWords = 512;         // 7 carried bits + kLzwCodes * 12 bits: under 388 words
__global__ __launch_bounds__(64) void k_tiffw_lzw(const Img* __restrict__ imgs, Strip* __restrict__ strips,
                                                  uint8_t* __restrict__ Z) {
    __shared__ uint32_t dict[kTiffwLzwSlots];
    __shared__ uint32_t wbuf[kLzwWords];
    __shared__ uint16_t cbuf[kLzwCodes];  // code | (width - 9) << 12
    __shared__ uint8_t ibuf[kLzwIn];
    Strip& s = strips[blockIdx.x];
    const Img& I = imgs[s.img];
    if (I.status != kTiffOk) return;
    const TiffwGeom g = I.g;
    const int lane = threadIdx.x;
    uint8_t* dst = Z + s.at;
    const uint32_t S = s.S, room = s.room;
    for (int i = lane; i < kTiffwLzwSlots; i += 64) dict[i] = kTiffwLzwFree;
    for (int i = lane; i < kLzwWords; i += 64) wbuf[i] = 0;
    wave_sync();
    int nc = 0;             // codes in cbuf
    uint32_t bits = 0;      // bits of wbuf in use (< 8 between tiles: the carried partial byte)
    uint32_t written = 0;   // bytes of the stream already in dst
    auto sink = [&](uint32_t code, int width) {
        if (lane == 0) cbuf[nc] = (uint16_t)(code | (uint32_t)(width - 9) << 12);
        ++nc;
    };
    auto pack = [&](bool last) {  // the tile's codes into wbuf, its whole bytes out
        wave_sync();
        for (int i0 = 0; i0 < nc; i0 += 64) {
            const int i = i0 + lane;
            uint32_t code = 0, w = 0;
            if (i < nc) {
                const uint32_t e = cbuf[i];
                code = e & 0xFFFu;
                w = 9 + (e >> 12);
            }
            const uint32_t inc = wave_sum_scan(w, lane);
            if (w) {
                const uint32_t pos = bits + inc - w, wi = pos >> 5, end = (pos & 31) + w;  // bits [pos & 31, end) from the word's top
                if (end <= 32) {
                    atomicOr(&wbuf[wi], code << (32 - end));
                } else {
                    atomicOr(&wbuf[wi], code >> (end - 32));
                    atomicOr(&wbuf[wi + 1], code << (64 - end));
                }
            }
            bits += __shfl(inc, 63);
        }
        wave_sync();
        const uint32_t nbytes = last ? (bits + 7) >> 3 : bits >> 3, nwords = (bits + 31) >> 5;
        for (uint32_t k = lane; k < nbytes; k += 64)
            if (written + k < room) dst[written + k] = (uint8_t)(wbuf[k >> 2] >> (24 - 8 * (k & 3)));
        const uint32_t rem = last ? 0u : bits & 7u;
        const uint32_t carry = rem ? ((wbuf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) << 24 : 0u;
        wave_sync();
        for (uint32_t k = lane; k < nwords; k += 64) wbuf[k] = k == 0 ? carry : 0u;
        wave_sync();
        written += nbytes;
        bits = rem;
        nc = 0;
    };
    TiffwLzw z;
    z.begin(sink);
    for (uint32_t i0 = 0; i0 < S; i0 += kLzwIn) {
        const int cnt = (int)min((uint32_t)kLzwIn, S - i0);
        for (int k = lane; k < cnt; k += 64) ibuf[k] = (uint8_t)tiffw_strip_byte(I.src, g, s.y0, i0 + k);
        wave_sync();
        for (int k = 0; k < cnt; ++k) {
            const uint32_t byte = ibuf[k];
            if (z.feed(dict, byte, sink, lane == 0)) {  // (wave-uniform)
                wave_sync();
                for (int i = lane; i < kTiffwLzwSlots; i += 64) dict[i] = kTiffwLzwFree;
                wave_sync();
            }
        }
        const bool last = i0 + kLzwIn >= S;
        if (last) z.finish(sink);
        pack(last);
    }
    if (lane == 0) s.size = written;
}

// ------------------------------------------------------------------------------ Deflate
// Thread t of a segment's workgroup: 16 consecutive strip bytes, one 16-byte store (bytes past S
// are 0), and the segment's Adler-32 partials: sum b, sum (S - t) b.
__global__ __launch_bounds__(256) void k_tiffw_pack(const Img* __restrict__ imgs, const Strip* __restrict__ strips,
                                                    const int32_t* __restrict__ seg_strip, uint8_t* __restrict__ P,
                                                    uint32_t* __restrict__ adl) {
    __shared__ unsigned long long s_a[4], s_b[4];
    const int64_t seg = blockIdx.x;
    const Strip& c = strips[seg_strip[seg]];
    const Img& I = imgs[c.img];
    const TiffwGeom g = I.g;
    const uint32_t S = c.S, t0 = (uint32_t)(seg - c.seg0) * kSeg + threadIdx.x * 16u;
    unsigned long long a1 = 0, a2 = 0;
    if (t0 < ((S + 15u) & ~15u)) {
        uint8_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t t = t0 + j;
            uint32_t b = 0;
            if (t < S) {
                b = tiffw_strip_byte(I.src, g, c.y0, t);
                a1 += b;
                a2 += (unsigned long long)(S - t) * b;
            }
            v[j] = (uint8_t)b;
        }
        uint4 q;
        __builtin_memcpy(&q, v, 16);
        *reinterpret_cast<uint4*>(P + c.at + t0) = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a1 += __shfl_xor(a1, o);
        a2 += __shfl_xor(a2, o);
    }
    if ((threadIdx.x & 63) == 0) {
        s_a[threadIdx.x >> 6] = a1;
        s_b[threadIdx.x >> 6] = a2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        adl[2 * seg] = (uint32_t)((s_a[0] + s_a[1] + s_a[2] + s_a[3]) % kAdlerMod);
        adl[2 * seg + 1] = (uint32_t)((s_b[0] % kAdlerMod + s_b[1] % kAdlerMod + s_b[2] % kAdlerMod + s_b[3] % kAdlerMod) % kAdlerMod);
    }
}

// A wave's views of the strip's bytes in LDS: view 0 the segment and the 16 bytes before it
// (distances 1 and d), view 1 the same bytes one row back. Matches end at the segment's end.
constexpr int kNear = 16;
constexpr int kView = kSeg + 48;
struct View {
    const uint8_t* p;
    int64_t b0;
    __device__ __forceinline__ uint32_t dword(int64_t i) const {
        const int64_t o = i - b0;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p) + (o >> 2);
        return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(o & 3));
    }
};
__device__ __forceinline__ int match_len(const View& A, const View& B, int64_t p, int64_t dist, int maxlen) {
    int l = 0;
    while (l < maxlen) {
        const uint32_t x = A.dword(p + l) ^ B.dword(p - dist + l);
        if (x) return min(l + (int)(__builtin_ctz(x) >> 3), maxlen);
        l += 4;
    }
    return maxlen;
}

// Two waves per workgroup, a segment each; the window walk, the hash and the lazy parse are
// k_exrw_lz77's, the candidates TIFF's: the byte before, the pixel before, the row above.
constexpr int kLzWaves = 2;
constexpr int kHashBits = 11;
__global__ __launch_bounds__(64 * kLzWaves) void k_tiffw_lz77(const Img* __restrict__ imgs, const Strip* __restrict__ strips,
                                                              const int32_t* __restrict__ seg_strip, int64_t nseg,
                                                              const uint8_t* __restrict__ P, uint16_t* __restrict__ tok,
                                                              uint32_t* __restrict__ ntok, uint16_t* __restrict__ seghist,
                                                              uint32_t* __restrict__ segx) {
    __shared__ uint32_t s_h[kLzWaves][kNLL + kND];
    __shared__ uint32_t s_hash[kLzWaves][1 << kHashBits];
    __shared__ __attribute__((aligned(16))) uint8_t views[kLzWaves][2][kView];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * kLzWaves + wave;
    if (seg >= nseg) return;  // wave-uniform; no block barriers below
    const Strip& c = strips[seg_strip[seg]];
    const TiffwGeom g = imgs[c.img].g;
    const uint8_t* F = P + c.at;
    const int64_t N = c.S;
    const int64_t s0 = (seg - c.seg0) * kSeg, s1 = min(N, s0 + kSeg);
    int64_t cand[3] = {1, g.d, g.rb};
    if (cand[1] == 1) cand[1] = 0;
    if (cand[2] <= g.d || cand[2] > 32768) cand[2] = 0;
    View V[2];
    V[0].b0 = (s0 - kNear) & ~(int64_t)15;
    V[1].b0 = (s0 - cand[2]) & ~(int64_t)15;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        V[k].p = views[wave][k];
        stage_view(F, N, V[k].b0, views[wave][k], lane, kView);
    }
    uint32_t* SH = s_h[wave];
    for (int i = lane; i < kNLL + kND; i += 64) SH[i] = 0;
    uint32_t* HT = s_hash[wave];
    for (int i = lane; i < (1 << kHashBits); i += 64) HT[i] = 0;
    __builtin_amdgcn_wave_barrier();
    uint16_t* T = tok + seg * kSlots;
    uint32_t xbits = 0;
    uint32_t nt = 0, nm = 0;
    int64_t pos = s0;
    for (int64_t p0 = s0; p0 < s1; p0 += 64) {
        const int64_t q = p0 + lane;
        int best = 0, bd = 0;
        uint32_t lit = 0, hslot = 0, hprev = 0;
        const bool hashed = q + 4 <= s1;
        if (hashed) {
            hslot = (V[0].dword(q) * 2654435761u) >> (32 - kHashBits);
            hprev = HT[hslot];
        }
        __builtin_amdgcn_wave_barrier();
        if (hashed) atomicMax(&HT[hslot], (uint32_t)(q - s0) + 1u);
        if (q < s1) {
            const uint32_t t4 = V[0].dword(q);
            lit = t4 & 255u;
            const int maxlen = (int)min((int64_t)258, s1 - q);
            if (maxlen >= 4 && q >= pos && hprev) {
                const int64_t dd = q - (s0 + (int64_t)hprev - 1);
                if (V[0].dword(q - dd) == t4) {
                    best = 4 + match_len(V[0], V[0], q + 4, dd, maxlen - 4);
                    bd = (int)dd;
                }
            }
            if (maxlen >= 3 && q >= pos) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int64_t dd = cand[k];
                    if (dd == 0 || dd > q) continue;
                    const View& B = V[k < 2 ? 0 : 1];
                    if (((B.dword(q - dd) ^ t4) & 0xFFFFFFu) != 0) continue;
                    const int l = 3 + match_len(V[0], B, q + 3, dd, maxlen - 3);
                    if (l < (dd > 4096 ? 5 : dd > 2 ? 4 : 3)) continue;  // zlib's TOO_FAR
                    if (l > best || (l == best && dd < bd)) {
                        best = l;
                        bd = (int)dd;
                    }
                }
            }
        }
        parse_window(best, bd, lit, lane, p0, s1, T, SH, nt, nm, pos, xbits);
    }
    if (lane == 0) {
        ntok[seg] = nt;
        segx[seg] = xbits;
    }
    __builtin_amdgcn_wave_barrier();
    uint16_t* G = seghist + seg * (kNLL + kND);
    for (int i = lane; i < kNLL + kND; i += 64) G[i] = (uint16_t)SH[i];
}

// One workgroup per deflate block: codes, the dynamic header, bits per segment. The sequence of
// k_exrw_huff (icx_deflate_core.h says why each writer keeps its own text of it); a block has at
// most 65536 tokens, so the counts need no scaling.
__global__ __launch_bounds__(64) void k_tiffw_huff(const Block* __restrict__ blocks, const uint16_t* __restrict__ seghist,
                                                   const uint32_t* __restrict__ segx, BlockCodes* __restrict__ bc,
                                                   unsigned long long* __restrict__ off) {
    __shared__ uint32_t f_ll[kNLL], f_d[kND];
    __shared__ uint16_t order[kNLL], order_d[kND];
    __shared__ uint32_t wt[2 * kNLL];
    __shared__ int16_t parent[2 * kNLL];
    __shared__ uint8_t l_ll[kNLL], l_d[kND];
    __shared__ uint8_t rle_sym[kNLL + kND];
    __shared__ uint8_t rle_ext[kNLL + kND];
    __shared__ uint32_t s_hdr_bits;
    const Block& K = blocks[blockIdx.x];
    const int64_t seg0 = K.seg0, ns = K.nseg;
    for (int i = threadIdx.x; i < kNLL + kND; i += 64) {
        uint32_t f = 0;
        for (int64_t s = 0; s < ns; ++s) f += seghist[(seg0 + s) * (kNLL + kND) + i];
        if (i == 256) f += 1;  // EOB
        if (i < kNLL) f_ll[i] = f;
        else f_d[i - kNLL] = f;
    }
    BlockCodes& B = bc[blockIdx.x];
    for (int i = threadIdx.x; i < kHdrWords; i += 64) B.hdr[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) pad_block_counts(f_ll, f_d);
    __syncthreads();
    rank_order(f_ll, kNLL, order);
    rank_order(f_d, kND, order_d);
    __syncthreads();
    if (threadIdx.x == 0) {
        huff_lengths(f_ll, kNLL, 15, l_ll, order, wt, parent, true);
        huff_lengths(f_d, kND, 15, l_d, order_d, wt, parent, true);
        canon_codes(l_ll, kNLL, B.ll_code);
        canon_codes(l_d, kND, B.d_code);
        for (int i = 0; i < kNLL; ++i) B.ll_len[i] = l_ll[i];
        for (int i = 0; i < kND; ++i) B.d_len[i] = l_d[i];
        int hlit = kNLL;
        while (hlit > 257 && l_ll[hlit - 1] == 0) --hlit;
        int hdist = kND;
        while (hdist > 1 && l_d[hdist - 1] == 0) --hdist;
        // run-length code the concatenated lengths (16: repeat 3-6, 17: zeros 3-10, 18: zeros 11-138)
        int nsym = 0;
        const int tot = hlit + hdist;
        auto L = [&](int i) { return i < hlit ? l_ll[i] : l_d[i - hlit]; };
        for (int i = 0; i < tot;) {
            const int cur = L(i);
            int run = 1;
            while (i + run < tot && L(i + run) == cur) ++run;
            int left = run;
            if (cur == 0) {
                while (left >= 11) {
                    const int r = min(left, 138);
                    rle_sym[nsym] = 18;
                    rle_ext[nsym++] = (uint8_t)(r - 11);
                    left -= r;
                }
                if (left >= 3) {
                    rle_sym[nsym] = 17;
                    rle_ext[nsym++] = (uint8_t)(left - 3);
                    left = 0;
                }
                while (left > 0) {
                    rle_sym[nsym] = 0;
                    rle_ext[nsym++] = 0;
                    --left;
                }
            } else {
                rle_sym[nsym] = (uint8_t)cur;
                rle_ext[nsym++] = 0;
                --left;
                while (left >= 3) {
                    const int r = min(left, 6);
                    rle_sym[nsym] = 16;
                    rle_ext[nsym++] = (uint8_t)(r - 3);
                    left -= r;
                }
                while (left > 0) {
                    rle_sym[nsym] = (uint8_t)cur;
                    rle_ext[nsym++] = 0;
                    --left;
                }
            }
            i += run;
        }
        uint32_t f_cl[19];
        for (int i = 0; i < 19; ++i) f_cl[i] = 0;
        for (int i = 0; i < nsym; ++i) ++f_cl[rle_sym[i]];
        {
            int u = 0;
            for (int i = 0; i < 19; ++i) u += f_cl[i] != 0;
            if (u < 2) {
                if (!f_cl[0]) f_cl[0] = 1;
                else f_cl[1] = 1;
            }
        }
        uint8_t l_cl[19];
        uint16_t c_cl[19];
        huff_lengths(f_cl, 19, 7, l_cl, order, wt, parent, false);
        canon_codes(l_cl, 19, c_cl);
        int hclen = 19;
        while (hclen > 4 && l_cl[kClOrder[hclen - 1]] == 0) --hclen;
        BitW bw{B.hdr};
        bw.put(K.last ? 1u : 0u, 1);  // BFINAL
        bw.put(2u, 2);                // BTYPE = dynamic
        bw.put((uint32_t)(hlit - 257), 5);
        bw.put((uint32_t)(hdist - 1), 5);
        bw.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) bw.put(l_cl[kClOrder[i]], 3);
        for (int i = 0; i < nsym; ++i) {
            const int s = rle_sym[i];
            bw.put(c_cl[s], l_cl[s]);
            if (s == 16) bw.put(rle_ext[i], 2);
            else if (s == 17) bw.put(rle_ext[i], 3);
            else if (s == 18) bw.put(rle_ext[i], 7);
        }
        B.hdr_bits = bw.n;
        s_hdr_bits = bw.n;
    }
    __syncthreads();
    for (int64_t s = threadIdx.x; s < ns; s += 64) {
        const uint16_t* G = seghist + (seg0 + s) * (kNLL + kND);
        unsigned long long b = segx[seg0 + s];
        for (int i = 0; i < kNLL; ++i) b += (uint32_t)G[i] * l_ll[i];
        for (int i = 0; i < kND; ++i) b += (uint32_t)G[kNLL + i] * l_d[i];
        if (s == 0) b += s_hdr_bits;
        if (s == ns - 1) b += l_ll[256];  // EOB
        off[seg0 + s] = b;
    }
}

// One thread per strip: the segments' bits into bit offsets within the stream, the stream's size
// and Adler-32. A stream longer than its room (the bound failed) fails the image.
__global__ void k_tiffw_scan(Img* __restrict__ imgs, Strip* __restrict__ strips, int64_t nstrips,
                             const uint32_t* __restrict__ adl, unsigned long long* __restrict__ off) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nstrips) return;
    Strip& c = strips[k];
    const int64_t seg0 = c.seg0, ns = c.nseg;
    unsigned long long run = 0, a = 0, b = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const unsigned long long v = off[seg0 + s];
        off[seg0 + s] = run;
        run += v;
        a += adl[2 * (seg0 + s)];
        b += adl[2 * (seg0 + s) + 1];
    }
    const unsigned long long z = 2 + (run + 7) / 8 + 4;
    const uint32_t A = (uint32_t)((1 + a) % kAdlerMod), Bs = (uint32_t)((c.S + b) % kAdlerMod);
    c.adler = Bs << 16 | A;
    if (z > c.room) {
        c.size = 0;
        atomicExch(&imgs[c.img].status, kInternal);
    } else {
        c.size = (uint32_t)z;
    }
}

// One wave per segment: its bits at their offset in the strip's stream, two bytes into the
// strip's room (the zlib header comes first); OR into the zeroed room, so that segments sharing a
// word need no order.
constexpr int kEmitWords = 2048;
__global__ __launch_bounds__(256) void k_tiffw_emit(const Img* __restrict__ imgs, const Strip* __restrict__ strips,
                                                    const int32_t* __restrict__ seg_strip,
                                                    const int32_t* __restrict__ seg_block,
                                                    const Block* __restrict__ blocks, int64_t nseg,
                                                    const uint16_t* __restrict__ tok, const uint32_t* __restrict__ ntok,
                                                    const BlockCodes* __restrict__ bc,
                                                    const unsigned long long* __restrict__ off, uint8_t* __restrict__ Z) {
    __shared__ uint32_t img[4][kEmitWords];
    __shared__ BlockCodes Bs[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * 4 + wave;
    if (seg >= nseg) return;  // wave-uniform; no block barriers below
    const Strip& c = strips[seg_strip[seg]];
    if (imgs[c.img].status != kTiffOk || c.size == 0) return;
    BlockCodes& B = Bs[wave];
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bc + seg_block[seg]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&B);
        for (int i = lane; i < (int)(sizeof(BlockCodes) / 4); i += 64) dst[i] = src[i];
    }
    __builtin_amdgcn_wave_barrier();
    const Block& K = blocks[seg_block[seg]];
    const bool head = seg == K.seg0, eob = seg == (int64_t)K.seg0 + K.nseg - 1;
    // (bit 16 of the room is the stream's first: the two zlib header bytes are in front)
    const unsigned long long o0 = 16 + off[seg];
    const unsigned long long o1 =
        seg - c.seg0 == c.nseg - 1 ? 16 + (unsigned long long)(c.size - 6) * 8ull : 16 + off[seg + 1];
    if (o1 <= o0) return;
    uint32_t* out = reinterpret_cast<uint32_t*>(Z + c.at);
    const unsigned long long w0 = o0 >> 5, wl = (o1 - 1) >> 5;
    const int nw = (int)min((unsigned long long)kEmitWords + 1, wl - w0 + 1);
    const uint16_t* T = tok + seg * kSlots;
    if (nw > kEmitWords) {
        emit_segment(out + w0, o0 & 31, B, nullptr, 0, T, ntok[seg], head, eob, lane);
        return;
    }
    uint32_t* W = img[wave];
    for (int i = lane; i < nw; i += 64) W[i] = 0;
    __builtin_amdgcn_wave_barrier();
    emit_segment(W, o0 & 31, B, nullptr, 0, T, ntok[seg], head, eob, lane);
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < nw; i += 64) {
        const uint32_t v = W[i];
        if (i == 0 || i == nw - 1) atomicOr(out + w0 + i, v);
        else out[w0 + i] = v;
    }
}

// ------------------------------------------------------------------------------- layout
// One workgroup per image: thread 0 walks the strips' sizes into even file offsets; when the file
// fits its slot the workgroup writes the header, the arrays and the IFD, as byte stores (the slot
// may start at any address). Otherwise nothing is written and the image is TOO_LARGE.
__global__ __launch_bounds__(256) void k_tiffw_layout(Img* __restrict__ imgs, Strip* __restrict__ strips, int comp,
                                                      uint64_t out_stride, uint64_t* __restrict__ sizes,
                                                      int32_t* __restrict__ status) {
    __shared__ uint8_t s_ifd[kTiffwIfdMax];
    __shared__ TiffwLayout s_L;
    __shared__ int s_len, s_st;
    Img& I = imgs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_st = I.status;
        if (s_st == kTiffOk) {
            const TiffwGeom g = I.g;
            Strip* C = strips + I.strip0;
            uint64_t at = 8;
            for (int k = 0; k < g.nstrips; ++k) {
                if (comp == kTiffwNone) C[k].size = C[k].S;
                C[k].file_at = (uint32_t)at;
                at += ((uint64_t)C[k].size + 1) & ~1ull;
            }
            s_L = tiffw_layout(g, at);
            if (s_L.total > out_stride) s_st = kTiffTooLarge;
            else s_len = tiffw_ifd(s_ifd, g, s_L, C[0].file_at, C[0].size);
        }
        sizes[blockIdx.x] = s_st == kTiffOk || s_st == kTiffTooLarge ? s_L.total : 0;
        status[blockIdx.x] = s_st;
    }
    __syncthreads();
    if (s_st != kTiffOk) {
        __syncthreads();
        if (tid == 0) I.status = s_st;  // k_tiffw_gather skips it
        return;
    }
    const TiffwGeom g = I.g;
    const TiffwLayout L = s_L;
    const Strip* C = strips + I.strip0;
    uint8_t* o = I.out;
    if (tid < 8) {
        uint8_t h[8];
        tiffw_header(h, L);
        o[tid] = h[tid];
    }
    if (g.d >= 3 && tid < 2 * g.d) o[L.bps_at + tid] = (tid & 1) ? 0 : 8;
    if (g.nstrips > 1)
        for (int b = tid; b < 4 * g.nstrips; b += 256) {
            o[L.so_at + b] = (uint8_t)(C[b >> 2].file_at >> (8 * (b & 3)));
            o[L.sc_at + b] = (uint8_t)(C[b >> 2].size >> (8 * (b & 3)));
        }
    for (int b = tid; b < s_len; b += 256) o[L.ifd_at + b] = s_ifd[b];
}

// One workgroup per strip: its payload to file_at (16-byte stores where the destination is
// aligned), and the zero byte after an odd one. Uncompressed strips come straight from the pixels;
// a Deflate payload gets its two header bytes and the Adler-32 here.
__global__ __launch_bounds__(256) void k_tiffw_gather(const Img* __restrict__ imgs, const Strip* __restrict__ strips,
                                                      int comp, const uint8_t* __restrict__ Z) {
    const Strip& c = strips[blockIdx.x];
    const Img& I = imgs[c.img];
    if (I.status != kTiffOk) return;
    const uint32_t n = c.size;
    const uint8_t* src = comp == kTiffwNone ? I.src + (int64_t)c.y0 * I.g.rb : Z + c.at;
    uint8_t* dst = I.out + c.file_at;
    const uint32_t adler = c.adler;
    const bool zl = comp == kTiffwDeflate;
    auto byte_at = [&](int q) -> uint32_t {
        const uint32_t i = (uint32_t)q;
        if (i >= n) return 0;  // the pad byte
        if (zl) {
            if (i < 2) return i == 0 ? 0x78u : 0x01u;
            if (i >= n - 4) return (adler >> (8 * (n - 1 - i))) & 255u;
        }
        return src[i];
    };
    const uint32_t total = n + (n & 1);
    for (uint32_t i0 = 0; i0 < total; i0 += 1u << 20) {
        const int nb = (int)min(1u << 20, total - i0);
        store_segment(dst + i0, nb, threadIdx.x, [&](int q) { return byte_at((int)i0 + q); });
    }
}

}  // namespace tiffw

// Grow-only device buffers of one context's TIFF writes (icx_ctx::tiffw).
struct TiffwWs {
    Buf<uint8_t> tables, pred, payload, tok, hist;
};
TiffwWs* tiffw_ws_create() { return new TiffwWs(); }
void tiffw_ws_destroy(TiffwWs* w) { delete w; }

int tiffw_encode_batch(hipStream_t st, TiffwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                       const int32_t* heights, int d, int comp, int pred, int rows_per_strip, uint8_t* d_out,
                       uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, std::string& err) {
    using namespace tiffw;
    const char* name = "icx_tiff_encode_device_batch";
    std::vector<Img> imgs((size_t)n);
    std::vector<Strip> strips;
    std::vector<Block> blocks;
    std::vector<int32_t> seg_strip, seg_block;
    int64_t at = 0, rows = 0;
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        Img& I = imgs[i];
        I = Img{};
        I.src = d_src[i];
        I.out = d_out + (uint64_t)i * out_stride;
        I.strip0 = (int32_t)strips.size();
        I.row0 = rows;
        I.status = I.src && tiffw_geom(widths[i], heights[i], d, comp, pred, rows_per_strip, &I.g) ? kTiffOk : kTiffInvalidArgument;
        if (I.status != kTiffOk) continue;
        if (strips.size() + (size_t)I.g.nstrips > 0x7FFFFFFFu) {
            (err = name) += ": too many strips in one call";
            return -1;
        }
        max_h = std::max(max_h, I.g.h);
        rows += I.g.h;
        for (int k = 0; k < I.g.nstrips; ++k) {
            Strip c{};
            c.img = i;
            c.y0 = k * I.g.rps;
            c.rows = tiffw_strip_rows(I.g, k);
            c.S = (uint32_t)((uint64_t)c.rows * I.g.rb);
            c.room = (uint32_t)std::min<uint64_t>(tiffw_payload_bound(I.g, c.rows), 0xFFFFFFFFu);
            c.at = at;
            // (the emit kernel stores whole words, the pack kernel whole 16 bytes)
            if (comp != kTiffwNone) at += (((int64_t)std::max(c.room, c.S) + 15) & ~(int64_t)15) + 32;
            if (comp == kTiffwDeflate) {
                c.nseg = (int32_t)((c.S + kSeg - 1) / kSeg);
                if ((int64_t)seg_strip.size() + c.nseg > 0x7FFFFFFF) {
                    (err = name) += ": too many segments in one call";
                    return -1;
                }
                c.seg0 = (int32_t)seg_strip.size();
                seg_strip.insert(seg_strip.end(), (size_t)c.nseg, (int32_t)strips.size());
                const int nb = tiffw_deflate_blocks(c.S);
                for (int b = 0; b < nb; ++b) {
                    Block K{};
                    K.strip = (int32_t)strips.size();
                    const int32_t a0 = (int32_t)((int64_t)c.nseg * b / nb), a1 = (int32_t)((int64_t)c.nseg * (b + 1) / nb);
                    K.seg0 = c.seg0 + a0;
                    K.nseg = a1 - a0;
                    K.last = b == nb - 1;
                    seg_block.insert(seg_block.end(), (size_t)K.nseg, (int32_t)blocks.size());
                    blocks.push_back(K);
                }
            }
            strips.push_back(c);
        }
    }
    const size_t ns = strips.size(), nseg = seg_strip.size(), nblk = blocks.size();
    size_t tat = 0;
    auto take = [&](size_t bytes) {
        const size_t o = tat;
        tat += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_img = take(sizeof(Img) * (size_t)n), o_st = take(sizeof(Strip) * ns),
                 o_rows = take(comp == kTiffwPackBits ? sizeof(uint32_t) * (size_t)rows : 0),
                 o_ss = take(sizeof(int32_t) * nseg), o_sb = take(sizeof(int32_t) * nseg), o_blk = take(sizeof(Block) * nblk),
                 o_bc = take(sizeof(BlockCodes) * nblk), o_off = take(sizeof(unsigned long long) * (nseg + 1)),
                 o_nt = take(sizeof(uint32_t) * nseg), o_sx = take(sizeof(uint32_t) * nseg),
                 o_ad = take(sizeof(uint32_t) * 2 * nseg);
    const size_t wbytes = (size_t)std::max<int64_t>(at, 64);
    const bool zl = comp == kTiffwDeflate && nseg > 0;
    if (!ws.tables.reserve(tat) || (comp != kTiffwNone && !ws.payload.reserve(wbytes)) ||
        (zl && (!ws.pred.reserve(wbytes) || !ws.tok.reserve(sizeof(uint16_t) * (size_t)kSlots * nseg) ||
                !ws.hist.reserve(sizeof(uint16_t) * (size_t)(kNLL + kND) * nseg)))) {
        (err = name) += ": allocation: ";
        err += hipGetErrorString(hipGetLastError());
        return -1;
    }
    uint8_t* A = ws.tables.p;
    Img* d_img = reinterpret_cast<Img*>(A + o_img);
    Strip* d_strip = reinterpret_cast<Strip*>(A + o_st);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(A + o_rows);
    int32_t* d_ss = reinterpret_cast<int32_t*>(A + o_ss);
    int32_t* d_sb = reinterpret_cast<int32_t*>(A + o_sb);
    Block* d_blk = reinterpret_cast<Block*>(A + o_blk);
    BlockCodes* d_bc = reinterpret_cast<BlockCodes*>(A + o_bc);
    unsigned long long* d_off = reinterpret_cast<unsigned long long*>(A + o_off);
    uint32_t* d_nt = reinterpret_cast<uint32_t*>(A + o_nt);
    uint32_t* d_sx = reinterpret_cast<uint32_t*>(A + o_sx);
    uint32_t* d_ad = reinterpret_cast<uint32_t*>(A + o_ad);
    auto ok = [&](hipError_t e) { return e == hipSuccess; };
    if (!ok(hipMemcpyAsync(d_img, imgs.data(), sizeof(Img) * (size_t)n, hipMemcpyHostToDevice, st)) ||
        (ns && !ok(hipMemcpyAsync(d_strip, strips.data(), sizeof(Strip) * ns, hipMemcpyHostToDevice, st))) ||
        (zl && (!ok(hipMemcpyAsync(d_ss, seg_strip.data(), sizeof(int32_t) * nseg, hipMemcpyHostToDevice, st)) ||
                !ok(hipMemcpyAsync(d_sb, seg_block.data(), sizeof(int32_t) * nseg, hipMemcpyHostToDevice, st)) ||
                !ok(hipMemcpyAsync(d_blk, blocks.data(), sizeof(Block) * nblk, hipMemcpyHostToDevice, st)) ||
                !ok(hipMemsetAsync(ws.payload.p, 0, wbytes, st))))) {
        (err = name) += ": copy: ";
        err += hipGetErrorString(hipGetLastError());
        return -1;
    }
    const unsigned gs = (unsigned)((ns + 63) / 64);
    if (ns && comp == kTiffwPackBits) {
        const dim3 grid((unsigned)((rows_grid(max_h, n) + 3) / 4), (unsigned)n);
        hipLaunchKernelGGL(k_tiffw_pb<false>, grid, dim3(256), 0, st, d_img, d_strip, d_rows, ws.payload.p);
        hipLaunchKernelGGL(k_tiffw_pb_scan, dim3(gs), dim3(64), 0, st, d_img, d_strip, (int64_t)ns, d_rows);
        hipLaunchKernelGGL(k_tiffw_pb<true>, grid, dim3(256), 0, st, d_img, d_strip, d_rows, ws.payload.p);
    } else if (ns && comp == kTiffwLzw) {
        hipLaunchKernelGGL(k_tiffw_lzw, dim3((unsigned)ns), dim3(64), 0, st, d_img, d_strip, ws.payload.p);
    } else if (zl) {
        hipLaunchKernelGGL(k_tiffw_pack, dim3((unsigned)nseg), dim3(256), 0, st, d_img, d_strip, d_ss, ws.pred.p, d_ad);
        hipLaunchKernelGGL(k_tiffw_lz77, dim3((unsigned)((nseg + kLzWaves - 1) / kLzWaves)), dim3(64 * kLzWaves), 0, st, d_img,
                           d_strip, d_ss, (int64_t)nseg, ws.pred.p, reinterpret_cast<uint16_t*>(ws.tok.p), d_nt,
                           reinterpret_cast<uint16_t*>(ws.hist.p), d_sx);
        hipLaunchKernelGGL(k_tiffw_huff, dim3((unsigned)nblk), dim3(64), 0, st, d_blk,
                           reinterpret_cast<const uint16_t*>(ws.hist.p), d_sx, d_bc, d_off);
        hipLaunchKernelGGL(k_tiffw_scan, dim3(gs), dim3(64), 0, st, d_img, d_strip, (int64_t)ns, d_ad, d_off);
    }
    hipLaunchKernelGGL(k_tiffw_layout, dim3((unsigned)n), dim3(256), 0, st, d_img, d_strip, comp, out_stride, d_sizes, d_status);
    if (zl)
        hipLaunchKernelGGL(k_tiffw_emit, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, d_img, d_strip, d_ss, d_sb, d_blk,
                           (int64_t)nseg, reinterpret_cast<const uint16_t*>(ws.tok.p), d_nt, d_bc, d_off, ws.payload.p);
    if (ns) hipLaunchKernelGGL(k_tiffw_gather, dim3((unsigned)ns), dim3(256), 0, st, d_img, d_strip, comp, ws.payload.p);
    return encode_finish(name, st, err);
}

}  // namespace icx
