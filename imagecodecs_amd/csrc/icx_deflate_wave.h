// icx_deflate_wave.h -- the wave-level part of the device deflate writer (gfx950, wave64), the write
// side's counterpart of icx_inflate_wave.h: staging a view of the stream in LDS, the 64-position
// window parse (ballot, one-step lazy evaluation, tokens + symbol counts), the workgroup's rank
// count for the Huffman sort, and the bit packing of a segment's tokens. Shared by icx_png.hip,
// icx_exrw.hip and icx_tiffw.hip, which keep their own views, candidate scoring, seams and layout;
// the serial part is icx_deflate_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "icx_deflate_core.h"

namespace icx {
namespace deflate {

// A lane's value at a wave-uniform lane index: v_readlane into a scalar register (__shfl is an LDS
// permute, and its round trip sat on the parse's serial chain)
__device__ __forceinline__ int rdl(int v, int i) { return __builtin_amdgcn_readlane(v, i); }

// nbytes (a 16-byte multiple) of the stream F[0..N) from index b0 (16-byte aligned) into LDS with
// 16-byte loads; bytes outside the stream read 0.
__device__ __forceinline__ void stage_view(const uint8_t* __restrict__ F, int64_t N, int64_t b0, uint8_t* lds, int lane,
                                           int nbytes) {
    for (int k = lane; k < nbytes / 16; k += 64) {
        const int64_t g = b0 + 16 * k;
        uint4 v;
        if (g >= 0 && g + 16 <= N) {
            v = *reinterpret_cast<const uint4*>(F + g);
        } else {
            uint8_t t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = (g + j >= 0 && g + j < N) ? F[g + j] : 0;
            __builtin_memcpy(&v, t, 16);
        }
        *reinterpret_cast<uint4*>(lds + 16 * k) = v;
    }
}

// The wave parses the window [p0, min(p0 + 64, s1)) of its segment from the lanes' scores (best:
// the longest match at the lane's position, 0 for none; bd: its distance; lit: the byte there):
// the literal run up to the first position with a match is emitted by all lanes at once, the match
// by lane 0. One-step lazy evaluation (zlib's deflate_slow): a match start whose successor in the
// window has a longer match becomes a literal, and the successor is considered in turn.
// T: the segment's token slots, SH: its symbol counts (LDS); nt slots, nm matches, xbits length /
// distance extra bits so far (lane 0's), pos: the first position not yet covered by a token.
__device__ __forceinline__ void parse_window(int best, int bd, uint32_t lit, int lane, int64_t p0, int64_t s1, uint16_t* T,
                                             uint32_t* SH, uint32_t& nt, uint32_t& nm, int64_t& pos, uint32_t& xbits) {
    const uint64_t cmask = __ballot(best >= 3);
    const int wend = (int)min((int64_t)64, s1 - p0);  // live lanes of this window
    while (pos < p0 + wend) {  // wave-uniform
        const int li = (int)(pos - p0);
        uint64_t m = cmask & (~0ull << li);
        int mi = m ? __ffsll((unsigned long long)m) - 1 : 64;
        while (mi + 1 < wend && rdl(best, mi + 1) > rdl(best, mi)) {
            m &= m - 1;
            mi = __ffsll((unsigned long long)m) - 1;
        }
        const int le = min(mi, wend);
        if (lane >= li && lane < le) {  // the literal run li .. le-1
            T[nt + (lane - li)] = (uint16_t)lit;
            atomicAdd(&SH[lit], 1u);
        }
        nt += (uint32_t)(le - li);
        pos = p0 + le;
        if (mi < wend) {  // the match at lane mi
            const int len = rdl(best, mi), dist = rdl(bd, mi);
            if (lane == 0) {
                T[nt] = (uint16_t)(0x4000u | (uint32_t)(len - 3));       // match: length slot,
                T[nt + 1] = (uint16_t)(0x8000u | (uint32_t)(dist - 1));  // then distance slot
                const int lc = len_code(len), dc = dist_code(dist);
                SH[257 + lc] += 1u;
                SH[kNLL + dc] += 1u;
                xbits += kLenExtra[lc] + kDistExtra[dc];
            }
            nt += 2;
            nm += 1;
            pos += len;
        }
    }
}

// The used symbols of freq[0..n) in (freq, symbol) ascending order, by rank counting over all
// lanes of the workgroup (blockDim.x lanes; the caller synchronises before and after).
__device__ inline void rank_order(const uint32_t* freq, int n, uint16_t* order) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t f = freq[i];
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            r += g && (g < f || (g == f && j < i));
        }
        order[r] = (uint16_t)i;
    }
}

__device__ __forceinline__ void or_bits(uint32_t* w, unsigned long long bitpos, uint64_t v, int nb) {
    if (!nb) return;
    const unsigned long long wi = bitpos >> 5;
    const int sh = (int)(bitpos & 31);
    const uint64_t hi = sh ? (v >> (32 - sh)) : (v >> 32);  // the bits above word wi
    atomicOr(w + wi, (uint32_t)(v << sh));
    if (sh + nb > 32) atomicOr(w + wi + 1, (uint32_t)hi);
    if (sh + nb > 64) atomicOr(w + wi + 2, (uint32_t)(hi >> 32));
}
// The block header: its words, shifted into place at bit `pos` of W; -> the bit after it.
__device__ __forceinline__ unsigned long long emit_header(uint32_t* W, unsigned long long pos, const BlockCodes& B, int lane) {
    const uint32_t hb = B.hdr_bits;
    for (uint32_t i = lane; i * 32 < hb; i += 64) {
        const int n = (int)min(32u, hb - i * 32);
        or_bits(W, pos + i * 32, n == 32 ? B.hdr[i] : (B.hdr[i] & ((1u << n) - 1u)), n);
    }
    return pos + hb;
}
// The segment's bits OR-ed into W (word 0 = the output word holding bit `pos`; zeroed), starting
// at bit `pos`: the block header (head), nh re-parsed head slots Hd (the PNG seams'; nullptr, 0
// without), its own slots T[0 .. nt), the end-of-block code (eob). Each round of 64 tokens gets
// bit offsets from a wave prefix sum.
__device__ __forceinline__ void emit_segment(uint32_t* W, unsigned long long pos, const BlockCodes& B,
                                             const uint16_t* Hd, uint32_t nh, const uint16_t* T, uint32_t nt,
                                             bool head, bool eob, int lane) {
    if (head) pos = emit_header(W, pos, B, lane);
    const uint32_t n = nh + nt;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        int nb = 0;
        uint64_t v = 0;
        if (i < nh) v = token_code(B, Hd[i], i + 1 < nh ? Hd[i + 1] : 0u, nb);
        else if (i < n) v = token_code(B, T[i - nh], i + 1 < n ? T[i + 1 - nh] : 0u, nb);
        uint32_t inc;  // inclusive scan of nb over the wave (rocprim's DPP cross-lane scan)
        using WScan = rocprim::warp_scan<uint32_t, 64>;
        typename WScan::storage_type wst;  // empty for the cross-lane implementation
        WScan().inclusive_scan((uint32_t)nb, inc, wst);
        or_bits(W, pos + inc - nb, v, nb);
        pos += (uint32_t)rdl((int)inc, 63);
    }
    if (eob && lane == 0) or_bits(W, pos, B.ll_code[256], B.ll_len[256]);
}
// emit_segment for a wave's private LDS image: each lane takes kRun consecutive token slots, one
// wave prefix sum of the lanes' bit totals places them, and each lane packs its slots into whole
// words in a register -- the words it fills alone are plain stores, only its first and last
// (shared with the neighbouring lanes) are atomicOr. (One slot per lane OR-ed every token into LDS
// with up to three atomics, several lanes on each word.)
constexpr int kRun = 8;
__device__ __forceinline__ void emit_segment_runs(uint32_t* W, unsigned long long pos, const BlockCodes& B,
                                                  const uint16_t* Hd, uint32_t nh, const uint16_t* T, uint32_t nt,
                                                  bool head, bool eob, int lane) {
    if (head) pos = emit_header(W, pos, B, lane);
    const uint32_t n = nh + nt;
    auto slot = [&](uint32_t i) -> uint32_t { return i < nh ? (uint32_t)Hd[i] : (uint32_t)T[i - nh]; };
    for (uint32_t i0 = 0; i0 < n; i0 += 64 * kRun) {
        const uint32_t ib = i0 + (uint32_t)lane * kRun;
        uint64_t v[kRun];
        int nb[kRun];
        uint32_t tot = 0;
#pragma unroll
        for (int r = 0; r < kRun; ++r) {
            const uint32_t i = ib + r;
            nb[r] = 0;
            v[r] = i < n ? token_code(B, slot(i), i + 1 < n ? slot(i + 1) : 0u, nb[r]) : 0;
            tot += (uint32_t)nb[r];
        }
        uint32_t inc;  // inclusive scan of the lanes' bit totals (rocprim's DPP cross-lane scan)
        using WScan = rocprim::warp_scan<uint32_t, 64>;
        typename WScan::storage_type wst;
        WScan().inclusive_scan(tot, inc, wst);
        const unsigned long long s0 = pos + inc - tot;
        uint32_t wi = (uint32_t)(s0 >> 5);
        int an = (int)(s0 & 31);
        uint64_t acc = 0;
        bool first = true;
        auto put = [&](uint32_t piece, int k) {  // k <= 32 bits; an < 32 before
            acc |= (uint64_t)piece << an;
            an += k;
            if (an >= 32) {
                if (first) atomicOr(W + wi, (uint32_t)acc);  // (shared with the lane before)
                else W[wi] = (uint32_t)acc;
                first = false;
                ++wi;
                acc >>= 32;
                an -= 32;
            }
        };
#pragma unroll
        for (int r = 0; r < kRun; ++r) {
            if (nb[r] > 32) {
                put((uint32_t)v[r], 32);
                put((uint32_t)(v[r] >> 32), nb[r] - 32);
            } else if (nb[r] > 0) {
                put((uint32_t)v[r], nb[r]);
            }
        }
        if (tot && an > 0) atomicOr(W + wi, (uint32_t)acc);  // (shared with the lane after)
        pos += (uint32_t)rdl((int)inc, 63);
    }
    if (eob && lane == 0) or_bits(W, pos, B.ll_code[256], B.ll_len[256]);
}

}  // namespace deflate
}  // namespace icx
