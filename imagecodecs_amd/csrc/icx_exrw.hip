// icx_exrw.hip -- OpenEXR write on the MI355X: Image::writeExr (codecs.cpp:495-505), i.e. tinyexr's
// SaveEXR(float*, w, h, components, fp16, path) (tinyexr.h:9333-9480).
//
// Parity contract: header, offset table, chunk headers, NONE payloads and raw ZIP
// payloads are tinyexr's bytes; a compressed ZIP payload is our own zlib stream that inflates to
// exactly the predictor bytes tinyexr hands to compress(). A file is ceil(h / 16) independent
// chunks, and every kernel runs over all chunks of all images of a call at once.
//
//   k_exrw_pack    one workgroup per 4 KiB segment of a chunk: the predictor bytes as a gather from
//                  the float pixels (icx_exrw_core.h), 16-byte stores, Adler-32 partials
//   k_exrw_lz77    one wave per segment: lazy LZ77 over the distances the transform makes likely
//                  (1, 2, the previous channel plane, the previous line) and a hash of the segment's
//                  own earlier bytes, tokens + symbol counts;
//                  matches end at the segment's end
//   k_exrw_huff    one workgroup per deflate block (runs of at most 16 segments, an even number per
//                  chunk): length-limited codes (15 / 7 bits), the dynamic header, bits per segment
//   k_exrw_scan    one workgroup per chunk: the segments' bit offsets, the stream's size and
//                  Adler-32, and whether the chunk is stored raw (stream >= samples)
//   k_exrw_layout  one workgroup per image: payload sizes -> file offsets, the file's size; header,
//                  offset table and chunk headers
//   k_exrw_emit    one wave per segment: LSB-first bit packing at its offset in the chunk's stream
//   k_exrw_gather  each payload (stream or raw sample bytes) to its place in the file
// The deflate stages follow the PNG coder's (icx_png.hip), and the back end (tables, Huffman code
// lengths and codes, token bits, window parse, bit packing) is one text for both:
// icx_deflate_core.h and icx_deflate_wave.h. tests/test_gpu_deflate_pin.py pins both writers' bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "icx_deflate_wave.h"
#include "icx_exrw_core.h"
#include "icx_internal.h"
#include "icx_mem.h"

namespace icx {

namespace exrw {

using namespace deflate;  // the deflate back end shared with icx_png.hip

constexpr int kSeg = 4096;            // LZ77 / emit segment (predictor bytes)
constexpr int kSlots = kSeg;          // token slots per segment: a match takes 2 slots for >= 3 bytes
constexpr int kBlockSegs = 16;        // deflate blocks of at most 64 KiB ...
constexpr int kMinBlockSegs = 4;      // ... and a chunk under 32 KiB is one block (a header is ~80 bytes)
constexpr int kOk = 0, kInvalidArgument = -3;  // TINYEXR_SUCCESS, TINYEXR_ERROR_INVALID_ARGUMENT
constexpr uint32_t kMaxTreeWeight = 1u << 18;  // symbol counts are scaled under this before the code
                                               // is built (tree depth < 40, huff_lengths' histogram)

struct Img {
    const uint32_t* src;  // interleaved float pixels, as bit patterns
    uint8_t* out;
    uint64_t cap;
    ExrwGeom g;
    int32_t chunk0, nchunk;
    uint32_t hdr_at, hdr_len;  // this image's header bytes in the header blob
};
struct Chunk {
    int32_t img, y0;
    uint32_t S;         // sample bytes
    int32_t seg0, nseg;
    int64_t at;         // its bytes in the predictor and stream workspaces (16-byte aligned)
    // written on the device
    uint32_t zsize;     // zlib stream bytes
    uint32_t raw;       // payload = the sample bytes (NONE, or stream >= S)
    uint32_t adler;
    uint32_t pad_;
    uint64_t file_at;   // the chunk header's offset in the file
};
// A deflate block: a run of a chunk's segments with codes of its own. The two halves of the
// reordered bytes (even / odd sample bytes) and the channel planes have different statistics.
struct Block {
    int32_t chunk;
    int32_t seg0, nseg;  // global segment index, count
    int32_t last;        // the chunk's last block (BFINAL)
};
struct Out {
    unsigned long long total, fits;  // file bytes; total <= cap (only then is anything written)
};

// -------------------------------------------------------------------------------- pack
// Thread t of segment workgroup: 16 consecutive predictor bytes (17 reordered bytes), one 16-byte
// store; bytes past S are 0. The segment's Adler-32 partials: sum b, sum (S - t) b.
__global__ __launch_bounds__(256) void k_exrw_pack(const Img* __restrict__ imgs, const Chunk* __restrict__ chunks,
                                                   const int32_t* __restrict__ seg_chunk, uint8_t* __restrict__ P,
                                                   uint32_t* __restrict__ adl) {
    __shared__ unsigned long long s_a[4], s_b[4];
    const int64_t seg = blockIdx.x;
    const Chunk& c = chunks[seg_chunk[seg]];
    const Img& I = imgs[c.img];
    if (!I.g.zip) return;  // (uniform)
    const ExrwGeom g = I.g;
    const uint32_t S = c.S, t0 = (uint32_t)(seg - c.seg0) * kSeg + threadIdx.x * 16u;
    unsigned long long a1 = 0, a2 = 0;
    if (t0 < ((S + 15u) & ~15u)) {
        uint8_t v[16];
        uint32_t prev = (t0 > 0 && t0 <= S) ? exrw_reordered_byte(I.src, g, c.y0, S, t0 - 1) : 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t t = t0 + j;
            uint32_t b = 0;
            if (t < S) {
                const uint32_t r = exrw_reordered_byte(I.src, g, c.y0, S, t);
                b = t == 0 ? r : (r - prev + 384u) & 255u;
                prev = r;
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

// -------------------------------------------------------------------------------- LZ77
// Token slots (uint16): a literal is its byte value (< 256); a match is a length slot
// 0x4000 | (len - 3) followed by a distance slot 0x8000 | (dist - 1).
// A wave's views of the chunk's predictor bytes, staged in LDS: view 0 holds the segment and the 16
// bytes before it (distances 1 and 2), view 1 the same bytes one channel plane back, view 2 one
// line back. A match ends at the segment's end, so a candidate at distance d compares bytes of
// [s0 - d, s1 - d) only. Every view starts at a 16-byte-aligned index and has dword-read slack.
constexpr int kNear = 16;
constexpr int kView = kSeg + 48;  // 16-byte multiple: kSeg + alignment (<= 31) + dword reads (<= 8)
struct View {
    const uint8_t* p;  // LDS base = chunk index b0
    int64_t b0;
    __device__ __forceinline__ uint32_t dword(int64_t i) const {  // bytes i .. i+3, byte i lowest
        const int64_t o = i - b0;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p) + (o >> 2);
        return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(o & 3));
    }
};
// Length of the match at p (view A) against p - dist (view B), at most maxlen.
__device__ __forceinline__ int match_len(const View& A, const View& B, int64_t p, int64_t dist, int maxlen) {
    int l = 0;
    while (l < maxlen) {
        const uint32_t x = A.dword(p + l) ^ B.dword(p - dist + l);
        if (x) return min(l + (int)(__builtin_ctz(x) >> 3), maxlen);
        l += 4;
    }
    return maxlen;
}

// Two waves per workgroup, a segment each. The wave walks its segment in 64-position windows:
// every lane scores the position under it against the four structural candidates and against the
// latest earlier position of the segment with the same four bytes (a hash table of the windows
// already walked, kept in LDS; atomicMax keeps it deterministic), then the wave parses the
// window with ballots -- the literal run up to the first match is emitted by all lanes at once, the
// match by one. One-step lazy evaluation as zlib's deflate_slow (a match whose successor has a
// longer one becomes a literal).
constexpr int kLzWaves = 2;
constexpr int kHashBits = 11;
__global__ __launch_bounds__(64 * kLzWaves) void k_exrw_lz77(const Img* __restrict__ imgs, const Chunk* __restrict__ chunks,
                                                   const int32_t* __restrict__ seg_chunk, int64_t nseg,
                                                   const uint8_t* __restrict__ P, uint16_t* __restrict__ tok,
                                                   uint32_t* __restrict__ ntok, uint16_t* __restrict__ seghist,
                                                   uint32_t* __restrict__ segx) {
    __shared__ uint32_t s_h[kLzWaves][kNLL + kND];
    __shared__ uint32_t s_hash[kLzWaves][1 << kHashBits];  // 1 + segment offset of the latest position, 0: none
    __shared__ __attribute__((aligned(16))) uint8_t views[kLzWaves][3][kView];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * kLzWaves + wave;
    if (seg >= nseg) return;  // wave-uniform; no block barriers below
    const Chunk& c = chunks[seg_chunk[seg]];
    const ExrwGeom g = imgs[c.img].g;
    if (!g.zip) return;
    const uint8_t* F = P + c.at;
    const int64_t N = c.S;
    const int64_t s0 = (seg - c.seg0) * kSeg, s1 = min(N, s0 + kSeg);
    const int64_t plane = (int64_t)g.w * g.s / 2, line = plane * g.nch;
    int64_t cand[4] = {1, 2, plane, line};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (cand[k] <= 0 || cand[k] > 32768) cand[k] = 0;
    View V[3];
    V[0].b0 = (s0 - kNear) & ~(int64_t)15;
    V[1].b0 = (s0 - cand[2]) & ~(int64_t)15;
    V[2].b0 = (s0 - cand[3]) & ~(int64_t)15;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        V[k].p = views[wave][k];
        stage_view(F, N, V[k].b0, views[wave][k], lane, kView);
    }
    uint32_t* SH = s_h[wave];
    for (int i = lane; i < kNLL + kND; i += 64) SH[i] = 0;
    uint32_t* HT = s_hash[wave];
    for (int i = lane; i < (1 << kHashBits); i += 64) HT[i] = 0;
    __builtin_amdgcn_wave_barrier();
    uint16_t* T = tok + seg * kSlots;
    uint32_t xbits = 0;  // length / distance extra bits of the segment's matches (lane 0)
    uint32_t nt = 0, nm = 0;  // token slots, matches (not used here)
    int64_t pos = s0;  // first position not yet covered by a token
    for (int64_t p0 = s0; p0 < s1; p0 += 64) {
        const int64_t q = p0 + lane;
        int best = 0, bd = 0;
        uint32_t lit = 0, hslot = 0, hprev = 0;
        const bool hashed = q + 4 <= s1;
        if (hashed) {
            hslot = (V[0].dword(q) * 2654435761u) >> (32 - kHashBits);
            hprev = HT[hslot];
        }
        __builtin_amdgcn_wave_barrier();  // (every lane has read the table of the windows before)
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
                for (int k = 0; k < 4; ++k) {
                    const int64_t dd = cand[k];
                    if (dd == 0 || dd > q) continue;
                    const View& B = V[k < 2 ? 0 : k - 1];
                    if (((B.dword(q - dd) ^ t4) & 0xFFFFFFu) != 0) continue;  // first three bytes
                    const int l = 3 + match_len(V[0], B, q + 3, dd, maxlen - 3);
                    // a short match far back costs more bits than its literals (zlib's TOO_FAR)
                    if (l < (dd > 4096 ? 5 : dd > 2 ? 4 : 3)) continue;
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

// ------------------------------------------------------------------------------ Huffman
// One workgroup per deflate block. Thread 0 builds the codes and the header (deterministic, tiny);
// then the workgroup computes the bits of each of the block's segments from its symbol counts and
// the code lengths (k_exrw_scan turns them into offsets).
__global__ __launch_bounds__(64) void k_exrw_huff(const Img* __restrict__ imgs, const Chunk* __restrict__ chunks,
                                                  const Block* __restrict__ blocks,
                                                  const uint16_t* __restrict__ seghist, const uint32_t* __restrict__ segx,
                                                  BlockCodes* __restrict__ bc, unsigned long long* __restrict__ off) {
    __shared__ uint32_t f_ll[kNLL], f_d[kND];
    __shared__ uint16_t order[kNLL], order_d[kND];
    __shared__ uint32_t wt[2 * kNLL];
    __shared__ int16_t parent[2 * kNLL];
    __shared__ uint8_t l_ll[kNLL], l_d[kND];
    __shared__ uint8_t rle_sym[kNLL + kND];
    __shared__ uint8_t rle_ext[kNLL + kND];
    __shared__ uint32_t s_hdr_bits;
    const Block& K = blocks[blockIdx.x];
    if (!imgs[chunks[K.chunk].img].g.zip) return;  // (uniform)
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
    if (threadIdx.x == 0) {
        // a very large block: scale the counts so that the tree stays shallow (used stays used)
        uint64_t tot = 0;
        for (int i = 0; i < kNLL; ++i) tot += f_ll[i];
        int sh = 0;
        while ((tot >> sh) > kMaxTreeWeight) ++sh;
        if (sh) {
            for (int i = 0; i < kNLL; ++i)
                if (f_ll[i]) f_ll[i] = max(1u, f_ll[i] >> sh);
            for (int i = 0; i < kND; ++i)
                if (f_d[i]) f_d[i] = max(1u, f_d[i] >> sh);
        }
        pad_block_counts(f_ll, f_d);
    }
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
    // bits per segment: its symbol counts times the code lengths, plus its matches' extra bits
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

// One workgroup per chunk: the segments' bits scanned into bit offsets within the stream (thread
// 0: a chunk has S / 4 KiB segments), the stream's size and Adler-32, and whether the chunk is
// stored raw.
__global__ __launch_bounds__(64) void k_exrw_scan(const Img* __restrict__ imgs, Chunk* __restrict__ chunks,
                                                  const uint32_t* __restrict__ adl, unsigned long long* __restrict__ off) {
    Chunk& c = chunks[blockIdx.x];
    if (!imgs[c.img].g.zip) return;
    const int64_t seg0 = c.seg0, ns = c.nseg;
    if (threadIdx.x == 0) {
        unsigned long long run = 0, a = 0, b = 0;
        for (int64_t s = 0; s < ns; ++s) {
            const unsigned long long v = off[seg0 + s];
            off[seg0 + s] = run;
            run += v;
            a += adl[2 * (seg0 + s)];
            b += adl[2 * (seg0 + s) + 1];
        }
        const unsigned long long z = 2 + (run + 7) / 8 + 4;
        c.raw = z >= c.S ? 1u : 0u;
        c.zsize = c.raw ? 0u : (uint32_t)z;
        const uint32_t A = (uint32_t)((1 + a) % kAdlerMod), Bs = (uint32_t)((c.S + b) % kAdlerMod);
        c.adler = Bs << 16 | A;
    }
}

// ------------------------------------------------------------------------------- layout
__device__ __forceinline__ void put_le(uint8_t* p, unsigned long long v, int n) {
    for (int k = 0; k < n; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
// One workgroup per image: thread 0 walks the chunks (payload = min(stream, samples)) into file
// offsets; when the file fits, the workgroup writes the header, the offset table and the chunk
// headers (byte stores: the output may start at any address).
__global__ __launch_bounds__(256) void k_exrw_layout(const Img* __restrict__ imgs, Chunk* __restrict__ chunks,
                                                     const uint8_t* __restrict__ hdrs, Out* __restrict__ outs) {
    __shared__ unsigned long long s_total;
    const Img& I = imgs[blockIdx.x];
    Chunk* C = chunks + I.chunk0;
    if (threadIdx.x == 0) {
        unsigned long long at = (unsigned long long)I.hdr_len + 8ull * (unsigned long long)I.nchunk;
        for (int k = 0; k < I.nchunk; ++k) {
            C[k].file_at = at;
            at += 8ull + (C[k].raw ? C[k].S : C[k].zsize);
        }
        s_total = at;
        outs[blockIdx.x].total = at;
        outs[blockIdx.x].fits = at <= I.cap ? 1ull : 0ull;
    }
    __syncthreads();
    if (s_total > I.cap) return;
    for (uint32_t i = threadIdx.x; i < I.hdr_len; i += 256) I.out[i] = hdrs[I.hdr_at + i];
    for (int k = threadIdx.x; k < I.nchunk; k += 256) {
        put_le(I.out + I.hdr_len + 8ull * k, C[k].file_at, 8);
        uint8_t* p = I.out + C[k].file_at;
        put_le(p, (uint32_t)C[k].y0, 4);
        put_le(p + 4, C[k].raw ? C[k].S : C[k].zsize, 4);
    }
}

// --------------------------------------------------------------------------------- emit
// One wave per segment: its bits are built in the wave's LDS image of its output words and leave
// with coalesced stores -- the two boundary words (shared with the neighbouring segments) with
// atomicOr into the zeroed stream workspace. A segment whose bits exceed the image ORs straight
// into the workspace.
constexpr int kEmitWords = 2048;
__global__ __launch_bounds__(256) void k_exrw_emit(const Img* __restrict__ imgs, const Chunk* __restrict__ chunks,
                                                   const int32_t* __restrict__ seg_chunk,
                                                   const int32_t* __restrict__ seg_block,
                                                   const Block* __restrict__ blocks, int64_t nseg,
                                                   const uint16_t* __restrict__ tok, const uint32_t* __restrict__ ntok,
                                                   const BlockCodes* __restrict__ bc,
                                                   const unsigned long long* __restrict__ off, const Out* __restrict__ outs,
                                                   uint8_t* __restrict__ Z) {
    __shared__ uint32_t img[4][kEmitWords];
    __shared__ BlockCodes Bs[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * 4 + wave;
    if (seg >= nseg) return;  // wave-uniform; no block barriers below
    const int32_t ci = seg_chunk[seg];
    const Chunk& c = chunks[ci];
    if (!imgs[c.img].g.zip || c.raw || !outs[c.img].fits) return;
    BlockCodes& B = Bs[wave];
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bc + seg_block[seg]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&B);
        for (int i = lane; i < (int)(sizeof(BlockCodes) / 4); i += 64) dst[i] = src[i];
    }
    __builtin_amdgcn_wave_barrier();
    const Block& K = blocks[seg_block[seg]];
    const bool head = seg == K.seg0, eob = seg == (int64_t)K.seg0 + K.nseg - 1;  // opens / closes its block
    const unsigned long long o0 = off[seg];
    // the stream's bits: the last segment's end is the stream's (zsize - 6 bytes, rounded up)
    const unsigned long long o1 =
        seg - c.seg0 == c.nseg - 1 ? (unsigned long long)(c.zsize - 6) * 8ull : off[seg + 1];
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

// ------------------------------------------------------------------------------- gather
// One workgroup per 4 KiB of a chunk's payload: the zlib stream (78 01, the deflate bytes, the
// Adler-32 big-endian) or the raw sample bytes, to file_at + 8.
__global__ __launch_bounds__(256) void k_exrw_gather(const Img* __restrict__ imgs, const Chunk* __restrict__ chunks,
                                                     const int32_t* __restrict__ seg_chunk, const Out* __restrict__ outs,
                                                     const uint8_t* __restrict__ Z) {
    const int64_t seg = blockIdx.x;
    const Chunk& c = chunks[seg_chunk[seg]];
    const Img& I = imgs[c.img];
    if (!outs[c.img].fits) return;
    const uint32_t n = c.raw ? c.S : c.zsize;
    const uint32_t i0 = (uint32_t)(seg - c.seg0) * kSeg;
    uint8_t* dst = I.out + c.file_at + 8;
    const uint8_t* z = Z + c.at;
    const ExrwGeom g = I.g;
    for (uint32_t k = threadIdx.x; k < (uint32_t)kSeg; k += 256) {
        const uint32_t i = i0 + k;
        if (i >= n) break;
        uint32_t b;
        if (c.raw) b = exrw_raw_byte(I.src, g, c.y0, i);
        else if (i < 2) b = i == 0 ? 0x78u : 0x01u;
        else if (i >= n - 4) b = (c.adler >> (8 * (n - 1 - i))) & 255u;
        else b = z[i - 2];
        dst[i] = (uint8_t)b;
    }
}

}  // namespace exrw

// Grow-only device buffers of one context's EXR writes (icx_ctx::exrw).
struct ExrwWs {
    Buf<uint8_t> tables, pred, stream, tok, hist, io;
    Buf<exrw::Out> h_out{true};
};
ExrwWs* exrw_ws_create() { return new ExrwWs(); }
void exrw_ws_destroy(ExrwWs* w) { delete w; }

bool exrw_args_ok(int width, int height, int components) {
    if (!(components == 1 || components == 3 || components == 4) || width < 1 || height < 1) return false;
    // a chunk's bytes are indexed with 32 bits
    return (uint64_t)width * (uint64_t)components * 4u * (uint64_t)kExrwZipLines < (1ull << 31);
}
size_t exrw_encode_bound(int width, int height, int components, int fp16) {
    if (!exrw_args_ok(width, height, components)) return 0;
    return (size_t)exrw_bound(exrw_geom(width, height, components, fp16));
}

// n writes in one pass. d_src[i]: width*height*components floats on the device; d_out[i]: caps[i]
// bytes on the device (any alignment). codes[i]: ICX_EXR_SUCCESS, INVALID_ARGUMENT, or INTERNAL_ERR
// when the file does not fit caps[i] (nothing of it is written; sizes[i] says what it needs).
// Returns 0, or -100 with err set (a device failure).
int exrw_encode_batch(hipStream_t st, ExrwWs& ws, int n, const float* const* d_src, const int32_t* widths,
                      const int32_t* heights, int components, int fp16, uint8_t* const* d_out, const size_t* caps,
                      int32_t* codes, size_t* sizes, std::string& err) {
    using namespace exrw;
    std::vector<Img> imgs;
    std::vector<Chunk> chunks;
    std::vector<int32_t> seg_chunk, seg_block;
    std::vector<Block> blocks;
    std::vector<uint8_t> hdrs;
    std::vector<int> slot((size_t)n, -1);
    int64_t at = 0;
    bool any_zip = false;
    for (int i = 0; i < n; ++i) {
        sizes[i] = 0;
        if (!exrw_args_ok(widths[i], heights[i], components) || !d_src[i] || !d_out[i]) {
            codes[i] = exrw::kInvalidArgument;
            continue;
        }
        codes[i] = exrw::kOk;
        Img I{};
        I.src = reinterpret_cast<const uint32_t*>(d_src[i]);
        I.out = d_out[i];
        I.cap = caps[i];
        I.g = exrw_geom(widths[i], heights[i], components, fp16);
        any_zip = any_zip || I.g.zip;
        const std::vector<uint8_t> h = exrw_header(I.g);
        I.hdr_at = (uint32_t)hdrs.size();
        I.hdr_len = (uint32_t)h.size();
        hdrs.insert(hdrs.end(), h.begin(), h.end());
        const int64_t nc = exrw_nchunks(I.g);
        if (nc > 0x7FFFFFFF - (int64_t)chunks.size()) {
            codes[i] = exrw::kInvalidArgument;
            continue;
        }
        I.chunk0 = (int32_t)chunks.size();
        I.nchunk = (int32_t)nc;
        for (int64_t k = 0; k < nc; ++k) {
            Chunk c{};
            c.img = (int32_t)imgs.size();
            c.y0 = (int32_t)(k * I.g.lines);
            c.S = (uint32_t)exrw_chunk_bytes(I.g, k);
            c.nseg = (int32_t)((c.S + kSeg - 1) / kSeg);
            if ((int64_t)seg_chunk.size() + c.nseg > 0x7FFFFFFF) {
                err = "icx_exr_encode: too many segments in one call";
                return -100;
            }
            c.seg0 = (int32_t)seg_chunk.size();
            c.at = at;
            c.raw = I.g.zip ? 0u : 1u;
            at += (((int64_t)c.S + 15) & ~(int64_t)15) + 32;
            seg_chunk.insert(seg_chunk.end(), (size_t)c.nseg, (int32_t)chunks.size());
            // deflate blocks: an even number of near-equal runs of at most kBlockSegs segments (the
            // middle boundary is the boundary of the reordered halves); a small chunk is one block
            const int nb = c.nseg < 2 * kMinBlockSegs ? 1 : 2 * ((c.nseg + 2 * kBlockSegs - 1) / (2 * kBlockSegs));
            for (int b = 0; b < nb; ++b) {
                Block K{};
                K.chunk = (int32_t)chunks.size();
                const int32_t a0 = (int32_t)((int64_t)c.nseg * b / nb), a1 = (int32_t)((int64_t)c.nseg * (b + 1) / nb);
                K.seg0 = c.seg0 + a0;
                K.nseg = a1 - a0;
                K.last = b == nb - 1;
                seg_block.insert(seg_block.end(), (size_t)K.nseg, (int32_t)blocks.size());
                blocks.push_back(K);
            }
            chunks.push_back(c);
        }
        slot[i] = (int)imgs.size();
        imgs.push_back(I);
    }
    if (imgs.empty()) return 0;
    const size_t ni = imgs.size(), nc = chunks.size(), nseg = seg_chunk.size(), nblk = blocks.size();
    // tables: images, chunks, segment -> chunk, header bytes, block codes, bit offsets, results
    size_t tat = 0;
    auto take = [&](size_t bytes) {
        const size_t o = tat;
        tat += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_img = take(sizeof(Img) * ni), o_ch = take(sizeof(Chunk) * nc), o_sc = take(sizeof(int32_t) * nseg),
                 o_sb = take(sizeof(int32_t) * nseg), o_blk = take(sizeof(Block) * nblk), o_hdr = take(hdrs.size()),
                 o_bc = take(sizeof(BlockCodes) * nblk),
                 o_off = take(sizeof(unsigned long long) * (nseg + 1)), o_out = take(sizeof(Out) * ni);
    // per segment: token count, extra bits, Adler partials (2)
    const size_t o_nt = take(sizeof(uint32_t) * nseg), o_sx = take(sizeof(uint32_t) * nseg),
                 o_ad = take(sizeof(uint32_t) * 2 * nseg);
    const size_t wbytes = (size_t)std::max<int64_t>(at, 64);
    if (!ws.tables.reserve(tat) || !ws.h_out.reserve(sizeof(Out) * ni) ||
        (any_zip && (!ws.pred.reserve(wbytes) || !ws.stream.reserve(wbytes) ||
                     !ws.tok.reserve(sizeof(uint16_t) * (size_t)kSlots * nseg) ||
                     !ws.hist.reserve(sizeof(uint16_t) * (size_t)(kNLL + kND) * nseg)))) {
        (void)hipGetLastError();
        err = "icx_exr_encode: device allocation failed";
        return -100;
    }
    uint8_t* A = ws.tables.p;
    Img* d_img = reinterpret_cast<Img*>(A + o_img);
    Chunk* d_ch = reinterpret_cast<Chunk*>(A + o_ch);
    int32_t* d_sc = reinterpret_cast<int32_t*>(A + o_sc);
    int32_t* d_sb = reinterpret_cast<int32_t*>(A + o_sb);
    Block* d_blk = reinterpret_cast<Block*>(A + o_blk);
    BlockCodes* d_bc = reinterpret_cast<BlockCodes*>(A + o_bc);
    unsigned long long* d_off = reinterpret_cast<unsigned long long*>(A + o_off);
    Out* d_res = reinterpret_cast<Out*>(A + o_out);
    uint32_t* d_nt = reinterpret_cast<uint32_t*>(A + o_nt);
    uint32_t* d_sx = reinterpret_cast<uint32_t*>(A + o_sx);
    uint32_t* d_ad = reinterpret_cast<uint32_t*>(A + o_ad);
    auto ok = [&](hipError_t e) { return e == hipSuccess; };
    if (!ok(hipMemcpyAsync(d_img, imgs.data(), sizeof(Img) * ni, hipMemcpyHostToDevice, st)) ||
        !ok(hipMemcpyAsync(d_ch, chunks.data(), sizeof(Chunk) * nc, hipMemcpyHostToDevice, st)) ||
        !ok(hipMemcpyAsync(d_sc, seg_chunk.data(), sizeof(int32_t) * nseg, hipMemcpyHostToDevice, st)) ||
        !ok(hipMemcpyAsync(d_sb, seg_block.data(), sizeof(int32_t) * nseg, hipMemcpyHostToDevice, st)) ||
        !ok(hipMemcpyAsync(d_blk, blocks.data(), sizeof(Block) * nblk, hipMemcpyHostToDevice, st)) ||
        !ok(hipMemcpyAsync(A + o_hdr, hdrs.data(), hdrs.size(), hipMemcpyHostToDevice, st)) ||
        (any_zip && !ok(hipMemsetAsync(ws.stream.p, 0, wbytes, st)))) {
        (void)hipGetLastError();
        err = "icx_exr_encode: device copy failed";
        return -100;
    }
    const unsigned g4 = (unsigned)((nseg + 3) / 4), glz = (unsigned)((nseg + kLzWaves - 1) / kLzWaves);
    if (any_zip) {
        hipLaunchKernelGGL(k_exrw_pack, dim3((unsigned)nseg), dim3(256), 0, st, d_img, d_ch, d_sc, ws.pred.p, d_ad);
        hipLaunchKernelGGL(k_exrw_lz77, dim3(glz), dim3(64 * kLzWaves), 0, st, d_img, d_ch, d_sc, (int64_t)nseg, ws.pred.p,
                           reinterpret_cast<uint16_t*>(ws.tok.p), d_nt, reinterpret_cast<uint16_t*>(ws.hist.p), d_sx);
        hipLaunchKernelGGL(k_exrw_huff, dim3((unsigned)nblk), dim3(64), 0, st, d_img, d_ch, d_blk,
                           reinterpret_cast<const uint16_t*>(ws.hist.p), d_sx, d_bc, d_off);
        hipLaunchKernelGGL(k_exrw_scan, dim3((unsigned)nc), dim3(64), 0, st, d_img, d_ch, d_ad, d_off);
    }
    hipLaunchKernelGGL(k_exrw_layout, dim3((unsigned)ni), dim3(256), 0, st, d_img, d_ch, A + o_hdr, d_res);
    if (any_zip)
        hipLaunchKernelGGL(k_exrw_emit, dim3(g4), dim3(256), 0, st, d_img, d_ch, d_sc, d_sb, d_blk, (int64_t)nseg,
                           reinterpret_cast<const uint16_t*>(ws.tok.p), d_nt, d_bc, d_off, d_res, ws.stream.p);
    hipLaunchKernelGGL(k_exrw_gather, dim3((unsigned)nseg), dim3(256), 0, st, d_img, d_ch, d_sc, d_res, ws.stream.p);
    if (!ok(hipGetLastError()) || !ok(hipMemcpyAsync(ws.h_out.p, d_res, sizeof(Out) * ni, hipMemcpyDeviceToHost, st)) ||
        !ok(hipStreamSynchronize(st))) {
        (void)hipGetLastError();
        err = "icx_exr_encode: HIP failure";
        return -100;
    }
    for (int i = 0; i < n; ++i) {
        if (slot[i] < 0) continue;
        sizes[i] = (size_t)ws.h_out.p[slot[i]].total;
        if (!ws.h_out.p[slot[i]].fits) codes[i] = -100;
    }
    return 0;
}

// One write from host pixels: they are copied to the device, the file comes back malloc'd.
int exrw_save_to_memory(hipStream_t st, ExrwWs& ws, const float* data, int width, int height, int components, int fp16,
                        uint8_t** out, size_t* size, std::string& err) {
    const size_t nin = (size_t)width * height * components * sizeof(float);
    const size_t bound = exrw_encode_bound(width, height, components, fp16);
    const size_t o_out = (nin + 255) & ~(size_t)255;
    if (!ws.io.reserve(o_out + bound)) {
        (void)hipGetLastError();
        err = "icx_exr_save_to_memory: device allocation failed";
        return -100;
    }
    if (hipMemcpyAsync(ws.io.p, data, nin, hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        err = "icx_exr_save_to_memory: device copy failed";
        return -100;
    }
    const float* src = reinterpret_cast<const float*>(ws.io.p);
    uint8_t* dst = ws.io.p + o_out;
    int32_t code = 0, w = width, h = height;
    size_t total = 0;
    const int rc = exrw_encode_batch(st, ws, 1, &src, &w, &h, components, fp16, &dst, &bound, &code, &total, err);
    if (rc != 0) return rc;
    if (code != exrw::kOk) {
        if (code == -100) err = "icx_exr_save_to_memory: the file exceeds its bound";
        return code;
    }
    uint8_t* host = (uint8_t*)std::malloc(std::max<size_t>(1, total));
    if (!host || hipMemcpy(host, dst, total, hipMemcpyDeviceToHost) != hipSuccess) {
        std::free(host);
        (void)hipGetLastError();
        err = "icx_exr_save_to_memory: host allocation or copy failed";
        return -100;
    }
    *out = host;
    *size = total;
    return exrw::kOk;
}

}  // namespace icx
