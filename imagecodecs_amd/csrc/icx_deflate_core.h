// icx_deflate_core.h -- the serial part of the device deflate writer, host and device: the RFC 1951
// tables, a block's code tables (BlockCodes), length-limited Huffman code lengths, canonical codes,
// the header's bit writer, and a token slot's bits. One text for the PNG encoder (icx_png.hip),
// the OpenEXR ZIP write (icx_exrw.hip) and the TIFF Deflate strips (icx_tiffw.hip); the wave-level
// part is icx_deflate_wave.h. Plain C++: the
// CPU test builds it with g++ (tests/test_deflate_core.py), the two writers with hipcc. Their bytes
// are pinned by tests/test_gpu_deflate_pin.py.
//
// Not here: the sequence that calls these for one block (thread 0 of k_png_huff / k_exrw_huff /
// k_tiffw_huff: both codes, the run-length coded lengths, the 7-bit code, the header bits). As a
// function of its own it is simplified before it is inlined, with pointers of unknown address
// space, and the PNG and EXR kernels compiled to other code (one or two more VGPRs, 14 % more
// instructions), so it stays in them, and the TIFF kernel carries the same text.
//
// Token slots (uint16): a literal is its byte value (< 256); a match is a length slot
// 0x4000 | (len - 3) followed by a distance slot 0x8000 | (dist - 1).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_DEFLATE_HD __host__ __device__ inline
#else
#define ICX_DEFLATE_HD inline
#endif

namespace icx {
namespace deflate {

constexpr int kNLL = 286, kND = 30;   // literal/length and distance alphabets
constexpr int kHdrWords = 96;         // per-block header bit buffer (<= 3072 bits)
constexpr uint32_t kAdlerMod = 65521;

// ---- deflate tables (RFC 1951 3.2.5), one text for every translation unit: in device code
// __constant__ memory, as they were in each writer, and plain constants everywhere else.
#if defined(__HIP_DEVICE_COMPILE__)
#define ICX_DEFLATE_TABLE inline __constant__
#else
#define ICX_DEFLATE_TABLE static constexpr
#endif
ICX_DEFLATE_TABLE uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
                                           35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
ICX_DEFLATE_TABLE uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
ICX_DEFLATE_TABLE uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769,
                                            1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
ICX_DEFLATE_TABLE uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
ICX_DEFLATE_TABLE uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

ICX_DEFLATE_HD int len_code(int len) {  // 3..258 -> 0..28
    int c = 0;
    while (c < 28 && kLenBase[c + 1] <= len) ++c;
    return c;
}
ICX_DEFLATE_HD int dist_code(int d) {  // 1..32768 -> 0..29
    int c = 0;
    while (c < 29 && kDistBase[c + 1] <= d) ++c;
    return c;
}

struct BlockCodes {
    uint16_t ll_code[kNLL];  // bit-reversed (LSB-first emission)
    uint8_t ll_len[kNLL];
    uint16_t d_code[kND];
    uint8_t d_len[kND];
    uint32_t hdr[kHdrWords];  // header bits, LSB-first
    uint32_t hdr_bits;
    uint32_t pad_;
};
static_assert(sizeof(BlockCodes) % 4 == 0, "staged a dword at a time");

// Code lengths for freq[0..n) limited to maxbits (Huffman by sorting + JPEG Annex K.3 "adjust
// bits" length limiting, which keeps the code complete). Single thread.
// presorted: order[] already holds the used symbols sorted by (freq, symbol) ascending.
ICX_DEFLATE_HD void huff_lengths(const uint32_t* freq, int n, int maxbits, uint8_t* len, uint16_t* order, uint32_t* wt,
                                 int16_t* parent, bool presorted) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (freq[i]) {
            if (!presorted) order[m] = (uint16_t)i;
            ++m;
        }
    }
    if (m == 0) return;
    if (m == 1) {
        len[order[0]] = 1;
        return;
    }
    // insertion sort by (freq, symbol) ascending
    for (int a = 1; a < m && !presorted; ++a) {
        const uint16_t v = order[a];
        int b = a - 1;
        while (b >= 0 && (freq[order[b]] > freq[v] || (freq[order[b]] == freq[v] && order[b] > v))) {
            order[b + 1] = order[b];
            --b;
        }
        order[b + 1] = v;
    }
    // two-queue Huffman: leaves 0..m-1 (sorted), internal nodes m..2m-2
    for (int i = 0; i < m; ++i) wt[i] = freq[order[i]];
    int li = 0, ii = m, in_end = m;
    for (int k = 0; k < m - 1; ++k) {
        int pick[2];
        for (int q = 0; q < 2; ++q) {
            if (li < m && (ii >= in_end || wt[li] <= wt[ii])) pick[q] = li++;
            else pick[q] = ii++;
        }
        wt[in_end] = wt[pick[0]] + wt[pick[1]];
        parent[pick[0]] = (int16_t)in_end;
        parent[pick[1]] = (int16_t)in_end;
        ++in_end;
    }
    // depths top-down (a parent always has a larger index than its children); wt is reused
    uint32_t* dep = wt;
    dep[in_end - 1] = 0;
    for (int k = in_end - 2; k >= 0; --k) dep[k] = dep[parent[k]] + 1;
    int bl[40];
    for (int i = 0; i < 40; ++i) bl[i] = 0;
    int maxd = 0;
    for (int i = 0; i < m; ++i) {
        const int dd = dep[i] > 39 ? 39 : (int)dep[i];
        ++bl[dd];
        maxd = dd > maxd ? dd : maxd;
    }
    for (int i = maxd; i > maxbits; --i) {  // Annex K.3 Adjust_BITS
        while (bl[i] > 0) {
            int j = i - 2;
            while (j > 1 && bl[j] == 0) --j;
            bl[i] -= 2;
            bl[i - 1] += 1;
            bl[j + 1] += 2;
            bl[j] -= 1;
        }
    }
    // most frequent symbols get the shortest codes: walk sorted order from the top
    int k = m - 1;
    for (int l = 1; l <= maxbits; ++l)
        for (int c = 0; c < bl[l]; ++c) len[order[k--]] = (uint8_t)l;
}

ICX_DEFLATE_HD uint32_t bit_reverse(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
#endif
}

ICX_DEFLATE_HD void canon_codes(const uint8_t* len, int n, uint16_t* code) {  // RFC 1951 3.2.2, bit-reversed
    int bl[16] = {0};
    for (int i = 0; i < n; ++i) ++bl[len[i]];
    bl[0] = 0;
    int next[16];
    int c = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + bl[b - 1]) << 1;
        next[b] = c;
    }
    for (int i = 0; i < n; ++i) {
        const int l = len[i];
        code[i] = 0;
        if (!l) continue;
        const uint32_t v = (uint32_t)next[l]++;
        code[i] = (uint16_t)(bit_reverse(v) >> (32 - l));
    }
}

struct BitW {
    uint32_t* w;     // zeroed words
    uint32_t n = 0;  // bits written
    ICX_DEFLATE_HD void put(uint32_t v, int nb) {
        if (!nb) return;
        const uint32_t s = n & 31;
        w[n >> 5] |= v << s;
        if (s + nb > 32) w[(n >> 5) + 1] |= v >> (32 - s);
        n += nb;
    }
};

// At least two codes per tree keeps every code complete: a block's summed counts get the missing
// ones. Single thread, before the symbols are ordered (the padding adds used symbols).
ICX_DEFLATE_HD void pad_block_counts(uint32_t* f_ll, uint32_t* f_d) {
    int u = 0;
    for (int i = 0; i < kNLL; ++i) u += f_ll[i] != 0;
    if (u < 2) f_ll[f_ll[0] ? 1 : 0] = 1;
    u = 0;
    for (int i = 0; i < kND; ++i) u += f_d[i] != 0;
    if (u < 2) {
        if (!f_d[0]) f_d[0] = 1;
        if (!f_d[1]) f_d[1] = 1;
    }
}

// Token slot -> (bits, count), LSB-first: a literal; or, at a match's length slot, code, length
// extra, distance code, distance extra (at most 15 + 5 + 15 + 13 = 48 bits); a distance slot
// emits nothing (its match's length slot took it).
ICX_DEFLATE_HD uint64_t token_code(const BlockCodes& B, uint32_t t, uint32_t tnext, int& nb) {
    if (t < 256) {
        nb = B.ll_len[t];
        return B.ll_code[t];
    }
    if (t & 0x8000u) {
        nb = 0;
        return 0;
    }
    const int len = (int)(t & 255) + 3, dist = (int)(tnext & 0x7FFFu) + 1;
    const int lc = len_code(len), dc = dist_code(dist);
    uint64_t v = B.ll_code[257 + lc];
    int n = B.ll_len[257 + lc];
    v |= (uint64_t)(len - kLenBase[lc]) << n;
    n += kLenExtra[lc];
    v |= (uint64_t)B.d_code[dc] << n;
    n += B.d_len[dc];
    v |= (uint64_t)(dist - kDistBase[dc]) << n;
    nb = n + kDistExtra[dc];
    return v;
}

}  // namespace deflate
}  // namespace icx
