// deflate_core_demo.cpp -- TEST PROGRAM for icx_deflate_core.h without a GPU (tests/test_deflate_core.py
// builds it with g++, plain and with -fsanitize=address,undefined): the serial part of the device
// deflate writer -- symbol counts, pad_block_counts, huff_lengths, canon_codes, BitW, token_code --
// run over token slots the test supplies, one zlib stream per job.
//
//   deflate_core_demo <jobs> <streams>
// jobs:    per job  int32 nslots, int32 nblocks, uint32 cap, int32 end[nblocks], uint16 slot[nslots]
//          (end[b]: the slot after block b's last; cap: scale the counts while the literal/length
//          total exceeds it, as k_exrw_huff does before it builds the codes; 0 = never)
// streams: per job  uint64 size, the zlib stream
// Every array the core writes is a heap block of exactly the size the kernels give it in LDS, so
// the sanitizer sees an index past any of them. Exit 3: huff_lengths gave other lengths from its own
// sort than from the order handed to it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "icx_deflate_core.h"

using namespace icx::deflate;

// rank_order (icx_deflate_wave.h) restated serially: the used symbols in (freq, symbol) ascending order.
static void rank_order_serial(const uint32_t* freq, int n, uint16_t* order) {
    for (int i = 0; i < n; ++i) {
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

// Thread 0's work in k_png_huff / k_exrw_huff, restated (it stays in those kernels, which call the
// core's huff_lengths / canon_codes / BitW as this does): both codes, the run-length coded lengths,
// the 7-bit code-length code and the header bits.
struct Work {
    std::vector<uint32_t> wt = std::vector<uint32_t>(2 * kNLL);
    std::vector<uint16_t> order = std::vector<uint16_t>(kNLL), order_d = std::vector<uint16_t>(kND);
    std::vector<int16_t> parent = std::vector<int16_t>(2 * kNLL);
    std::vector<uint8_t> l_ll = std::vector<uint8_t>(kNLL), l_d = std::vector<uint8_t>(kND);
    std::vector<uint8_t> rle_sym = std::vector<uint8_t>(kNLL + kND), rle_ext = std::vector<uint8_t>(kNLL + kND);
};
static void build_block(const uint32_t* f_ll, const uint32_t* f_d, bool bfinal, Work& S, BlockCodes& B) {
    uint8_t* l_ll = S.l_ll.data();
    uint8_t* l_d = S.l_d.data();
    uint8_t* rle_sym = S.rle_sym.data();
    uint8_t* rle_ext = S.rle_ext.data();
    uint16_t* order = S.order.data();
    uint16_t* order_d = S.order_d.data();
    uint32_t* wt = S.wt.data();
    int16_t* parent = S.parent.data();
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
    int ns = 0;
    const int tot = hlit + hdist;
    auto L = [&](int i) { return i < hlit ? l_ll[i] : l_d[i - hlit]; };
    for (int i = 0; i < tot;) {
        const int cur = L(i);
        int run = 1;
        while (i + run < tot && L(i + run) == cur) ++run;
        int left = run;
        if (cur == 0) {
            while (left >= 11) {
                const int r = left < 138 ? left : 138;
                rle_sym[ns] = 18;
                rle_ext[ns++] = (uint8_t)(r - 11);
                left -= r;
            }
            if (left >= 3) {
                rle_sym[ns] = 17;
                rle_ext[ns++] = (uint8_t)(left - 3);
                left = 0;
            }
            while (left > 0) {
                rle_sym[ns] = 0;
                rle_ext[ns++] = 0;
                --left;
            }
        } else {
            rle_sym[ns] = (uint8_t)cur;
            rle_ext[ns++] = 0;
            --left;
            while (left >= 3) {
                const int r = left < 6 ? left : 6;
                rle_sym[ns] = 16;
                rle_ext[ns++] = (uint8_t)(r - 3);
                left -= r;
            }
            while (left > 0) {
                rle_sym[ns] = (uint8_t)cur;
                rle_ext[ns++] = 0;
                --left;
            }
        }
        i += run;
    }
    uint32_t f_cl[19];
    for (int i = 0; i < 19; ++i) f_cl[i] = 0;
    for (int i = 0; i < ns; ++i) ++f_cl[rle_sym[i]];
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
    bw.put(bfinal ? 1u : 0u, 1);  // BFINAL
    bw.put(2u, 2);                // BTYPE = dynamic
    bw.put((uint32_t)(hlit - 257), 5);
    bw.put((uint32_t)(hdist - 1), 5);
    bw.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) bw.put(l_cl[kClOrder[i]], 3);
    for (int i = 0; i < ns; ++i) {
        const int s = rle_sym[i];
        bw.put(c_cl[s], l_cl[s]);
        if (s == 16) bw.put(rle_ext[i], 2);
        else if (s == 17) bw.put(rle_ext[i], 3);
        else if (s == 18) bw.put(rle_ext[i], 7);
    }
    B.hdr_bits = bw.n;
}

static bool read_all(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: deflate_core_demo <jobs> <streams>\n");
        return 2;
    }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in)) return 2;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    size_t at = 0;
    while (at < in.size()) {
        int32_t nslots, nblocks;
        uint32_t cap;
        memcpy(&nslots, &in[at], 4);
        memcpy(&nblocks, &in[at + 4], 4);
        memcpy(&cap, &in[at + 8], 4);
        at += 12;
        std::vector<int32_t> end(nblocks);
        memcpy(end.data(), &in[at], 4 * (size_t)nblocks);
        at += 4 * (size_t)nblocks;
        std::vector<uint16_t> T(nslots);
        memcpy(T.data(), &in[at], 2 * (size_t)nslots);
        at += 2 * (size_t)nslots;

        // the stream's words: at most 48 bits a token, a header and an end-of-block code a block
        std::vector<uint32_t> words(((size_t)nslots * 48 + (size_t)nblocks * (kHdrWords * 32 + 15)) / 32 + 2, 0u);
        BitW bw{words.data()};
        std::vector<uint8_t> bytes;  // the tokens applied, for the Adler-32
        std::vector<uint32_t> f_ll(kNLL), f_d(kND);
        std::vector<uint8_t> own_ll(kNLL), own_d(kND);
        Work S;
        int32_t s0 = 0;
        for (int32_t b = 0; b < nblocks; ++b) {
            const int32_t s1 = end[b];
            std::fill(f_ll.begin(), f_ll.end(), 0u);
            std::fill(f_d.begin(), f_d.end(), 0u);
            for (int32_t i = s0; i < s1; ++i) {
                const uint32_t t = T[i];
                if (t < 256) {
                    ++f_ll[t];
                } else if (!(t & 0x8000u)) {
                    ++f_ll[257 + len_code((int)(t & 255) + 3)];
                    ++f_d[dist_code((int)(T[i + 1] & 0x7FFFu) + 1)];
                }
            }
            ++f_ll[256];  // EOB
            if (cap) {  // k_exrw_huff's scaling, in front of the padding
                uint64_t tot = 0;
                for (int i = 0; i < kNLL; ++i) tot += f_ll[i];
                int sh = 0;
                while ((tot >> sh) > cap) ++sh;
                if (sh) {
                    for (int i = 0; i < kNLL; ++i)
                        if (f_ll[i]) f_ll[i] = f_ll[i] >> sh ? f_ll[i] >> sh : 1u;
                    for (int i = 0; i < kND; ++i)
                        if (f_d[i]) f_d[i] = f_d[i] >> sh ? f_d[i] >> sh : 1u;
                }
            }
            pad_block_counts(f_ll.data(), f_d.data());
            rank_order_serial(f_ll.data(), kNLL, S.order.data());
            rank_order_serial(f_d.data(), kND, S.order_d.data());
            BlockCodes B;
            memset(&B, 0, sizeof B);
            build_block(f_ll.data(), f_d.data(), b == nblocks - 1, S, B);
            // the same lengths from huff_lengths' own sort (order / order_d are free again)
            huff_lengths(f_ll.data(), kNLL, 15, own_ll.data(), S.order.data(), S.wt.data(), S.parent.data(), false);
            huff_lengths(f_d.data(), kND, 15, own_d.data(), S.order_d.data(), S.wt.data(), S.parent.data(), false);
            if (own_ll != S.l_ll || own_d != S.l_d) {
                fprintf(stderr, "block %d: presorted and sorted code lengths differ\n", b);
                return 3;
            }
            for (uint32_t i = 0; i * 32 < B.hdr_bits; ++i) {
                const int n = B.hdr_bits - i * 32 < 32 ? (int)(B.hdr_bits - i * 32) : 32;
                bw.put(n == 32 ? B.hdr[i] : (B.hdr[i] & ((1u << n) - 1u)), n);
            }
            for (int32_t i = s0; i < s1; ++i) {
                int nb = 0;
                const uint64_t v = token_code(B, T[i], i + 1 < s1 ? T[i + 1] : 0u, nb);
                bw.put((uint32_t)v, nb < 32 ? nb : 32);
                if (nb > 32) bw.put((uint32_t)(v >> 32), nb - 32);
                const uint32_t t = T[i];
                if (t < 256) {
                    bytes.push_back((uint8_t)t);
                } else if (!(t & 0x8000u)) {
                    const size_t len = (t & 255) + 3, dist = (size_t)(T[i + 1] & 0x7FFFu) + 1;
                    for (size_t k = 0; k < len; ++k) bytes.push_back(bytes[bytes.size() - dist]);
                }
            }
            bw.put(B.ll_code[256], B.ll_len[256]);
            s0 = s1;
        }
        uint32_t a1 = 1, a2 = 0;
        for (uint8_t c : bytes) {
            a1 = (a1 + c) % kAdlerMod;
            a2 = (a2 + a1) % kAdlerMod;
        }
        std::vector<uint8_t> z = {0x78, 0x01};
        for (uint32_t i = 0; i < (bw.n + 7) / 8; ++i) z.push_back((uint8_t)(words[i >> 2] >> (8 * (i & 3))));
        const uint32_t adler = a2 << 16 | a1;
        for (int k = 3; k >= 0; --k) z.push_back((uint8_t)(adler >> (8 * k)));
        const uint64_t size = z.size();
        fwrite(&size, 8, 1, out);
        fwrite(z.data(), 1, z.size(), out);
    }
    fclose(out);
    return 0;
}
