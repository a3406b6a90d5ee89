// icx_gifw_core.h -- the serial part of the GIF write (contract: include/icx.h, "GIF write"), host
// and device: the argument checks and the segment geometry, the bound, the cube's arithmetic, the
// container's bytes from the table bits and the payload's size, the LZW dictionary and state
// machine, and (host only) a serial writer of the whole file. Plain C++: the CPU test builds it
// with g++ (tests/cxx/gifw_core_demo.cpp) and compares it with tests/gifwutil.py; icx_gifw.hip
// builds its kernels from the same text and is compared with the same restatement on the GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "icx_gif_core.h"

namespace icx {

constexpr int kGifInvalidArgument = 7;  // ICX_GIF_INVALID_ARGUMENT
constexpr int kGifwAuto = 0, kGifwCube = 1;  // ICX_GIF_PALETTE_*
constexpr int kGifwDefaultSeg = 65536;       // segment_pixels = 0
constexpr int kGifwMinSeg = 64;
constexpr int kGifwFill = 3838;              // codes a table fill needs at least: 4094 - 256

struct GifwGeom {
    int32_t w, h, d;
    int32_t dither, mode;
    int64_t N;     // pixels
    int64_t seg;   // pixels per segment (the last one may be shorter), 1 <= seg <= N
    int64_t nseg;
};

// The geometry of a write, or false for arguments the contract refuses.
ICX_GIF_HD bool gifw_geom(int w, int h, int d, int segment_pixels, int dither, int palette_mode, GifwGeom* out) {
    if (!(d == 1 || d == 3 || d == 4) || w < 1 || h < 1 || w > 65535 || h > 65535) return false;
    if (!(dither == 0 || dither == 1) || !(palette_mode == kGifwAuto || palette_mode == kGifwCube)) return false;
    if (segment_pixels < -1 || (segment_pixels > 0 && segment_pixels < kGifwMinSeg)) return false;
    const int64_t N = (int64_t)w * h;
    if (N > (1ll << 30)) return false;
    GifwGeom g;
    g.w = w; g.h = h; g.d = d; g.dither = dither; g.mode = palette_mode;
    g.N = N;
    int64_t seg = segment_pixels == 0 ? kGifwDefaultSeg : segment_pixels < 0 ? N : segment_pixels;
    if (seg > N) seg = N;
    g.seg = seg;
    g.nseg = (N + seg - 1) / seg;
    *out = g;
    return true;
}

// An upper bound of the code stream of a segment-cut image of N pixels in nseg segments, in codes:
//   every code but a Clear and the stop code stands for at least one pixel: at most N of them;
//   one Clear leads the stream and one Clear or the stop code ends each segment: 1 + nseg;
//   a table-full Clear follows the code that adds entry 4095. The first free entry is at most 258,
//   every code but a segment's first adds one entry, so at least 4096 - 258 = 3838 codes of the
//   segment, each a pixel or more, come between two of them (and before the first): a segment of
//   n pixels has at most floor(n / 3838) of them, all segments together at most floor(N / 3838).
// Each code is at most 12 bits; zero bits fill the last byte. The file around the payload of P
// bytes: 13 bytes of header and screen descriptor, a table of at most 768 bytes, 10 bytes of image
// descriptor, the code size byte, ceil(P / 255) sub-block length bytes, the terminator and ';'.
ICX_GIF_HD uint64_t gifw_code_bound(uint64_t N, uint64_t nseg) { return N + nseg + 1 + N / kGifwFill; }
ICX_GIF_HD uint64_t gifw_payload_bound(uint64_t N, uint64_t nseg) { return (12 * gifw_code_bound(N, nseg) + 7) / 8; }
ICX_GIF_HD uint64_t gifw_data_size(uint64_t P) { return P + (P + 254) / 255; }  // payload and length bytes
ICX_GIF_HD uint64_t gifw_head_size(int tb) { return 13 + (3ull << tb) + 10 + 1; }
ICX_GIF_HD uint64_t gifw_file_size(int tb, uint64_t P) { return gifw_head_size(tb) + gifw_data_size(P) + 2; }
// The largest file the write can make (0: refused arguments). Independent of d and the content.
ICX_GIF_HD uint64_t gifw_bound(int w, int h, int segment_pixels) {
    GifwGeom g;
    if (!gifw_geom(w, h, 1, segment_pixels, 0, kGifwAuto, &g)) return 0;
    return gifw_file_size(8, gifw_payload_bound((uint64_t)g.N, (uint64_t)g.nseg));
}
// Room for one segment's bit string (segment 0 carries the leading Clear).
ICX_GIF_HD uint64_t gifw_segment_room(uint64_t seg) { return gifw_payload_bound(seg, 1); }

// ---- palette
// A pixel's colour as R << 16 | G << 8 | B; d = 1: grey v is v, v, v; d = 4: alpha is ignored.
ICX_GIF_HD uint32_t gifw_key(const uint8_t* px, int d, int64_t p) {
    if (d == 1) return (uint32_t)px[p] * 0x010101u;
    const uint8_t* q = px + p * d;
    return (uint32_t)q[0] << 16 | (uint32_t)q[1] << 8 | q[2];
}
// Table bits for n distinct colours (exact mode): max(1, ceil(log2 n)).
ICX_GIF_HD int gifw_table_bits(int n) {
    int tb = 1;
    while ((1 << tb) < n) ++tb;
    return tb;
}
// The cube: 6 x 7 x 6 levels of R, G, B.
constexpr int kGifwCubeR = 6, kGifwCubeG = 7, kGifwCubeB = 6, kGifwCubeSize = 252;
ICX_GIF_HD uint32_t gifw_level_value(int k, int L) { return (uint32_t)((255 * k + (L - 1) / 2) / (L - 1)); }
ICX_GIF_HD int gifw_level(uint32_t c, int L, int T) { return (int)((32u * c * (uint32_t)(L - 1) + 255u * (uint32_t)T) / 8160u); }
ICX_GIF_HD int gifw_threshold(int x, int y, int dither) {
    const int B4[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};
    return dither ? 2 * B4[(y & 3) * 4 + (x & 3)] + 1 : 16;
}
ICX_GIF_HD int gifw_cube_index(uint32_t key, int x, int y, int dither) {
    const int T = gifw_threshold(x, y, dither);
    const int kr = gifw_level(key >> 16, kGifwCubeR, T), kg = gifw_level((key >> 8) & 255u, kGifwCubeG, T),
              kb = gifw_level(key & 255u, kGifwCubeB, T);
    return (kr * kGifwCubeG + kg) * kGifwCubeB + kb;
}
// Entry i of the cube's table as a key (252..255: black).
ICX_GIF_HD uint32_t gifw_cube_entry(int i) {
    if (i >= kGifwCubeSize) return 0;
    const int kr = i / (kGifwCubeG * kGifwCubeB), kg = (i / kGifwCubeB) % kGifwCubeG, kb = i % kGifwCubeB;
    return gifw_level_value(kr, kGifwCubeR) << 16 | gifw_level_value(kg, kGifwCubeG) << 8 | gifw_level_value(kb, kGifwCubeB);
}

// ---- container
// Byte i of the file's first gifw_head_size(tb) bytes: signature, screen descriptor, the table
// (table: 3 << tb bytes), the image descriptor and the code size byte.
ICX_GIF_HD uint32_t gifw_head_byte(uint32_t i, int w, int h, int tb, int m, const uint8_t* table) {
    const uint32_t tbytes = 3u << tb;
    if (i < 13) {
        const uint8_t hd[13] = {'G', 'I', 'F', '8', '9', 'a', (uint8_t)w, (uint8_t)(w >> 8), (uint8_t)h, (uint8_t)(h >> 8),
                                (uint8_t)(0x80 | (tb - 1) << 4 | (tb - 1)), 0, 0};
        return hd[i];
    }
    if (i < 13 + tbytes) return table[i - 13];
    const uint8_t de[11] = {',', 0, 0, 0, 0, (uint8_t)w, (uint8_t)(w >> 8), (uint8_t)h, (uint8_t)(h >> 8), 0, (uint8_t)m};
    return de[i - 13 - tbytes];
}
// Byte q of the data area (the sub-blocks of a payload of P bytes, q < gifw_data_size(P)): a length
// byte, or payload(j).
template <class Payload>
ICX_GIF_HD uint32_t gifw_data_byte(uint64_t q, uint64_t P, Payload payload) {
    const uint64_t blk = q >> 8, r = q & 255u;
    if (r == 0) {
        const uint64_t left = P - 255 * blk;
        return (uint32_t)(left < 255 ? left : 255);
    }
    return payload(255 * blk + r - 1);
}

// ---- LZW: the dictionary (prefix code, index) -> code as an open-addressed table of kGifwLzwSlots
// words (key << 12 | code, all ones: free). Between two Clears at most 4096 - 6 = 4090 entries are
// made, so the table is never more than half full. (A prefix is below 4095, so no entry is all ones.)
constexpr int kGifwLzwBits = 13, kGifwLzwSlots = 1 << kGifwLzwBits;
constexpr uint32_t kGifwLzwFree = 0xFFFFFFFFu;

// The chain's state between indices, for one segment: it starts where a Clear leaves the decoder.
// sink(code, width) takes the stream's codes in order, each as wide as the decoder expects it: the
// width rule follows the decoder's table, which trails the coder's by one entry. feed() returns
// true when it wrote a Clear (the table was full): the caller then frees every slot of the
// dictionary before the next feed. writer: this caller's stores to the dictionary count (the
// kernel's lanes run the same chain, lane 0 alone stores).
struct GifwLzw {
    int m = 8, clear = 256;
    int width = 9;   // of the next code
    int dnext = 258; // the decoder's next free entry
    bool prev = false;  // the decoder has a previous code since the last Clear
    int next = 258;  // the coder's next free entry
    int cur = -1;    // the string matched so far

    ICX_GIF_HD void init(int mcs) {
        m = mcs;
        clear = 1 << mcs;
        reset();
        cur = -1;
    }
    ICX_GIF_HD void reset() {
        width = m + 1;
        dnext = next = clear + 2;
        prev = false;
    }
    template <class Sink>
    ICX_GIF_HD void emit(uint32_t code, Sink& sink) {
        sink(code, width);
        if ((int)code == clear) {
            reset();
        } else if ((int)code != clear + 1) {
            if (prev && dnext < 4096) {
                ++dnext;
                if (dnext == (1 << width) && width < 12) ++width;
            }
            prev = true;
        }
    }
    // The Clear that leads the whole stream (before segment 0).
    template <class Sink>
    ICX_GIF_HD void begin(Sink& sink) { emit((uint32_t)clear, sink); }
    template <class Sink>
    ICX_GIF_HD bool feed(uint32_t* dict, uint32_t b, Sink& sink, bool writer = true) {
        if (cur < 0) {
            cur = (int)b;
            return false;
        }
        const uint32_t key = (uint32_t)cur << 8 | b;
        uint32_t h = (key * 2654435761u) >> (32 - kGifwLzwBits);
        for (;;) {
            const uint32_t e = dict[h];
            if (e == kGifwLzwFree) break;
            if ((e >> 12) == key) {
                cur = (int)(e & 0xFFFu);
                return false;
            }
            h = (h + 1) & (kGifwLzwSlots - 1);
        }
        emit((uint32_t)cur, sink);
        cur = (int)b;
        if (next == 4095) {  // this code adds entry 4095: the table is full, nothing will use the entry
            emit((uint32_t)clear, sink);
            return true;
        }
        if (writer) dict[h] = key << 12 | (uint32_t)next;
        ++next;
        return false;
    }
    // The segment's end: the pending code, then a Clear, or the stop code after the last segment.
    template <class Sink>
    ICX_GIF_HD void finish(Sink& sink, bool last_segment) {
        if (cur >= 0) emit((uint32_t)cur, sink);
        cur = -1;
        emit((uint32_t)(last_segment ? clear + 1 : clear), sink);
    }
};

// Codes into bytes, LSB first, serially; close() pads the last byte with zero bits.
struct GifwBits {
    uint32_t acc = 0;
    int nacc = 0;  // bits waiting in acc (< 8 between calls)
    template <class Out>
    ICX_GIF_HD void put(uint32_t code, int width, Out& out) {
        acc |= code << nacc;
        nacc += width;
        while (nacc >= 8) {
            out((uint8_t)acc);
            acc >>= 8;
            nacc -= 8;
        }
    }
    template <class Out>
    ICX_GIF_HD void close(Out& out) {
        if (nacc > 0) out((uint8_t)acc);
        acc = 0;
        nacc = 0;
    }
};

// The payload of the index plane idx(0 .. N-1) cut into segments of g.seg -> its size in bytes.
// dict: kGifwLzwSlots words. seg_bits (may be null): the bit offset of each segment's string in
// the stream (segment 0's starts with the leading Clear, at 0).
template <class In, class Out>
ICX_GIF_HD uint64_t gifw_lzw_encode(uint32_t* dict, const GifwGeom& g, int m, In idx, Out put_byte, uint64_t* seg_bits = nullptr) {
    uint64_t size = 0, nbits = 0;
    auto out = [&](uint8_t v) {
        put_byte(v);
        ++size;
    };
    GifwBits bits;
    auto sink = [&](uint32_t code, int width) {
        bits.put(code, width, out);
        nbits += (uint64_t)width;
    };
    for (int64_t s = 0; s < g.nseg; ++s) {
        if (seg_bits) seg_bits[s] = nbits;
        GifwLzw z;
        z.init(m);
        for (int k = 0; k < kGifwLzwSlots; ++k) dict[k] = kGifwLzwFree;
        if (s == 0) z.begin(sink);
        const int64_t p0 = s * g.seg, p1 = p0 + g.seg < g.N ? p0 + g.seg : g.N;
        for (int64_t p = p0; p < p1; ++p)
            if (z.feed(dict, idx(p), sink))
                for (int k = 0; k < kGifwLzwSlots; ++k) dict[k] = kGifwLzwFree;
        z.finish(sink, s == g.nseg - 1);
    }
    bits.close(out);
    return size;
}

// The whole file, serially, on the host (the CPU tests' side of the contract). seg_bits as above.
inline std::vector<uint8_t> gifw_write_serial(const uint8_t* px, const GifwGeom& g, std::vector<uint64_t>* seg_bits = nullptr) {
    std::vector<uint32_t> keys((size_t)g.N);
    for (int64_t p = 0; p < g.N; ++p) keys[(size_t)p] = gifw_key(px, g.d, p);
    std::vector<uint32_t> set(keys);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    const bool cube = g.mode == kGifwCube || set.size() > 256;
    const int tb = cube ? 8 : gifw_table_bits((int)set.size()), m = tb < 2 ? 2 : tb;
    std::vector<uint8_t> table((size_t)3 << tb, 0), plane((size_t)g.N);
    for (int i = 0; i < (1 << tb); ++i) {
        const uint32_t k = cube ? gifw_cube_entry(i) : (size_t)i < set.size() ? set[(size_t)i] : 0u;
        table[3 * i] = (uint8_t)(k >> 16);
        table[3 * i + 1] = (uint8_t)(k >> 8);
        table[3 * i + 2] = (uint8_t)k;
    }
    for (int64_t p = 0; p < g.N; ++p) {
        const uint32_t k = keys[(size_t)p];
        plane[(size_t)p] = cube ? (uint8_t)gifw_cube_index(k, (int)(p % g.w), (int)(p / g.w), g.dither)
                                : (uint8_t)(std::lower_bound(set.begin(), set.end(), k) - set.begin());
    }
    std::vector<uint32_t> dict(kGifwLzwSlots);
    std::vector<uint8_t> payload;
    if (seg_bits) seg_bits->assign((size_t)g.nseg, 0);
    const uint64_t P = gifw_lzw_encode(dict.data(), g, m, [&](int64_t p) { return (uint32_t)plane[(size_t)p]; },
                                       [&](uint8_t v) { payload.push_back(v); }, seg_bits ? seg_bits->data() : nullptr);
    std::vector<uint8_t> file;
    const uint32_t head = (uint32_t)gifw_head_size(tb);
    for (uint32_t i = 0; i < head; ++i) file.push_back((uint8_t)gifw_head_byte(i, g.w, g.h, tb, m, table.data()));
    const uint64_t D = gifw_data_size(P);
    for (uint64_t q = 0; q < D; ++q) file.push_back((uint8_t)gifw_data_byte(q, P, [&](uint64_t j) { return (uint32_t)payload[(size_t)j]; }));
    file.push_back(0);
    file.push_back(';');
    return file;
}

}  // namespace icx
