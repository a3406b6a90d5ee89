// icx_tiffw_core.h -- the serial part of the TIFF write (contract: include/icx.h, "TIFF write"),
// host and device: the argument checks and the geometry, the bound, the file's layout and its
// header / array / IFD bytes from the strips' sizes, the predictor as a gather from the pixels, a
// serial LZW encoder and a serial PackBits packer. Plain C++: the CPU test builds it with g++
// (tests/cxx/tiffw_core_demo.cpp) and compares it with tests/tiffwutil.py; icx_tiffw.hip builds its
// kernels from the same text (geometry, layout, IFD bytes, the gather, the LZW dictionary and state
// machine) and is compared with the same restatement on the GPU.
#pragma once
#include <cstdint>

#include "icx_tiff_core.h"

namespace icx {

constexpr int kTiffInvalidArgument = 8;  // ICX_TIFF_INVALID_ARGUMENT
constexpr int kTiffwNone = 1, kTiffwLzw = 5, kTiffwDeflate = 8, kTiffwPackBits = 32773;
constexpr int kTiffwLzwClearAt = 3836;   // a Clear follows the 3836th code since the last one
constexpr int kTiffwSeg = 4096;          // deflate: LZ77 / emit segment
constexpr int kTiffwBlockSegs = 16;      // deflate: segments per block at most
constexpr int kTiffwHdrBytes = 384;      // deflate: a dynamic block header's buffer (deflate::kHdrWords * 4)

struct TiffwGeom {
    int32_t w, h, d, comp, pred;
    int32_t rps;      // rows per strip, clamped to h
    int32_t nstrips;
    int32_t rb;       // row bytes
};

ICX_TIFF_HD int tiffw_strip_rows(const TiffwGeom& g, int k) {
    const int64_t left = (int64_t)g.h - (int64_t)k * g.rps;
    return (int)(left < g.rps ? left : g.rps);
}
// Deflate blocks of a strip of S bytes: near-equal runs of at most kTiffwBlockSegs segments.
ICX_TIFF_HD int tiffw_deflate_blocks(uint64_t S) {
    const uint64_t nseg = (S + kTiffwSeg - 1) / kTiffwSeg;
    return (int)((nseg + kTiffwBlockSegs - 1) / kTiffwBlockSegs);
}

// An upper bound of a strip's payload, `rows` rows of rb bytes (S = rows * rb):
//   none      S, exactly.
//   PackBits  per row rb + ceil(rb / 128). A row is L literal bytes in m stretches and R repeat
//             packets of >= 3 bytes each (rb >= L + 3R); a stretch of L_i bytes costs L_i +
//             ceil(L_i / 128), a repeat packet 2. There are at most R + 1 stretches and
//             ceil(a) + ceil(b) <= ceil(a + b) + 1, so the headers are at most ceil(L / 128) + R and
//             the row costs at most L + ceil(L / 128) + 3R <= rb + ceil(rb / 128).
//   LZW       every code covers at least one byte: at most S codes, a Clear after each 3836 of
//             them, the leading Clear and the EOI, each of at most 12 bits, then zero bits to the
//             byte: ceil(12 * (S + floor(S / 3836) + 2) / 8).
//   Deflate   2 + 4 bytes of zlib framing; per block kTiffwHdrBytes (the whole header buffer) and
//             the end-of-block code (<= 15 bits); the tokens: with a flat 9-bit literal/length code
//             (286 <= 512) and a flat 5-bit distance code (30 <= 32) a literal costs 9 bits and a
//             match 14 bits plus its extra bits (length: none up to 10 bytes, at most 5 from 11
//             on; distance: none up to 4, at most 10 up to 4096, at most 13 beyond). The matches
//             the parse keeps are 3 bytes or more at distance <= 2 (14 bits), 4 or more at
//             distance <= 4096 (24 bits, 29 from 11 bytes on) and 5 or more beyond (27 bits, 32
//             from 11 bytes on): never more than 9 bits per byte covered.
//             A Huffman-optimal code costs no more than the flat one, and
//             the length limiter's documented worst ratio over the optimum is 1.000036
//             (tests/deflate_read.py LIMITER_WORST); 1/1024 is allowed here.
ICX_TIFF_HD uint64_t tiffw_payload_bound(const TiffwGeom& g, int rows) {
    const uint64_t rb = (uint64_t)g.rb, S = rb * (uint64_t)rows;
    switch (g.comp) {
    case kTiffwNone: return S;
    case kTiffwPackBits: return (uint64_t)rows * (rb + (rb + 127) / 128);
    case kTiffwLzw: return (3 * (S + S / kTiffwLzwClearAt + 2) + 1) / 2;
    default: {
        const uint64_t nb = (uint64_t)tiffw_deflate_blocks(S);
        const uint64_t bits = 9 * S + (9 * S + 1023) / 1024 + 15 * nb;
        return 6 + nb * kTiffwHdrBytes + (bits + 7) / 8;
    }
    }
}

// The file's parts after the strips' data (data_end: the even offset after the last strip).
struct TiffwLayout {
    uint64_t bps_at, so_at, sc_at, ifd_at, total;
    int32_t nent;
};
ICX_TIFF_HD TiffwLayout tiffw_layout(const TiffwGeom& g, uint64_t data_end) {
    TiffwLayout L;
    L.bps_at = data_end;
    L.so_at = L.bps_at + (g.d >= 3 ? 2u * (uint32_t)g.d : 0u);
    L.sc_at = L.so_at + (g.nstrips > 1 ? 4ull * (uint64_t)g.nstrips : 0ull);
    L.ifd_at = L.sc_at + (g.nstrips > 1 ? 4ull * (uint64_t)g.nstrips : 0ull);
    L.nent = 10 + (g.pred == 2) + (g.d == 4);
    L.total = L.ifd_at + 2 + 12ull * (uint64_t)L.nent + 4;
    return L;
}

// The geometry of a write, or false for arguments the contract refuses.
ICX_TIFF_HD bool tiffw_geom(int w, int h, int d, int comp, int pred, int rows_per_strip, TiffwGeom* out) {
    if (!(d == 1 || d == 3 || d == 4) || w < 1 || h < 1 || rows_per_strip < 0) return false;
    if (!(comp == kTiffwNone || comp == kTiffwLzw || comp == kTiffwDeflate || comp == kTiffwPackBits)) return false;
    if (!(pred == 1 || (pred == 2 && (comp == kTiffwLzw || comp == kTiffwDeflate)))) return false;
    if ((int64_t)w * h > (1ll << 30)) return false;
    TiffwGeom g;
    g.w = w; g.h = h; g.d = d; g.comp = comp; g.pred = pred;
    g.rps = rows_per_strip == 0 || rows_per_strip > h ? h : rows_per_strip;
    const int64_t n = ((int64_t)h + g.rps - 1) / g.rps;
    if (n > kTiffMaxChunks) return false;
    g.nstrips = (int)n;
    if ((int64_t)w * d * g.rps >= (1ll << 31)) return false;
    g.rb = w * d;
    const uint64_t full = (tiffw_payload_bound(g, g.rps) + 1) & ~1ull;
    const uint64_t last = (tiffw_payload_bound(g, tiffw_strip_rows(g, g.nstrips - 1)) + 1) & ~1ull;
    if (tiffw_layout(g, 8 + full * (uint64_t)(g.nstrips - 1) + last).total >= (1ull << 32)) return false;
    *out = g;
    return true;
}
// The largest file the write can make (0: refused arguments).
ICX_TIFF_HD uint64_t tiffw_bound(int w, int h, int d, int comp, int pred, int rows_per_strip) {
    TiffwGeom g;
    if (!tiffw_geom(w, h, d, comp, pred, rows_per_strip, &g)) return 0;
    const uint64_t full = (tiffw_payload_bound(g, g.rps) + 1) & ~1ull;
    const uint64_t last = (tiffw_payload_bound(g, tiffw_strip_rows(g, g.nstrips - 1)) + 1) & ~1ull;
    return tiffw_layout(g, 8 + full * (uint64_t)(g.nstrips - 1) + last).total;
}

ICX_TIFF_HD void tiffw_le(uint8_t* p, uint32_t v, int n) {
    for (int k = 0; k < n; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
ICX_TIFF_HD void tiffw_header(uint8_t* p, const TiffwLayout& L) {
    p[0] = 'I'; p[1] = 'I'; p[2] = 42; p[3] = 0;
    tiffw_le(p + 4, (uint32_t)L.ifd_at, 4);
}
// The IFD (2 + 12 * nent + 4 bytes, at most 150) into p. off0 / cnt0: the one strip's offset and
// size when nstrips == 1.
constexpr int kTiffwIfdMax = 2 + 12 * 12 + 4;
ICX_TIFF_HD int tiffw_ifd(uint8_t* p, const TiffwGeom& g, const TiffwLayout& L, uint32_t off0, uint32_t cnt0) {
    int at = 2;
    auto entry = [&](int tag, int type, uint32_t count, uint32_t value) {
        tiffw_le(p + at, (uint32_t)tag, 2);
        tiffw_le(p + at + 2, (uint32_t)type, 2);
        tiffw_le(p + at + 4, count, 4);
        tiffw_le(p + at + 8, value, 4);  // (a SHORT sits in the low two bytes, the rest zero)
        at += 12;
    };
    const uint32_t n = (uint32_t)g.nstrips;
    tiffw_le(p, (uint32_t)L.nent, 2);
    entry(256, 4, 1, (uint32_t)g.w);
    entry(257, 4, 1, (uint32_t)g.h);
    entry(258, 3, (uint32_t)g.d, g.d == 1 ? 8u : (uint32_t)L.bps_at);
    entry(259, 3, 1, (uint32_t)g.comp);
    entry(262, 3, 1, g.d == 1 ? 1u : 2u);
    entry(273, 4, n, n == 1 ? off0 : (uint32_t)L.so_at);
    entry(277, 3, 1, (uint32_t)g.d);
    entry(278, 4, 1, (uint32_t)g.rps);
    entry(279, 4, n, n == 1 ? cnt0 : (uint32_t)L.sc_at);
    entry(284, 3, 1, 1);
    if (g.pred == 2) entry(317, 3, 1, 2);
    if (g.d == 4) entry(338, 3, 1, 2);
    tiffw_le(p + at, 0, 4);
    return at + 4;
}

// Byte i of the strip that starts at row y0: the pixel byte, or with predictor 2 its difference
// from the sample d bytes before it in the row.
ICX_TIFF_HD uint32_t tiffw_strip_byte(const uint8_t* px, const TiffwGeom& g, int y0, uint32_t i) {
    const uint32_t rb = (uint32_t)g.rb, row = i / rb, x = i - row * rb;
    const uint8_t* r = px + (uint64_t)((uint32_t)y0 + row) * rb;
    uint32_t v = r[x];
    if (g.pred == 2 && x >= (uint32_t)g.d) v = (v - r[x - g.d]) & 255u;
    return v;
}

// ---- LZW: the dictionary (prefix code, byte) -> code as an open-addressed table of kTiffwLzwSlots
// words (key << 12 | code, all ones: free), at most 3835 entries between two Clears.
constexpr int kTiffwLzwBits = 13, kTiffwLzwSlots = 1 << kTiffwLzwBits;
constexpr uint32_t kTiffwLzwFree = 0xFFFFFFFFu;
ICX_TIFF_HD int tiffw_lzw_width(int t) { return 9 + (t >= 254) + (t >= 766) + (t >= 1790); }

// The chain's state between bytes. sink(code, width) takes the stream's codes in order; packing
// them into bytes is not the chain's business (serially: TiffwBits; in the kernel all lanes do it).
// feed() returns true when it wrote a Clear: the caller then frees every slot of the dictionary
// before the next feed (the kernel does that with all lanes). writer: this caller's stores to the
// dictionary count (the kernel's lanes run the same chain, lane 0 alone stores).
struct TiffwLzw {
    int t = 0;      // codes since the last Clear
    int next = 258;
    int cur = -1;   // the string matched so far

    template <class Sink>
    ICX_TIFF_HD bool emit(uint32_t code, Sink& sink) {
        sink(code, tiffw_lzw_width(t));
        if (++t != kTiffwLzwClearAt) return false;
        sink(256u, tiffw_lzw_width(t));
        t = 0;
        next = 258;
        return true;
    }
    template <class Sink>
    ICX_TIFF_HD void begin(Sink& sink) { sink(256u, 9); }
    template <class Sink>
    ICX_TIFF_HD bool feed(uint32_t* dict, uint32_t b, Sink& sink, bool writer = true) {
        if (cur < 0) {
            cur = (int)b;
            return false;
        }
        const uint32_t key = (uint32_t)cur << 8 | b;
        uint32_t h = (key * 2654435761u) >> (32 - kTiffwLzwBits);
        for (;;) {
            const uint32_t e = dict[h];
            if (e == kTiffwLzwFree) break;
            if ((e >> 12) == key) {
                cur = (int)(e & 0xFFFu);
                return false;
            }
            h = (h + 1) & (kTiffwLzwSlots - 1);
        }
        const bool cleared = emit((uint32_t)cur, sink);
        if (!cleared) {
            if (writer) dict[h] = key << 12 | (uint32_t)next;
            ++next;
        }
        cur = (int)b;
        return cleared;
    }
    template <class Sink>
    ICX_TIFF_HD void finish(Sink& sink) {
        if (cur >= 0) (void)emit((uint32_t)cur, sink);
        sink(257u, tiffw_lzw_width(t));
    }
};

// Codes into bytes, MSB first, serially; close() pads the last byte with zero bits.
struct TiffwBits {
    uint32_t acc = 0;
    int nacc = 0;  // bits waiting in acc (< 8 between calls)
    template <class Out>
    ICX_TIFF_HD void put(uint32_t code, int width, Out& out) {
        acc = (acc << width) | code;
        nacc += width;
        while (nacc >= 8) {
            out((uint8_t)(acc >> (nacc - 8)));
            nacc -= 8;
        }
    }
    template <class Out>
    ICX_TIFF_HD void close(Out& out) {
        if (nacc > 0) out((uint8_t)(acc << (8 - nacc)));
        nacc = 0;
    }
};

// The stream of n bytes in(0 .. n-1) -> its size. dict: kTiffwLzwSlots words.
template <class In, class Out>
ICX_TIFF_HD uint64_t tiffw_lzw_encode(uint32_t* dict, uint64_t n, In in, Out put_byte) {
    uint64_t size = 0;
    auto out = [&](uint8_t v) {
        put_byte(v);
        ++size;
    };
    TiffwBits bits;
    auto sink = [&](uint32_t code, int width) { bits.put(code, width, out); };
    TiffwLzw z;
    for (int i = 0; i < kTiffwLzwSlots; ++i) dict[i] = kTiffwLzwFree;
    z.begin(sink);
    for (uint64_t i = 0; i < n; ++i)
        if (z.feed(dict, in(i), sink))
            for (int k = 0; k < kTiffwLzwSlots; ++k) dict[k] = kTiffwLzwFree;
    z.finish(sink);
    bits.close(out);
    return size;
}

// ---- PackBits, serially, one row: each maximal run of equal bytes is cut into pieces of 128 from
// its start, a piece of 3 or more is a repeat packet, everything else joins the neighbouring
// literal stretch, stretches are cut into packets of 128 from their start.
template <class In, class Out>
ICX_TIFF_HD uint64_t tiffw_packbits_row(uint32_t n, In in, Out out) {
    uint64_t size = 0;
    uint32_t lit0 = 0, i = 0;  // the pending literal stretch is [lit0, i)
    auto flush = [&](uint32_t end) {
        for (uint32_t q = lit0; q < end; q += 128) {
            const uint32_t len = end - q < 128 ? end - q : 128;
            out((uint8_t)(len - 1));
            for (uint32_t k = 0; k < len; ++k) out((uint8_t)in(q + k));
            size += 1 + len;
        }
    };
    while (i < n) {
        uint32_t j = i;
        const uint32_t v = in(i);
        while (j < n && in(j) == v && j - i < 128) ++j;
        if (j - i >= 3) {
            flush(i);
            out((uint8_t)(257 - (j - i)));
            out((uint8_t)v);
            size += 2;
            lit0 = j;
        }
        i = j;
    }
    flush(n);
    return size;
}

}  // namespace icx
