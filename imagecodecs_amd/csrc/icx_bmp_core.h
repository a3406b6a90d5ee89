// icx_bmp_core.h -- the arithmetic of the BMP read and write (Image::readBmp, codecs.cpp:255-320;
// Image::writeBmp, :324-375), host and device: the header walk into a descriptor with its result
// codes, the mask -> shift / width helper, one stored element -> one output pixel, the run-length
// packet step with its cursor transform, a serial decode that restates the contract of
// include/icx.h, and the header writers. Plain C++: the CPU test builds it with g++
// (tests/test_bmp_core.py), icx_bmp.hip with hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_BMP_HD __host__ __device__ inline
#else
#define ICX_BMP_HD inline
#endif

namespace icx {

// include/icx.h ICX_BMP_*; kBmpPending is internal (the packets of an RLE file are still to be walked).
enum : int32_t {
    kBmpOk = 0, kBmpNotBmp = 1, kBmpBadHeader = 2, kBmpUnsupported = 3, kBmpTruncated = 4, kBmpTooLarge = 5,
    kBmpInvalidArgument = 6, kBmpPending = 7
};

struct BmpHead {
    int32_t w, h;         // h: rows (the header's |biHeight|)
    int32_t d;            // output channels: 1, 3 or 4
    int32_t bits;         // 1, 4, 8, 16, 24, 32
    int32_t rle;          // 0 raw, 8 RLE8, 4 RLE4
    int32_t flip;         // the file's first row is the bottom row (biHeight > 0)
    int32_t pal_n;        // palette entries an index may select (bits <= 8)
    int32_t pal_es;       // bytes per palette entry: 3 (core header) or 4
    int64_t pal_at;       // file offset of the palette (entries B,G,R(,x))
    int64_t ds;           // bfOffBits: file offset of the raster / the packet stream
    int64_t stride;       // bytes per raster row of a raw file
    uint32_t mask[4];     // 16 / 32 bits: R, G, B, A fields (mask[3] == 0: no alpha)
    int32_t shift[4], width[4];
};

ICX_BMP_HD uint32_t bmp_u16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
ICX_BMP_HD uint32_t bmp_u32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// A mask's lowest set bit and its number of set bits; false when the set bits are not contiguous.
ICX_BMP_HD bool bmp_mask_field(uint32_t m, int* shift, int* width) {
    *shift = *width = 0;
    if (m == 0) return true;
    int s = 0;
    while (!((m >> s) & 1)) ++s;
    const uint32_t v = m >> s;
    int n = 0;
    while (n < 32 && ((v >> n) & 1)) ++n;
    *shift = s;
    *width = n;
    return n == 32 || (v >> n) == 0;
}

// A field's value -> 8 bits: exact rounding of v * 255 / (2^n - 1) for n <= 8, the top 8 bits of a
// wider field, 0 for an absent one.
ICX_BMP_HD uint32_t bmp_field8(uint32_t px, uint32_t mask, int shift, int width) {
    if (width == 0) return 0;
    const uint32_t v = (px & mask) >> shift;
    if (width > 8) return v >> (width - 8);
    const uint32_t m = (1u << width) - 1;
    return (v * 510 + m) / (2 * m);
}

// Palette entry idx as R | G << 8 | B << 16; an index at or past the number of entries gives 0.
ICX_BMP_HD uint32_t bmp_pal_rgb(const BmpHead& H, const uint8_t* f, uint32_t idx) {
    if (idx >= (uint32_t)H.pal_n) return 0;
    const uint8_t* e = f + H.pal_at + (int64_t)idx * H.pal_es;
    return e[2] | (uint32_t)e[1] << 8 | (uint32_t)e[0] << 16;
}

// The header walk. kBmpOk: a raw file is complete (palette and raster lie inside the file); an RLE
// file (H->rle != 0) still needs the packet walk. Otherwise the code of include/icx.h's list, in
// the order NOT_BMP, BAD_HEADER, UNSUPPORTED, TOO_LARGE, TRUNCATED.
ICX_BMP_HD int bmp_parse(const uint8_t* f, int64_t n, BmpHead* H) {
    if (n < 18 || f[0] != 'B' || f[1] != 'M') return kBmpNotBmp;
    const int64_t offbits = bmp_u32(f + 10);
    const uint32_t hs = bmp_u32(f + 14);
    if (hs != 12 && hs != 40 && hs != 52 && hs != 56 && hs != 64 && hs != 108 && hs != 124) return kBmpBadHeader;
    if (14 + (int64_t)hs > n) return kBmpBadHeader;
    int64_t w, h;
    uint32_t bits, comp = 0, used = 0;
    if (hs == 12) {
        w = bmp_u16(f + 18);
        h = bmp_u16(f + 20);
        bits = bmp_u16(f + 24);
    } else {
        w = (int32_t)bmp_u32(f + 18);
        h = (int32_t)bmp_u32(f + 22);
        bits = bmp_u16(f + 28);
        comp = bmp_u32(f + 30);
        used = bmp_u32(f + 46);
    }
    if (w <= 0 || h == 0 || h == INT32_MIN) return kBmpBadHeader;
    if (bits != 1 && bits != 4 && bits != 8 && bits != 16 && bits != 24 && bits != 32) return kBmpBadHeader;
    if ((comp == 1 && bits != 8) || (comp == 2 && bits != 4) || ((comp == 3 || comp == 6) && bits != 16 && bits != 32))
        return kBmpBadHeader;
    if (bits < 32 && used > (1u << bits)) return kBmpBadHeader;
    // masks after a 40-byte header; inside a larger one (52: three, 56 and up: four)
    const bool fields = comp == 3 || comp == 6;
    const int64_t extra = hs == 40 && fields ? (comp == 6 ? 16 : 12) : 0;
    if (14 + hs + extra > n) return kBmpBadHeader;
    H->pal_es = hs == 12 ? 3 : 4;
    H->pal_at = 14 + (int64_t)hs + extra;
    H->pal_n = bits <= 8 ? (int32_t)(used ? used : 1u << bits) : 0;
    const int64_t pal_end = H->pal_at + (int64_t)(bits <= 8 ? (uint32_t)H->pal_n : used) * H->pal_es;
    if (offbits < pal_end) return kBmpBadHeader;
    if (comp > 3 && comp != 6) return kBmpUnsupported;
    if (hs == 64 && comp != 0) return kBmpUnsupported;
    if ((comp == 1 || comp == 2) && h < 0) return kBmpUnsupported;
    H->w = (int32_t)w;
    H->h = (int32_t)(h < 0 ? -h : h);
    H->flip = h > 0;
    H->bits = (int32_t)bits;
    H->rle = comp == 1 ? 8 : comp == 2 ? 4 : 0;
    H->ds = offbits;
    H->stride = (w * bits + 31) / 32 * 4;
    for (int c = 0; c < 4; ++c) H->mask[c] = 0;
    if (bits == 16 || bits == 32) {
        if (fields) {
            // (every mask read lies inside the header or the `extra` bytes checked above: a 52-byte
            // header holds three masks, whatever the compression says)
            const bool alpha = hs >= 56 || (hs == 40 && comp == 6);
            for (int c = 0; c < (alpha ? 4 : 3); ++c) H->mask[c] = bmp_u32(f + 54 + 4 * c);
        } else if (bits == 16) {
            H->mask[0] = 0x7C00; H->mask[1] = 0x03E0; H->mask[2] = 0x001F;
        } else {
            H->mask[0] = 0x00FF0000; H->mask[1] = 0x0000FF00; H->mask[2] = 0x000000FF;
        }
    }
    uint32_t seen = 0;
    for (int c = 0; c < 4; ++c) {
        if (!bmp_mask_field(H->mask[c], &H->shift[c], &H->width[c])) return kBmpUnsupported;
        if (seen & H->mask[c]) return kBmpUnsupported;
        seen |= H->mask[c];
    }
    H->d = H->mask[3] ? 4 : 3;
    if (w * H->h > ((int64_t)1 << 30)) return kBmpTooLarge;
    if (pal_end > n || offbits > n) return kBmpTruncated;
    if (!H->rle && offbits + H->stride * H->h > n) return kBmpTruncated;
    if (bits == 8) {  // a grey-identity palette: the index is the grey value
        bool grey = true;
        for (int i = 0; i < H->pal_n && grey; ++i) grey = bmp_pal_rgb(*H, f, (uint32_t)i) == (uint32_t)i * 0x010101u;
        if (grey) H->d = 1;
    }
    return kBmpOk;
}

// Pixel x of the raw row at `row` -> d output bytes at o.
ICX_BMP_HD uint32_t bmp_raw_rgba(const BmpHead& H, const uint8_t* f, const uint8_t* row, int64_t x) {
    switch (H.bits) {
    case 1: return bmp_pal_rgb(H, f, (row[x >> 3] >> (7 - (x & 7))) & 1);
    case 4: return bmp_pal_rgb(H, f, (row[x >> 1] >> ((x & 1) ? 0 : 4)) & 15);
    case 8: return bmp_pal_rgb(H, f, row[x]);
    case 24: return row[3 * x + 2] | (uint32_t)row[3 * x + 1] << 8 | (uint32_t)row[3 * x] << 16;
    default: {
        const uint32_t v = H.bits == 16 ? bmp_u16(row + 2 * x) : bmp_u32(row + 4 * x);
        uint32_t r = 0;
        for (int c = 0; c < 4; ++c) r |= bmp_field8(v, H.mask[c], H.shift[c], H.width[c]) << (8 * c);
        return r;
    }
    }
}
ICX_BMP_HD void bmp_put(uint8_t* o, uint32_t rgba, int d) {
    for (int c = 0; c < d; ++c) o[c] = (uint8_t)(rgba >> (8 * c));
}

// ------------------------------------------------------------------------- run-length packets
// What a packet does to the cursor: x = reset ? dx : x + dx; y += dy. Composing two of them is
// associative, so a scan may compose them in any grouping. dx and dy only grow; they are clamped
// at kBmpFar, past every accepted width and height, so that 32 bits hold any stream's cursor
// (a pixel at or past w or h is dropped either way).
constexpr int32_t kBmpFar = 1 << 30;
struct BmpMove {
    int32_t reset, dx, dy;
};
ICX_BMP_HD int32_t bmp_far_add(int32_t a, int32_t b) {  // (0 <= a, b <= kBmpFar: the sum fits 32 unsigned bits)
    const uint32_t s = (uint32_t)a + (uint32_t)b;
    return s > (uint32_t)kBmpFar ? kBmpFar : (int32_t)s;
}
ICX_BMP_HD BmpMove bmp_compose(const BmpMove& a, const BmpMove& b) {  // a, then b
    return BmpMove{a.reset | b.reset, b.reset ? b.dx : bmp_far_add(a.dx, b.dx), bmp_far_add(a.dy, b.dy)};
}
ICX_BMP_HD void bmp_apply(const BmpMove& m, int32_t* x, int32_t* y) {
    *x = m.reset ? m.dx : bmp_far_add(*x, m.dx);
    *y = bmp_far_add(*y, m.dy);
}

enum : int32_t { kBmpPkRun = 0, kBmpPkLiteral = 1, kBmpPkMove = 2, kBmpPkEnd = 3, kBmpPkCut = 4 };
struct BmpPacket {
    int32_t kind;    // kBmpPk*: End = end-of-bitmap or fewer than 2 bytes left; Cut = the file cuts it short
    int32_t len;     // bytes, pad byte included
    int32_t count;   // pixels of a run or a literal
    BmpMove move;
};
// The packet at p[0..) of which `left` bytes are inside the file (only min(left, 4) are read
// here). rle: 8 or 4.
ICX_BMP_HD BmpPacket bmp_packet(const uint8_t* p, int64_t left, int rle) {
    BmpPacket k{kBmpPkEnd, 0, 0, {0, 0, 0}};
    if (left < 2) return k;
    const int a = p[0], b = p[1];
    if (a > 0) {
        k.kind = kBmpPkRun;
        k.len = 2;
        k.count = a;
        k.move.dx = a;
    } else if (b == 0) {
        k.kind = kBmpPkMove;
        k.len = 2;
        k.move.reset = 1;
        k.move.dy = 1;
    } else if (b == 1) {
        k.len = 2;
    } else if (b == 2) {
        k.kind = kBmpPkMove;
        k.len = 4;
        if (left < 4) { k.kind = kBmpPkCut; return k; }
        k.move.dx = p[2];
        k.move.dy = p[3];
    } else {
        k.kind = kBmpPkLiteral;
        k.count = b;
        k.len = 2 + (((rle == 8 ? b : (b + 1) / 2) + 1) & ~1);
        k.move.dx = b;
        if (left < k.len) k.kind = kBmpPkCut;
    }
    return k;
}
// Palette index of pixel k of a run or literal packet at p.
ICX_BMP_HD uint32_t bmp_packet_index(const uint8_t* p, int kind, int rle, int k) {
    if (rle == 8) return kind == kBmpPkRun ? p[1] : p[2 + k];
    const uint8_t b = kind == kBmpPkRun ? p[1] : p[2 + (k >> 1)];
    return (k & 1) ? b & 15 : b >> 4;
}

// The whole read, serial as the contract states it (and what a GPU result must equal). `out` has
// room for w*h*d bytes once the header is accepted (cap bytes; too little -> kBmpTooLarge).
ICX_BMP_HD int bmp_decode_serial(const uint8_t* f, int64_t n, BmpHead* H, uint8_t* out, int64_t cap) {
    const int rc = bmp_parse(f, n, H);
    if (rc != kBmpOk) return rc;
    const int w = H->w, h = H->h, d = H->d;
    if ((int64_t)w * h * d > cap) return kBmpTooLarge;
    if (!H->rle) {
        for (int r = 0; r < h; ++r) {
            const uint8_t* row = f + H->ds + H->stride * r;
            uint8_t* o = out + (int64_t)(H->flip ? h - 1 - r : r) * w * d;
            for (int x = 0; x < w; ++x) bmp_put(o + (int64_t)x * d, bmp_raw_rgba(*H, f, row, x), d);
        }
        return kBmpOk;
    }
    // first the walk alone: a packet cut short leaves no pixels
    for (int64_t pos = H->ds;;) {
        const BmpPacket k = bmp_packet(f + pos, n - pos, H->rle);
        if (k.kind == kBmpPkCut) return kBmpTruncated;
        if (k.kind == kBmpPkEnd) break;
        pos += k.len;
    }
    const uint32_t bg = bmp_pal_rgb(*H, f, 0);
    for (int64_t p = 0; p < (int64_t)w * h; ++p) bmp_put(out + p * d, bg, d);
    int32_t x = 0, y = 0;
    for (int64_t pos = H->ds;;) {
        const BmpPacket k = bmp_packet(f + pos, n - pos, H->rle);
        if (k.kind == kBmpPkEnd) break;
        if (y < h)
            for (int q = 0; q < k.count && x + q < w; ++q)
                bmp_put(out + ((int64_t)(h - 1 - y) * w + x + q) * d, bmp_pal_rgb(*H, f, bmp_packet_index(f + pos, k.kind, H->rle, q)), d);
        bmp_apply(k.move, &x, &y);
        pos += k.len;
    }
    return kBmpOk;
}

// ------------------------------------------------------------------------------------ write
ICX_BMP_HD bool bmp_write_args_ok(int w, int h, int d) {
    return (d == 1 || d == 3 || d == 4) && w >= 1 && w <= 65535 && h >= 1 && h <= 65535;
}
// Bytes before the raster: 14 + 40 (d = 3), + 1024 of palette (d = 1), 14 + 108 (d = 4).
ICX_BMP_HD int bmp_write_offbits(int d) { return d == 1 ? 54 + 1024 : d == 3 ? 54 : 122; }
ICX_BMP_HD int64_t bmp_write_stride(int w, int d) { return ((int64_t)w * d + 3) & ~(int64_t)3; }
ICX_BMP_HD uint64_t bmp_encode_bound(int w, int h, int d) {
    return bmp_write_args_ok(w, h, d) ? (uint64_t)bmp_write_offbits(d) + (uint64_t)bmp_write_stride(w, d) * h : 0;
}
ICX_BMP_HD void bmp_put_u32(uint8_t* o, uint32_t v) {
    o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24);
}
// The bmp_write_offbits(d) bytes in front of the raster (for d = 1 the grey palette included).
ICX_BMP_HD void bmp_write_header(uint8_t* o, int w, int h, int d) {
    const int off = bmp_write_offbits(d), hs = d == 4 ? 108 : 40;
    const uint32_t image = (uint32_t)(bmp_write_stride(w, d) * h);
    for (int i = 0; i < off; ++i) o[i] = 0;
    o[0] = 'B';
    o[1] = 'M';
    bmp_put_u32(o + 2, (uint32_t)off + image);
    bmp_put_u32(o + 10, (uint32_t)off);
    bmp_put_u32(o + 14, (uint32_t)hs);
    bmp_put_u32(o + 18, (uint32_t)w);
    bmp_put_u32(o + 22, (uint32_t)h);
    o[26] = 1;
    o[28] = (uint8_t)(d * 8);
    o[30] = d == 4 ? 3 : 0;
    bmp_put_u32(o + 34, image);
    if (d == 4) {
        bmp_put_u32(o + 54, 0x00FF0000);
        bmp_put_u32(o + 58, 0x0000FF00);
        bmp_put_u32(o + 62, 0x000000FF);
        bmp_put_u32(o + 66, 0xFF000000);
        o[70] = 'B'; o[71] = 'G'; o[72] = 'R'; o[73] = 's';  // LCS_sRGB
    }
    if (d == 1) {
        bmp_put_u32(o + 46, 256);
        for (int i = 0; i < 256; ++i) o[54 + 4 * i] = o[55 + 4 * i] = o[56 + 4 * i] = (uint8_t)i;
    }
}
// One written row: R,G,B(,A) or grey pixels -> the file's row with its zero pad bytes.
ICX_BMP_HD void bmp_write_row(const uint8_t* px, int w, int d, uint8_t* o) {
    const int64_t stride = bmp_write_stride(w, d);
    for (int x = 0; x < w; ++x) {
        const uint8_t* s = px + (int64_t)x * d;
        uint8_t* t = o + (int64_t)x * d;
        if (d == 1) { t[0] = s[0]; continue; }
        t[0] = s[2]; t[1] = s[1]; t[2] = s[0];
        if (d == 4) t[3] = s[3];
    }
    for (int64_t b = (int64_t)w * d; b < stride; ++b) o[b] = 0;
}

}  // namespace icx
