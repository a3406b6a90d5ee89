// icx_dds_core.h -- the arithmetic of the DDS read and write (Image::readDds / writeDds,
// codecs.cpp), host and device, written from the contract of include/icx.h: the header walk into a
// descriptor with its result codes, the BC1-BC5 block decoders, the range-fit block encoders, the
// masked and copied uncompressed forms, a serial decode and encode that restate the contract, and
// the header writer. Plain C++: the CPU test builds it with g++ (tests/test_dds_core.py),
// icx_dds.hip with hipcc.
#pragma once
#include <cstdint>

#include "icx_bmp_core.h"  // bmp_mask_field, bmp_field8: the field scaling is BMP's

#if defined(__HIPCC__)
#define ICX_DDS_HD __host__ __device__ inline
#else
#define ICX_DDS_HD inline
#endif

namespace icx {

// include/icx.h ICX_DDS_*
enum : int32_t {
    kDdsOk = 0, kDdsNotDds = 1, kDdsBadHeader = 2, kDdsUnsupported = 3, kDdsTruncated = 4, kDdsTooLarge = 5,
    kDdsInvalidArgument = 6
};
enum : int32_t { kDdsUbyte = 0, kDdsUshort = 1, kDdsFloat = 2 };  // icx_pnm_type = ImageCodecs::Type
enum : int32_t { kDdsRaw = 0, kDdsBc = 1 };                        // icx_dds_format (write)
// What the top level holds: 4 x 4 blocks, pixels cut into fields by masks, or samples to copy.
enum : int32_t { kDdsBc1 = 1, kDdsBc2 = 2, kDdsBc3 = 3, kDdsBc4 = 4, kDdsBc5 = 5, kDdsMasked = 6, kDdsCopy = 7 };
constexpr int64_t kDdsMaxPixels = (int64_t)1 << 30;

struct DdsHead {
    int32_t w, h;
    int32_t d;         // output channels, 1 .. 4
    int32_t type;      // kDdsUbyte / kDdsUshort / kDdsFloat
    int32_t kind;      // kDdsBc1 .. kDdsCopy
    int32_t bpp;       // Masked, Copy: bytes per stored pixel
    int32_t bytewise;  // Masked: every output channel is one whole byte of the stored pixel
    uint32_t at;       // bytewise: byte c of the stored pixel that is output channel c, at bits 8c
    int64_t ds;        // file offset of the top level
    int64_t bytes;     // its length
    uint32_t mask[4];  // Masked: the field of output channel c
    int32_t shift[4], width[4];
};

ICX_DDS_HD uint32_t dds_u32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
constexpr uint32_t dds_cc(char a, char b, char c, char d) {
    return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}
ICX_DDS_HD int dds_elem_bytes(int type) { return type == kDdsFloat ? 4 : type == kDdsUshort ? 2 : 1; }
ICX_DDS_HD int dds_block_bytes(int kind) { return kind == kDdsBc1 || kind == kDdsBc4 ? 8 : 16; }
ICX_DDS_HD int64_t dds_out_bytes(const DdsHead& H) { return (int64_t)H.w * H.h * H.d * dds_elem_bytes(H.type); }

// kind, channels and type of a block or copied form (true: the form is known).
ICX_DDS_HD bool dds_set_form(DdsHead* H, int kind, int d, int type) {
    H->kind = kind;
    H->d = d;
    H->type = type;
    H->bpp = kind == kDdsCopy ? d * dds_elem_bytes(type) : 0;
    return true;
}
// The four masks R, G, B, A of an uncompressed file -> the fields of the output channels. False
// for masks the contract refuses.
ICX_DDS_HD bool dds_set_masks(DdsHead* H, int bits, const uint32_t m[4], bool luminance) {
    uint32_t seen = 0;
    for (int c = 0; c < 4; ++c) {
        int s, n;
        if (!bmp_mask_field(m[c], &s, &n)) return false;
        if (bits < 32 && (m[c] >> bits)) return false;
        if (seen & m[c]) return false;
        seen |= m[c];
    }
    uint32_t o[4] = {0, 0, 0, 0};
    int d = 0;
    if (luminance) {
        if (!m[0]) return false;
        o[d++] = m[0];
        if (m[3]) o[d++] = m[3];
    } else if (!m[0] && !m[1] && !m[2]) {
        if (!m[3]) return false;
        o[d++] = m[3];
    } else if (m[0] && !m[1] && !m[2] && !m[3]) {
        o[d++] = m[0];
    } else if (m[0] && m[1] && !m[2] && !m[3]) {
        o[d++] = m[0];
        o[d++] = m[1];
    } else if (m[0] && m[1] && m[2]) {
        o[d++] = m[0];
        o[d++] = m[1];
        o[d++] = m[2];
        if (m[3]) o[d++] = m[3];
    } else {
        return false;
    }
    H->kind = kDdsMasked;
    H->d = d;
    H->type = kDdsUbyte;
    H->bpp = bits / 8;
    H->bytewise = 1;
    H->at = 0;
    for (int c = 0; c < 4; ++c) {
        H->mask[c] = o[c];
        bmp_mask_field(o[c], &H->shift[c], &H->width[c]);
        if (c < d) {
            if (H->width[c] != 8 || (H->shift[c] & 7)) H->bytewise = 0;
            H->at |= (uint32_t)(H->shift[c] >> 3) << (8 * c);
        }
    }
    return true;
}

// The header walk: kDdsOk with the descriptor filled and the top level wholly inside the file, or
// the code of include/icx.h's list, in the order NOT_DDS, BAD_HEADER, UNSUPPORTED, TOO_LARGE,
// TRUNCATED. Every read is below n.
ICX_DDS_HD int dds_parse(const uint8_t* f, int64_t n, DdsHead* H) {
    if (n < 4 || f[0] != 'D' || f[1] != 'D' || f[2] != 'S' || f[3] != ' ') return kDdsNotDds;
    if (n < 128) return kDdsBadHeader;
    if (dds_u32(f + 4) != 124 || dds_u32(f + 76) != 32) return kDdsBadHeader;
    const uint32_t h = dds_u32(f + 12), w = dds_u32(f + 16);
    if (w == 0 || h == 0) return kDdsBadHeader;
    const uint32_t pff = dds_u32(f + 80), cc = dds_u32(f + 84), bits = dds_u32(f + 88);
    const bool fourcc = (pff & 4) != 0, dx10 = fourcc && cc == dds_cc('D', 'X', '1', '0');
    if (dx10 && n < 148) return kDdsBadHeader;
    if (!fourcc && bits != 8 && bits != 16 && bits != 24 && bits != 32) return kDdsBadHeader;
    if (dds_u32(f + 112) & (0x200u | 0x200000u)) return kDdsUnsupported;  // cubemap, volume
    *H = DdsHead{};
    H->ds = dx10 ? 148 : 128;
    bool ok = false;
    if (dx10) {
        const uint32_t fmt = dds_u32(f + 128), dim = dds_u32(f + 132), misc = dds_u32(f + 136), arr = dds_u32(f + 140);
        if (arr != 1 || (misc & 4) || dim != 3) return kDdsUnsupported;
        const uint32_t rgba[4] = {0xFF, 0xFF00, 0xFF0000, 0xFF000000u}, bgra[4] = {0xFF0000, 0xFF00, 0xFF, 0xFF000000u};
        const uint32_t bgrx[4] = {0xFF0000, 0xFF00, 0xFF, 0}, r8[4] = {0xFF, 0, 0, 0}, rg8[4] = {0xFF, 0xFF00, 0, 0};
        switch (fmt) {
        case 71: case 72: ok = dds_set_form(H, kDdsBc1, 3, kDdsUbyte); break;
        case 74: case 75: ok = dds_set_form(H, kDdsBc2, 4, kDdsUbyte); break;
        case 77: case 78: ok = dds_set_form(H, kDdsBc3, 4, kDdsUbyte); break;
        case 80: ok = dds_set_form(H, kDdsBc4, 1, kDdsUbyte); break;
        case 83: ok = dds_set_form(H, kDdsBc5, 2, kDdsUbyte); break;
        case 2: ok = dds_set_form(H, kDdsCopy, 4, kDdsFloat); break;
        case 6: ok = dds_set_form(H, kDdsCopy, 3, kDdsFloat); break;
        case 16: ok = dds_set_form(H, kDdsCopy, 2, kDdsFloat); break;
        case 41: ok = dds_set_form(H, kDdsCopy, 1, kDdsFloat); break;
        case 11: ok = dds_set_form(H, kDdsCopy, 4, kDdsUshort); break;
        case 35: ok = dds_set_form(H, kDdsCopy, 2, kDdsUshort); break;
        case 56: ok = dds_set_form(H, kDdsCopy, 1, kDdsUshort); break;
        case 28: case 29: ok = dds_set_masks(H, 32, rgba, false); break;
        case 87: case 91: ok = dds_set_masks(H, 32, bgra, false); break;
        case 88: case 93: ok = dds_set_masks(H, 32, bgrx, false); break;
        case 61: ok = dds_set_masks(H, 8, r8, false); break;
        case 49: ok = dds_set_masks(H, 16, rg8, false); break;
        default: break;
        }
    } else if (fourcc) {
        switch (cc) {
        case dds_cc('D', 'X', 'T', '1'): ok = dds_set_form(H, kDdsBc1, 3, kDdsUbyte); break;
        case dds_cc('D', 'X', 'T', '2'): case dds_cc('D', 'X', 'T', '3'): ok = dds_set_form(H, kDdsBc2, 4, kDdsUbyte); break;
        case dds_cc('D', 'X', 'T', '4'): case dds_cc('D', 'X', 'T', '5'): case dds_cc('B', 'C', '3', 'U'):
            ok = dds_set_form(H, kDdsBc3, 4, kDdsUbyte);
            break;
        case dds_cc('A', 'T', 'I', '1'): case dds_cc('B', 'C', '4', 'U'): ok = dds_set_form(H, kDdsBc4, 1, kDdsUbyte); break;
        case dds_cc('A', 'T', 'I', '2'): case dds_cc('B', 'C', '5', 'U'): ok = dds_set_form(H, kDdsBc5, 2, kDdsUbyte); break;
        case 116: ok = dds_set_form(H, kDdsCopy, 4, kDdsFloat); break;
        case 115: ok = dds_set_form(H, kDdsCopy, 2, kDdsFloat); break;
        case 114: ok = dds_set_form(H, kDdsCopy, 1, kDdsFloat); break;
        case 36: ok = dds_set_form(H, kDdsCopy, 4, kDdsUshort); break;
        default: break;
        }
    } else {
        const uint32_t m[4] = {dds_u32(f + 92), dds_u32(f + 96), dds_u32(f + 100), dds_u32(f + 104)};
        ok = dds_set_masks(H, (int)bits, m, (pff & 0x20000u) != 0);
    }
    if (!ok) return kDdsUnsupported;
    if (w > (uint32_t)kDdsMaxPixels || h > (uint32_t)kDdsMaxPixels || (int64_t)w * h > kDdsMaxPixels) return kDdsTooLarge;
    H->w = (int32_t)w;
    H->h = (int32_t)h;
    H->bytes = H->kind <= kDdsBc5 ? (int64_t)((w + 3) / 4) * ((h + 3) / 4) * dds_block_bytes(H->kind) : (int64_t)w * h * H->bpp;
    if (H->ds + H->bytes > n) return kDdsTruncated;
    return kDdsOk;
}

// ------------------------------------------------------------------------------ block decode
// A block is 2 (BC1, BC4) or 4 little-endian 32-bit words.
// The four colours of a colour block, a channel to a word: entry k at bits 8k. (Words and shifts,
// not an array indexed by the pixel's two bits: the compiler would keep that array in scratch memory.)
struct DdsColors {
    uint32_t r, g, b;
};
ICX_DDS_HD uint32_t dds_four_entries(uint32_t p0, uint32_t p1, bool thirds) {
    const uint32_t e2 = thirds ? (2 * p0 + p1) / 3 : (p0 + p1) / 2, e3 = thirds ? (p0 + 2 * p1) / 3 : 0;
    return p0 | p1 << 8 | e2 << 16 | e3 << 24;
}
// The palette of the colour block whose first word is w0; `four`: BC2 / BC3, always the first form.
ICX_DDS_HD DdsColors dds_color_palette(uint32_t w0, bool four) {
    const uint32_t c0 = w0 & 0xFFFF, c1 = w0 >> 16;
    const bool thirds = four || c0 > c1;
    const uint32_t r0 = c0 >> 11 & 31, g0 = c0 >> 5 & 63, b0 = c0 & 31, r1 = c1 >> 11 & 31, g1 = c1 >> 5 & 63, b1 = c1 & 31;
    return DdsColors{dds_four_entries(r0 << 3 | r0 >> 2, r1 << 3 | r1 >> 2, thirds), dds_four_entries(g0 << 2 | g0 >> 4, g1 << 2 | g1 >> 4, thirds),
                     dds_four_entries(b0 << 3 | b0 >> 2, b1 << 3 | b1 >> 2, thirds)};
}
// Entry i as R | G << 8 | B << 16.
ICX_DDS_HD uint32_t dds_color_entry(const DdsColors& P, uint32_t i) {
    const uint32_t s = 8 * i;
    return (P.r >> s & 255) | (P.g >> s & 255) << 8 | (P.b >> s & 255) << 16;
}
// The eight values of an interpolated-alpha block (BC3 alpha, BC4, a half of BC5), entry k at bits 8k.
ICX_DDS_HD uint64_t dds_alpha_palette(uint32_t w0) {
    const uint32_t a0 = w0 & 255, a1 = w0 >> 8 & 255;
    uint64_t p = a0 | (uint64_t)a1 << 8;
    if (a0 > a1) {
        for (uint32_t k = 1; k <= 6; ++k) p |= (uint64_t)(((7 - k) * a0 + k * a1) / 7) << (8 * (k + 1));
    } else {
        for (uint32_t k = 1; k <= 4; ++k) p |= (uint64_t)(((5 - k) * a0 + k * a1) / 5) << (8 * (k + 1));
        p |= (uint64_t)255 << 56;
    }
    return p;
}
// Value of pixel i of the interpolated-alpha block in words w0, w1.
ICX_DDS_HD uint32_t dds_alpha_pixel(uint64_t pal, uint32_t w0, uint32_t w1, int i) {
    const uint64_t idx = (uint64_t)w1 << 16 | w0 >> 16;
    return (uint32_t)(pal >> (8 * (uint32_t)(idx >> (3 * i) & 7))) & 255u;
}
struct DdsBlockPal {
    DdsColors p;     // the colour block's palette
    uint64_t a, b;   // the first (BC3 alpha, BC4, BC5 red) and second (BC5 green) alpha palette
};
ICX_DDS_HD void dds_block_setup(int kind, const uint32_t* w, DdsBlockPal* P) {
    if (kind == kDdsBc1) P->p = dds_color_palette(w[0], false);
    if (kind == kDdsBc2 || kind == kDdsBc3) P->p = dds_color_palette(w[2], true);
    if (kind >= kDdsBc3) P->a = dds_alpha_palette(w[0]);
    if (kind == kDdsBc5) P->b = dds_alpha_palette(w[2]);
}
// Pixel i (4y + x) of the block: output channel c at bits 8c.
ICX_DDS_HD uint32_t dds_block_pixel(int kind, const uint32_t* w, const DdsBlockPal& P, int i) {
    switch (kind) {
    case kDdsBc1: return dds_color_entry(P.p, w[1] >> (2 * i) & 3);
    case kDdsBc2: return dds_color_entry(P.p, w[3] >> (2 * i) & 3) | ((w[i >> 3] >> (4 * (i & 7)) & 15) * 17) << 24;
    case kDdsBc3: return dds_color_entry(P.p, w[3] >> (2 * i) & 3) | dds_alpha_pixel(P.a, w[0], w[1], i) << 24;
    case kDdsBc4: return dds_alpha_pixel(P.a, w[0], w[1], i);
    default: return dds_alpha_pixel(P.a, w[0], w[1], i) | dds_alpha_pixel(P.b, w[2], w[3], i) << 8;
    }
}

// Stored pixel v of a masked file -> output channel c at bits 8c.
ICX_DDS_HD uint32_t dds_masked_pixel(const DdsHead& H, uint32_t v) {
    uint32_t r = 0;
    for (int c = 0; c < 4; ++c) r |= bmp_field8(v, H.mask[c], H.shift[c], H.width[c]) << (8 * c);
    return r;
}

// The whole read, serial as the contract states it (what a GPU result must equal). `out` has room
// for cap bytes; fewer than the image takes -> kDdsTooLarge.
ICX_DDS_HD int dds_decode_serial(const uint8_t* f, int64_t n, DdsHead* H, uint8_t* out, int64_t cap) {
    const int rc = dds_parse(f, n, H);
    if (rc != kDdsOk) return rc;
    if (dds_out_bytes(*H) > cap) return kDdsTooLarge;
    const int w = H->w, h = H->h, d = H->d;
    const uint8_t* s = f + H->ds;
    if (H->kind == kDdsCopy) {
        for (int64_t k = 0; k < H->bytes; ++k) out[k] = s[k];
    } else if (H->kind == kDdsMasked) {
        for (int64_t p = 0; p < (int64_t)w * h; ++p) {
            uint32_t v = 0;
            for (int b = 0; b < H->bpp; ++b) v |= (uint32_t)s[p * H->bpp + b] << (8 * b);
            const uint32_t px = dds_masked_pixel(*H, v);
            for (int c = 0; c < d; ++c) out[p * d + c] = (uint8_t)(px >> (8 * c));
        }
    } else {
        const int bw = (w + 3) / 4, bh = (h + 3) / 4, bs = dds_block_bytes(H->kind);
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                const uint8_t* b = s + ((int64_t)by * bw + bx) * bs;
                uint32_t wd[4] = {dds_u32(b), dds_u32(b + 4), 0, 0};
                if (bs == 16) { wd[2] = dds_u32(b + 8); wd[3] = dds_u32(b + 12); }
                DdsBlockPal P{};
                dds_block_setup(H->kind, wd, &P);
                for (int i = 0; i < 16; ++i) {
                    const int x = 4 * bx + (i & 3), y = 4 * by + (i >> 2);
                    if (x >= w || y >= h) continue;
                    const uint32_t px = dds_block_pixel(H->kind, wd, P, i);
                    for (int c = 0; c < d; ++c) out[((int64_t)y * w + x) * d + c] = (uint8_t)(px >> (8 * c));
                }
            }
    }
    return kDdsOk;
}

// ------------------------------------------------------------------------------------ write
ICX_DDS_HD bool dds_write_args_ok(int w, int h, int d, int format) {
    return d >= 1 && d <= 4 && w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (format == kDdsRaw || format == kDdsBc);
}
ICX_DDS_HD int dds_write_kind(int d) { return d == 3 ? kDdsBc1 : d == 4 ? kDdsBc3 : d == 1 ? kDdsBc4 : kDdsBc5; }
// Bytes after the 128 of the header.
ICX_DDS_HD uint64_t dds_write_payload(int w, int h, int d, int format) {
    if (format == kDdsRaw) return (uint64_t)w * h * d;
    return (uint64_t)((w + 3) / 4) * ((h + 3) / 4) * dds_block_bytes(dds_write_kind(d));
}
ICX_DDS_HD uint64_t dds_encode_bound(int w, int h, int d, int format) {
    return dds_write_args_ok(w, h, d, format) ? 128 + dds_write_payload(w, h, d, format) : 0;
}
ICX_DDS_HD void dds_put_u32(uint8_t* o, uint32_t v) {
    o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24);
}
// The 128 bytes in front of the top level.
ICX_DDS_HD void dds_write_header(uint8_t* o, int w, int h, int d, int format) {
    for (int i = 0; i < 128; ++i) o[i] = 0;
    dds_put_u32(o, dds_cc('D', 'D', 'S', ' '));
    dds_put_u32(o + 4, 124);
    dds_put_u32(o + 8, 0x1007u | (format == kDdsRaw ? 0x8u : 0x80000u));
    dds_put_u32(o + 12, (uint32_t)h);
    dds_put_u32(o + 16, (uint32_t)w);
    dds_put_u32(o + 20, format == kDdsRaw ? (uint32_t)(w * d) : (uint32_t)dds_write_payload(w, h, d, format));
    dds_put_u32(o + 76, 32);
    dds_put_u32(o + 108, 0x1000);
    if (format == kDdsBc) {
        dds_put_u32(o + 80, 4);
        dds_put_u32(o + 84, d == 3 ? dds_cc('D', 'X', 'T', '1') : d == 4 ? dds_cc('D', 'X', 'T', '5')
                          : d == 1 ? dds_cc('B', 'C', '4', 'U') : dds_cc('B', 'C', '5', 'U'));
        return;
    }
    dds_put_u32(o + 80, d == 3 ? 0x40u : d == 4 ? 0x41u : d == 1 ? 0x20000u : 0x20001u);
    dds_put_u32(o + 88, (uint32_t)(8 * d));
    if (d >= 3) {
        dds_put_u32(o + 92, 0xFF0000);
        dds_put_u32(o + 96, 0xFF00);
        dds_put_u32(o + 100, 0xFF);
        if (d == 4) dds_put_u32(o + 104, 0xFF000000u);
    } else {
        dds_put_u32(o + 92, 0xFF);
        if (d == 2) dds_put_u32(o + 104, 0xFF00);
    }
}
// Byte q of a RAW file's pixel bytes, from the image's bytes px: B,G,R(,A) for d >= 3, else as they are.
ICX_DDS_HD int64_t dds_raw_source(int64_t q, int d) {
    if (d < 3) return q;
    const int64_t x = q / d;
    const int c = (int)(q - x * d);
    return c < 3 ? x * d + 2 - c : q;
}

ICX_DDS_HD uint32_t dds_q5(uint32_t v) { return (31 * v + 127) / 255; }
ICX_DDS_HD uint32_t dds_q6(uint32_t v) { return (63 * v + 127) / 255; }
// The colour block of 16 pixels (R | G << 8 | B << 16 at least) -> two words.
ICX_DDS_HD void dds_encode_color(const uint32_t px[16], uint32_t out[2]) {
    uint32_t hi[3] = {0, 0, 0}, lo[3] = {255, 255, 255};
    for (int i = 0; i < 16; ++i)
        for (int c = 0; c < 3; ++c) {
            const uint32_t v = px[i] >> (8 * c) & 255;
            hi[c] = v > hi[c] ? v : hi[c];
            lo[c] = v < lo[c] ? v : lo[c];
        }
    const uint32_t c0 = dds_q5(hi[0]) << 11 | dds_q6(hi[1]) << 5 | dds_q5(hi[2]);
    const uint32_t c1 = dds_q5(lo[0]) << 11 | dds_q6(lo[1]) << 5 | dds_q5(lo[2]);
    out[0] = c0 | c1 << 16;
    out[1] = 0;
    if (c0 == c1) return;
    const DdsColors P = dds_color_palette(out[0], true);
    for (int i = 0; i < 16; ++i) {
        uint32_t best = 0, bd = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t pk = dds_color_entry(P, k);
            uint32_t dist = 0;
            for (int c = 0; c < 3; ++c) {
                const int32_t e = (int32_t)(px[i] >> (8 * c) & 255) - (int32_t)(pk >> (8 * c) & 255);
                dist += (uint32_t)(e * e);
            }
            if (dist < bd) { bd = dist; best = k; }
        }
        out[1] |= best << (2 * i);
    }
}
// An interpolated-alpha block of the 16 values at bits `shift` of px -> two words.
ICX_DDS_HD void dds_encode_alpha(const uint32_t px[16], int shift, uint32_t out[2]) {
    uint32_t a0 = 0, a1 = 255;
    for (int i = 0; i < 16; ++i) {
        const uint32_t v = px[i] >> shift & 255;
        a0 = v > a0 ? v : a0;
        a1 = v < a1 ? v : a1;
    }
    out[0] = a0 | a1 << 8;
    out[1] = 0;
    if (a0 == a1) return;
    const uint64_t pal = dds_alpha_palette(out[0]);
    uint64_t idx = 0;
    for (int i = 0; i < 16; ++i) {
        const int32_t v = (int32_t)(px[i] >> shift & 255);
        uint32_t best = 0;
        int32_t bd = 256;
        for (uint32_t k = 0; k < 8; ++k) {
            int32_t e = v - (int32_t)(pal >> (8 * k) & 255);
            e = e < 0 ? -e : e;
            if (e < bd) { bd = e; best = k; }
        }
        idx |= (uint64_t)best << (3 * i);
    }
    out[0] |= (uint32_t)(idx << 16);
    out[1] = (uint32_t)(idx >> 16);
}
// The block of a d-channel image (channel c at bits 8c of each pixel) -> 2 (d = 1, 3) or 4 words.
ICX_DDS_HD void dds_encode_block(int d, const uint32_t px[16], uint32_t out[4]) {
    if (d == 3) {
        dds_encode_color(px, out);
    } else if (d == 4) {
        dds_encode_alpha(px, 24, out);
        dds_encode_color(px, out + 2);
    } else {
        dds_encode_alpha(px, 0, out);
        if (d == 2) dds_encode_alpha(px, 8, out + 2);
    }
}

// The whole write, serial: dds_encode_bound(...) bytes to out.
ICX_DDS_HD void dds_encode_serial(const uint8_t* px, int w, int h, int d, int format, uint8_t* out) {
    dds_write_header(out, w, h, d, format);
    uint8_t* o = out + 128;
    if (format == kDdsRaw) {
        for (int64_t q = 0; q < (int64_t)w * h * d; ++q) o[q] = px[dds_raw_source(q, d)];
        return;
    }
    const int bw = (w + 3) / 4, bh = (h + 3) / 4, nw = dds_block_bytes(dds_write_kind(d)) / 4;
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
            uint32_t p[16], wd[4] = {0, 0, 0, 0};
            for (int i = 0; i < 16; ++i) {
                int x = 4 * bx + (i & 3), y = 4 * by + (i >> 2);
                x = x < w ? x : w - 1;
                y = y < h ? y : h - 1;
                p[i] = 0;
                for (int c = 0; c < d; ++c) p[i] |= (uint32_t)px[((int64_t)y * w + x) * d + c] << (8 * c);
            }
            dds_encode_block(d, p, wd);
            for (int k = 0; k < nw; ++k) dds_put_u32(o + (((int64_t)by * bw + bx) * nw + k) * 4, wd[k]);
        }
}

}  // namespace icx
