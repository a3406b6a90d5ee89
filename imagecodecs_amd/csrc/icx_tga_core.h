// icx_tga_core.h -- the arithmetic of the Targa read and write (Image::readTga, codecs.cpp:1304-1407;
// Image::writeTga, :1410-1437), host and device: the 18-byte header parse with its result codes,
// the run-length packet step, one element -> one output pixel (channel order, palette), a serial
// decode that restates the contract, the greedy per-row packer and the file header writer. Plain
// C++: the CPU test builds it with g++ (tests/test_tga_core.py), icx_tga.hip with hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_TGA_HD __host__ __device__ inline
#else
#define ICX_TGA_HD inline
#endif

namespace icx {

// include/icx.h ICX_TGA_*; kTgaPending is internal (the packets of an RLE file are still to be checked).
enum : int32_t {
    kTgaOk = 0, kTgaBadHeader = 1, kTgaUnsupported = 2, kTgaNoImage = 3, kTgaMalformed = 4, kTgaTruncated = 5,
    kTgaTooLarge = 6, kTgaInvalidArgument = 7, kTgaPending = 8
};

struct TgaHead {
    int32_t w, h;
    int32_t d;        // output channels: 1, 3 or 4
    int32_t bpp;      // bytes per stored element (a pixel, or a palette index): 1, 2, 3 or 4
    int32_t rle;      // types 9, 10, 11
    int32_t pal;      // types 1, 9: the element is an index into the colour map
    int32_t topdown;  // descriptor bit 5: the file's first row is the top row
    int32_t map_origin, map_len;
    int64_t map_at;   // file offset of the colour map (entries of d bytes)
    int64_t ds;       // file offset of the image data
};

ICX_TGA_HD int tga_u16(const uint8_t* p) { return p[0] | p[1] << 8; }

// The header walk. kTgaOk: raw types are complete (their data and colour map lie inside the file);
// RLE types still need the packet walk. Otherwise the code of include/icx.h's list.
ICX_TGA_HD int tga_parse(const uint8_t* f, int64_t n, TgaHead* H) {
    if (n < 18) return kTgaBadHeader;
    const int idlen = f[0], cmt = f[1], type = f[2], mes = f[7], bits = f[16], desc = f[17];
    H->map_origin = tga_u16(f + 3);
    H->map_len = tga_u16(f + 5);
    H->w = tga_u16(f + 12);
    H->h = tga_u16(f + 14);
    if (cmt > 1) return kTgaBadHeader;
    if (!(type <= 3 || (type >= 9 && type <= 11))) return kTgaBadHeader;
    if (H->w == 0 || H->h == 0) return kTgaBadHeader;
    H->pal = type == 1 || type == 9;
    H->rle = type >= 9;
    if (H->pal && (cmt == 0 || H->map_len == 0)) return kTgaBadHeader;
    if (type == 0) return kTgaNoImage;
    if (desc & 0x10) return kTgaUnsupported;  // right-to-left
    H->topdown = (desc >> 5) & 1;
    if (H->pal) {
        if ((bits != 8 && bits != 16) || (mes != 24 && mes != 32)) return kTgaUnsupported;
        H->d = mes / 8;
    } else if (type == 2 || type == 10) {
        if (bits != 24 && bits != 32) return kTgaUnsupported;
        H->d = bits / 8;
    } else {
        if (bits != 8) return kTgaUnsupported;
        H->d = 1;
    }
    H->bpp = bits / 8;
    H->map_at = 18 + (int64_t)idlen;
    const int64_t map_bytes = cmt ? (int64_t)H->map_len * ((mes + 7) / 8) : 0;  // skipped when the type has no use for it
    H->ds = H->map_at + map_bytes;
    if (H->ds > n) return kTgaTruncated;
    if (!H->rle && H->ds + (int64_t)H->w * H->h * H->bpp > n) return kTgaTruncated;
    return kTgaOk;
}

// The packet whose header byte is at `pos`: its pixel count and the position after it, or
// kTgaTruncated when the header byte or the payload is not wholly inside the file.
ICX_TGA_HD int tga_packet(const uint8_t* f, int64_t n, int64_t pos, int bpp, int* count, int64_t* next) {
    if (pos >= n) return kTgaTruncated;
    const int hb = f[pos];
    *count = (hb & 127) + 1;
    *next = pos + 1 + ((hb & 128) ? bpp : *count * bpp);
    return *next > n ? kTgaTruncated : kTgaOk;
}

// Output pixel index of the p-th pixel in file order.
ICX_TGA_HD int64_t tga_out_index(const TgaHead& H, int64_t p) {
    if (H.topdown) return p;
    const int64_t r = p / H.w;
    return (H.h - 1 - r) * H.w + (p - r * H.w);
}

// One stored element `e` (bpp bytes; anywhere) -> d output bytes R,G,B(,A) at `o`. `map` is the
// colour map (file + map_at); an index outside it gives zero bytes.
ICX_TGA_HD void tga_store_px(const TgaHead& H, const uint8_t* map, const uint8_t* e, uint8_t* o) {
    const uint8_t* s = e;
    if (H.pal) {
        const int idx = (H.bpp == 2 ? e[0] | e[1] << 8 : e[0]) - H.map_origin;
        if (idx < 0 || idx >= H.map_len) {
            for (int c = 0; c < H.d; ++c) o[c] = 0;
            return;
        }
        s = map + (int64_t)idx * H.d;
    }
    if (H.d == 1) { o[0] = s[0]; return; }
    o[0] = s[2];
    o[1] = s[1];
    o[2] = s[0];
    if (H.d == 4) o[3] = s[3];
}

// The whole read, one packet at a time: the contract restated (and what a GPU result must equal).
// `out` has room for w*h*d bytes once the header is accepted (cap bytes; too little -> kTgaTooLarge).
ICX_TGA_HD int tga_decode_serial(const uint8_t* f, int64_t n, TgaHead* H, uint8_t* out, int64_t cap) {
    const int rc = tga_parse(f, n, H);
    if (rc != kTgaOk) return rc;
    const int64_t npix = (int64_t)H->w * H->h;
    if (npix * H->d > cap) return kTgaTooLarge;
    const uint8_t* map = f + H->map_at;
    if (!H->rle) {
        for (int64_t p = 0; p < npix; ++p) tga_store_px(*H, map, f + H->ds + p * H->bpp, out + tga_out_index(*H, p) * H->d);
        return kTgaOk;
    }
    int64_t pos = H->ds, p = 0;
    while (p < npix) {
        int count;
        int64_t next;
        if (tga_packet(f, n, pos, H->bpp, &count, &next) != kTgaOk) return kTgaTruncated;
        if (count > npix - p) return kTgaMalformed;
        const bool run = f[pos] & 128;
        for (int k = 0; k < count; ++k)
            tga_store_px(*H, map, f + pos + 1 + (run ? 0 : (int64_t)k * H->bpp), out + tga_out_index(*H, p + k) * H->d);
        p += count;
        pos = next;
    }
    return kTgaOk;
}

// ------------------------------------------------------------------------------------ write
ICX_TGA_HD bool tga_write_args_ok(int w, int h, int d) {
    return (d == 1 || d == 3 || d == 4) && w >= 1 && w <= 65535 && h >= 1 && h <= 65535;
}

// writeTga's 18 bytes (codecs.cpp:1417-1426): type 2 (d = 1: 3), +8 when run-length coded.
ICX_TGA_HD void tga_write_header(uint8_t* o, int w, int h, int d, int rle) {
    for (int i = 0; i < 18; ++i) o[i] = 0;
    o[2] = (uint8_t)((d == 1 ? 3 : 2) + (rle ? 8 : 0));
    o[12] = (uint8_t)(w & 255);
    o[13] = (uint8_t)(w >> 8);
    o[14] = (uint8_t)(h & 255);
    o[15] = (uint8_t)(h >> 8);
    o[16] = (uint8_t)(d * 8);
    o[17] = 0x20;
}

ICX_TGA_HD uint64_t tga_encode_bound(int w, int h, int d) {
    return tga_write_args_ok(w, h, d) ? 18 + (uint64_t)w * h * (d + 1) : 0;
}

// Pixel k of a row of d-byte R,G,B(,A) pixels as one word (equal words = equal pixels).
ICX_TGA_HD uint32_t tga_px_word(const uint8_t* row, int d, int k) {
    const uint8_t* p = row + (int64_t)k * d;
    uint32_t v = p[0];
    if (d >= 3) v |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    if (d == 4) v |= (uint32_t)p[3] << 24;
    return v;
}

// The file's bytes of that pixel: B,G,R(,A).
ICX_TGA_HD void tga_put_file_px(uint8_t* o, uint32_t v, int d) {
    if (d == 1) { o[0] = (uint8_t)v; return; }
    o[0] = (uint8_t)(v >> 16);
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)v;
    if (d == 4) o[3] = (uint8_t)(v >> 24);
}

// The greedy packer of one row (include/icx.h), serial as stated: the bytes go to `out` (room for
// w*(d+1)) and their number is returned.
ICX_TGA_HD int64_t tga_pack_row(const uint8_t* row, int w, int d, uint8_t* out) {
    int64_t o = 0;
    int i = 0;
    while (i < w) {
        const uint32_t v = tga_px_word(row, d, i);
        int r = 1;
        while (r < 128 && i + r < w && tga_px_word(row, d, i + r) == v) ++r;
        if (r >= 2) {
            out[o++] = (uint8_t)(0x80 | (r - 1));
            tga_put_file_px(out + o, v, d);
            o += d;
            i += r;
        } else {
            int n = 0;
            for (int k = i; k < w && k - i < 128 && !(k + 1 < w && tga_px_word(row, d, k) == tga_px_word(row, d, k + 1)); ++k) ++n;
            out[o++] = (uint8_t)(n - 1);
            for (int k = 0; k < n; ++k) {
                tga_put_file_px(out + o, tga_px_word(row, d, i + k), d);
                o += d;
            }
            i += n;
        }
    }
    return o;
}

}  // namespace icx
