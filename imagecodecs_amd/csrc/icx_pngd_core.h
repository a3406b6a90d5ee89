// icx_pngd_core.h -- host/device core of the PNG read (icx_pngd.hip): the chunk walk, once, for the
// host probe (icx_png_probe), the device parse kernel (k_pngd_parse) and the IDAT gather
// (k_pngd_gather), the way icx_jpeg_probe and k_parse share theirs. Image::readPng
// (codecs.cpp:903-1020) leaves this to libpng; the rules here are the PNG specification's.
//
//  * signature, then IHDR first: length 13, CRC, width / height >= 1, a bit depth legal for the
//    colour type, compression 0, filter method 0 (else BAD_HEADER); interlace 0 (else UNSUPPORTED);
//    the reference's pixel limit (checkSize, codecs.cpp:881-892): w, h or w*h above 0x1000000 is
//    TOO_LARGE.
//  * then every chunk in file order until IEND or the end of the data (fewer than 12 bytes left):
//    PLTE and tRNS are collected (CRC verified), IDAT payloads are counted, ancillary chunks are
//    skipped, an unknown critical chunk is UNSUPPORTED. A chunk whose length runs past the file,
//    a PLTE / tRNS of an impossible length or with a bad CRC, colour type 3 without PLTE and a file
//    without IDAT are MALFORMED.
//  * the IDAT CRCs are not verified: the payloads are one zlib stream whose Adler-32 the inflate
//    checks.
// The number of IDAT chunks is unbounded (a writer may split the stream at every byte), so the
// result names the first one and the payload total; pngd_idat_next() steps from one to the next.
#pragma once
#include <stdint.h>

#include "icx_jpeg.h"  // ICX_HD

namespace icx {

// include/icx.h icx_png_read_result
enum : int32_t {
    kPngrOk = 0, kPngrNotPng = 1, kPngrBadHeader = 2, kPngrUnsupported = 3, kPngrMalformed = 4, kPngrBadData = 5,
    kPngrTooLarge = 6
};
constexpr uint32_t kPngrMaxPixels = 0x1000000;  // checkSize (codecs.cpp:881-892)

struct PngdInfo {
    int32_t w, h, bd, ct;
    int32_t bw;          // filter unit: bytes per complete pixel, at least 1 (1, 2, 3, 4, 6, 8)
    int32_t lb;          // bytes per row without the filter byte
    int32_t npal;        // PLTE entries (colour type 3)
    int32_t has_key;     // colour types 0 and 2 with tRNS
    uint32_t key[3];     // at file precision (grey: key[0])
    int64_t first_idat;  // file offset of the first IDAT chunk (its length field)
    int64_t idat_bytes;  // all IDAT payloads together
    uint32_t pal[256];   // R | G << 8 | B << 16 | A << 24 (the output's byte order)
};

ICX_HD uint32_t pngd_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}
// CRC-32 (PNG spec annex D) bit by bit: only IHDR, PLTE and tRNS go through it (at most 1 KiB).
ICX_HD uint32_t pngd_crc(const uint8_t* p, int64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}
ICX_HD bool pngd_is(const uint8_t* t, char a, char b, char c, char d) {
    return t[0] == (uint8_t)a && t[1] == (uint8_t)b && t[2] == (uint8_t)c && t[3] == (uint8_t)d;
}
// The chunk at p (its length field): false at the end of the data (fewer than 12 bytes left);
// *len = its payload length, or -1 when it runs past the file.
ICX_HD bool pngd_chunk_at(const uint8_t* d, int64_t n, int64_t p, int64_t* len) {
    if (p < 0 || n - p < 12) return false;
    const int64_t l = (int64_t)pngd_be32(d + p);
    *len = l > n - p - 12 ? -1 : l;
    return true;
}
// From the IDAT chunk at p (a chunk pngd_walk accepted) to the next IDAT chunk before IEND or
// the end of the data, or -1.
ICX_HD int64_t pngd_idat_next(const uint8_t* d, int64_t n, int64_t p) {
    int64_t len;
    if (!pngd_chunk_at(d, n, p, &len) || len < 0) return -1;
    for (p += 12 + len; pngd_chunk_at(d, n, p, &len) && len >= 0; p += 12 + len) {
        if (pngd_is(d + p + 4, 'I', 'D', 'A', 'T')) return p;
        if (pngd_is(d + p + 4, 'I', 'E', 'N', 'D')) return -1;
    }
    return -1;
}

ICX_HD int pngd_walk(const uint8_t* d, int64_t n, PngdInfo& I) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    I.w = I.h = I.bd = I.ct = I.bw = I.lb = I.npal = I.has_key = 0;
    I.key[0] = I.key[1] = I.key[2] = 0;
    I.first_idat = -1;
    I.idat_bytes = 0;
    if (n < 8) return kPngrNotPng;
    for (int i = 0; i < 8; ++i)
        if (d[i] != sig[i]) return kPngrNotPng;
    for (int i = 0; i < 256; ++i) I.pal[i] = 0xFF000000u;  // (0, 0, 0, 255)
    int64_t p = 8, len;
    if (!pngd_chunk_at(d, n, p, &len) || len != 13 || !pngd_is(d + p + 4, 'I', 'H', 'D', 'R')) return kPngrBadHeader;
    if (pngd_crc(d + p + 4, 17) != pngd_be32(d + p + 21)) return kPngrBadHeader;
    const uint8_t* q = d + p + 8;
    const uint32_t w = pngd_be32(q), h = pngd_be32(q + 4);
    const int bd = q[8], ct = q[9];
    if (w == 0 || h == 0 || q[10] != 0 || q[11] != 0) return kPngrBadHeader;
    int ch;
    bool depth_ok;
    switch (ct) {
        case 0: ch = 1; depth_ok = bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16; break;
        case 2: ch = 3; depth_ok = bd == 8 || bd == 16; break;
        case 3: ch = 1; depth_ok = bd == 1 || bd == 2 || bd == 4 || bd == 8; break;
        case 4: ch = 2; depth_ok = bd == 8 || bd == 16; break;
        case 6: ch = 4; depth_ok = bd == 8 || bd == 16; break;
        default: return kPngrBadHeader;
    }
    if (!depth_ok) return kPngrBadHeader;
    if (q[12] != 0) return kPngrUnsupported;  // Adam7 (or an unknown interlace method)
    if (w > kPngrMaxPixels || h > kPngrMaxPixels || (uint64_t)w * h > kPngrMaxPixels) return kPngrTooLarge;
    I.w = (int32_t)w;
    I.h = (int32_t)h;
    I.bd = bd;
    I.ct = ct;
    const int bpp = ch * bd;
    I.bw = bpp >= 8 ? bpp / 8 : 1;
    I.lb = (int32_t)(((int64_t)w * bpp + 7) / 8);  // (at most 2^27)
    bool have_plte = false;
    int ntrns = 0;
    for (p += 12 + 13; pngd_chunk_at(d, n, p, &len); p += 12 + len) {
        if (len < 0) return kPngrMalformed;
        const uint8_t* t = d + p + 4;
        const uint8_t* body = t + 4;
        if (pngd_is(t, 'I', 'E', 'N', 'D')) break;
        if (pngd_is(t, 'I', 'D', 'A', 'T')) {
            if (I.first_idat < 0) I.first_idat = p;
            I.idat_bytes += len;
        } else if (pngd_is(t, 'P', 'L', 'T', 'E')) {
            if (len == 0 || len > 768 || len % 3 != 0) return kPngrMalformed;
            if (pngd_crc(t, 4 + len) != pngd_be32(body + len)) return kPngrMalformed;
            I.npal = (int32_t)(len / 3);
            for (int i = 0; i < I.npal; ++i)
                I.pal[i] = (I.pal[i] & 0xFF000000u) | body[3 * i] | (uint32_t)body[3 * i + 1] << 8 | (uint32_t)body[3 * i + 2] << 16;
            have_plte = true;
        } else if (pngd_is(t, 't', 'R', 'N', 'S')) {
            if (len > 256) return kPngrMalformed;
            if (pngd_crc(t, 4 + len) != pngd_be32(body + len)) return kPngrMalformed;
            if (ct == 0 || ct == 2) {
                const int nk = ct == 0 ? 1 : 3;
                if (len != 2 * nk) return kPngrMalformed;
                for (int k = 0; k < nk; ++k) I.key[k] = (uint32_t)body[2 * k] << 8 | body[2 * k + 1];
                I.has_key = 1;
            } else if (ct == 3) {
                ntrns = (int)len;
                for (int i = 0; i < ntrns; ++i) I.pal[i] = (I.pal[i] & 0x00FFFFFFu) | (uint32_t)body[i] << 24;
            }  // (colour types 4 and 6 carry their alpha: a tRNS there is ignored)
        } else if (!(t[0] & 0x20)) {
            return kPngrUnsupported;  // a critical chunk this reader does not know
        }
    }
    if (ct == 3) {
        if (!have_plte) return kPngrMalformed;
        for (int i = I.npal; i < 256; ++i) I.pal[i] = 0xFF000000u;  // an index past PLTE: (0, 0, 0, 255)
    }
    if (I.first_idat < 0) return kPngrMalformed;
    return kPngrOk;
}

}  // namespace icx
