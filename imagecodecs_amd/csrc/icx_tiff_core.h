// icx_tiff_core.h -- the arithmetic of the TIFF read (Image::readTiff, codecs.cpp:1439-1484, which
// hands the file to libtiff's TIFFReadRGBAImage), host and device: endian-aware reads, the walk of
// the first IFD into a TiffHead with its result codes, the geometry of chunk k (a strip or a tile),
// the closed form for where the k-th LZW code after a Clear starts and how wide it is, and a serial
// decode of a whole image (the zlib inflate is the caller's: the project's own needs hipcc). Plain
// C++: the CPU test builds it with g++ (tests/test_tiff_core.py), icx_tiff.hip with hipcc. The
// contract is written out in include/icx.h.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_TIFF_HD __host__ __device__ inline
#else
#define ICX_TIFF_HD inline
#endif

namespace icx {

// include/icx.h ICX_TIFF_*.
enum : int32_t {
    kTiffOk = 0, kTiffNotTiff = 1, kTiffBadHeader = 2, kTiffUnsupported = 3, kTiffMalformed = 4, kTiffBadData = 5,
    kTiffTruncated = 6, kTiffTooLarge = 7
};

constexpr int kTiffMaxChunks = 4096;      // chunks per image
constexpr int kTiffLzwLastT = 3837;       // the last code number after a Clear that may add an entry (257 + t = 4094)

// What the IFD walk finds (the descriptor record of k_tiff_parse).
struct TiffHead {
    int32_t w, h, spp, d;        // d: output channels
    int32_t photo, comp, pred;   // pred: 2 only where it is honoured (compression 5 / 8 / 32946)
    int32_t tiled, be;
    int32_t cw, ch;              // a chunk's width in pixels (strips: w) and its rows
    int32_t across, down, nchunks;
    int32_t off_type, cnt_type;  // 3 SHORT, 4 LONG
    int64_t off_at, cnt_at;      // file offsets of the chunk offset and byte-count arrays
    int64_t cmap_at;             // of the ColorMap's 768 SHORTs
};

ICX_TIFF_HD uint32_t tiff_u16(const uint8_t* p, int be) { return be ? (uint32_t)p[0] << 8 | p[1] : (uint32_t)p[1] << 8 | p[0]; }
ICX_TIFF_HD uint32_t tiff_u32(const uint8_t* p, int be) {
    return be ? (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]
              : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
}
// element k of a SHORT (3) or LONG (4) array
ICX_TIFF_HD uint32_t tiff_elem(const uint8_t* f, int64_t at, int type, int be, int64_t k) {
    return type == 3 ? tiff_u16(f + at + 2 * k, be) : tiff_u32(f + at + 4 * k, be);
}

// The IFD walk. Every byte read lies inside [0, n). The order of the checks is the contract's
// (include/icx.h): header, then the entries in file order (type / count, then the array's extent),
// then what the tags say together.
ICX_TIFF_HD int tiff_parse(const uint8_t* f, int64_t n, TiffHead* H) {
    *H = TiffHead{};
    if (n < 8) return kTiffNotTiff;
    int be;
    if (f[0] == 'I' && f[1] == 'I') be = 0;
    else if (f[0] == 'M' && f[1] == 'M') be = 1;
    else return kTiffNotTiff;
    const uint32_t magic = tiff_u16(f + 2, be);
    if (magic == 43) return kTiffUnsupported;  // BigTIFF
    if (magic != 42) return kTiffNotTiff;
    H->be = be;
    const int64_t ifd = tiff_u32(f + 4, be);
    if (ifd + 2 > n) return kTiffBadHeader;
    const int64_t ne = tiff_u16(f + ifd, be);
    if (ifd + 2 + 12 * ne > n) return kTiffBadHeader;

    uint32_t w = 0, h = 0, spp = 1, comp = 1, photo = 0xFFFFFFFFu, fill = 1, orient = 1, planar = 1, pred = 1;
    uint32_t rps = 0xFFFFFFFFu, tw = 0, tl = 0;
    bool has_w = false, has_h = false, has_bps = false, has_tw = false, has_tl = false, has_cmap = false;
    bool bps_ok = true, sf_ok = true;
    uint32_t bps_n = 0;
    bool has_so = false, has_sc = false, has_to = false, has_tc = false;
    int64_t so_at = 0, sc_at = 0, to_at = 0, tc_at = 0;
    uint32_t so_n = 0, sc_n = 0, to_n = 0, tc_n = 0;
    int so_t = 0, sc_t = 0, to_t = 0, tc_t = 0;
    for (int64_t e = 0; e < ne; ++e) {
        const uint8_t* p = f + ifd + 2 + 12 * e;
        const uint32_t tag = tiff_u16(p, be), type = tiff_u16(p + 2, be), count = tiff_u32(p + 4, be);
        bool scalar = false, array = false, short_only = false;
        switch (tag) {
            case 256: case 257: case 259: case 262: case 266: case 274: case 277: case 278: case 284: case 317: case 322:
            case 323: scalar = true; break;
            case 273: case 279: case 324: case 325: array = true; break;
            case 258: case 320: case 339: array = true; short_only = true; break;
            default: break;
        }
        if (!scalar && !array) continue;  // an unknown tag
        if (!(type == 3 || (type == 4 && !short_only))) return kTiffMalformed;
        if (scalar ? count != 1 : count == 0) return kTiffMalformed;
        if (tag == 320 && count != 768) return kTiffMalformed;
        const int64_t bytes = (int64_t)count * (type == 3 ? 2 : 4);
        int64_t at = ifd + 2 + 12 * e + 8;
        if (bytes > 4) {
            at = tiff_u32(p + 8, be);
            if (at + bytes > n) return kTiffTruncated;
        }
        const uint32_t v = tiff_elem(f, at, (int)type, be, 0);
        switch (tag) {
            case 256: w = v; has_w = true; break;
            case 257: h = v; has_h = true; break;
            case 258:
                has_bps = true;
                bps_n = count;
                bps_ok = true;
                for (uint32_t k = 0; k < count && k < 4; ++k) bps_ok = bps_ok && tiff_elem(f, at, 3, be, k) == 8;
                break;
            case 259: comp = v; break;
            case 262: photo = v; break;
            case 266: fill = v; break;
            case 273: has_so = true; so_at = at; so_n = count; so_t = (int)type; break;
            case 274: orient = v; break;
            case 277: spp = v; break;
            case 278: rps = v; break;
            case 279: has_sc = true; sc_at = at; sc_n = count; sc_t = (int)type; break;
            case 284: planar = v; break;
            case 317: pred = v; break;
            case 320: has_cmap = true; H->cmap_at = at; break;
            case 322: tw = v; has_tw = true; break;
            case 323: tl = v; has_tl = true; break;
            case 324: has_to = true; to_at = at; to_n = count; to_t = (int)type; break;
            case 325: has_tc = true; tc_at = at; tc_n = count; tc_t = (int)type; break;
            case 339:
                sf_ok = true;
                for (uint32_t k = 0; k < count && k < 4; ++k) sf_ok = sf_ok && tiff_elem(f, at, 3, be, k) == 1;
                break;
            default: break;
        }
    }
    if (!has_w || !has_h || w == 0 || h == 0) return kTiffBadHeader;
    if (!has_so && !has_to) return kTiffBadHeader;
    // what this read does not take
    if (!has_bps || !(spp == 1 || spp == 3 || spp == 4) || bps_n != spp || !bps_ok) return kTiffUnsupported;
    if (!(comp == 1 || comp == 5 || comp == 8 || comp == 32946 || comp == 32773)) return kTiffUnsupported;
    if (!(((photo == 0 || photo == 1 || photo == 3) && spp == 1) || (photo == 2 && spp >= 3))) return kTiffUnsupported;
    if (!(planar == 1 || (planar == 2 && spp == 1))) return kTiffUnsupported;
    if (orient != 1 || fill != 1 || !sf_ok || !(pred == 1 || pred == 2)) return kTiffUnsupported;
    // what the tags say together
    const bool strips = has_so || has_sc, tiles = has_to || has_tc || has_tw || has_tl;
    if (strips && tiles) return kTiffMalformed;
    uint64_t cw, ch;
    if (tiles) {
        if (!has_to || !has_tc || !has_tw || !has_tl || tw == 0 || tl == 0) return kTiffMalformed;
        cw = tw;
        ch = tl;
    } else {
        if (!has_sc || rps == 0) return kTiffMalformed;
        cw = w;
        ch = rps < h ? rps : h;
    }
    const uint64_t across = (w + cw - 1) / cw, down = (h + ch - 1) / ch, nchunks = across * down;
    const uint32_t on = tiles ? to_n : so_n, cn = tiles ? tc_n : sc_n;
    if (on != nchunks || cn != nchunks) return kTiffMalformed;
    if (photo == 3 && !has_cmap) return kTiffMalformed;
    // sizes
    if (cw > (1u << 30) || ch > (1u << 30) || (uint64_t)w * h > (1ull << 30) || nchunks > (uint64_t)kTiffMaxChunks) return kTiffTooLarge;
    if ((across * cw) * (down * ch) > (1ull << 30) || cw * ch * spp >= (1ull << 31)) return kTiffTooLarge;
    H->w = (int32_t)w;
    H->h = (int32_t)h;
    H->spp = (int32_t)spp;
    H->d = photo == 3 ? 3 : (int32_t)spp;
    H->photo = (int32_t)photo;
    H->comp = (int32_t)comp;
    H->pred = (pred == 2 && (comp == 5 || comp == 8 || comp == 32946)) ? 2 : 1;
    H->tiled = tiles;
    H->cw = (int32_t)cw;
    H->ch = (int32_t)ch;
    H->across = (int32_t)across;
    H->down = (int32_t)down;
    H->nchunks = (int32_t)nchunks;
    H->off_type = tiles ? to_t : so_t;
    H->cnt_type = tiles ? tc_t : sc_t;
    H->off_at = tiles ? to_at : so_at;
    H->cnt_at = tiles ? tc_at : sc_at;
    return kTiffOk;
}

// Chunk k: its rectangle on the image (clipped), the bytes it must decompress to, and where its
// decompressed bytes sit in the image's scratch (each chunk's room rounded up to 16 bytes).
struct TiffChunk {
    int32_t x0, y0, cols, rows;  // the visible rectangle
    uint32_t want;               // rows_in_chunk * row_bytes (a tile is always full size)
    uint32_t row_bytes;          // cw * spp
};
ICX_TIFF_HD uint32_t tiff_chunk_room(const TiffHead& H) { return ((uint32_t)H.cw * (uint32_t)H.ch * (uint32_t)H.spp + 15u) & ~15u; }
ICX_TIFF_HD TiffChunk tiff_chunk(const TiffHead& H, int k) {
    TiffChunk c;
    const int cx = k % H.across, cy = k / H.across;
    c.x0 = cx * H.cw;  // (< w: no overflow)
    c.y0 = cy * H.ch;
    c.cols = H.w - c.x0 < H.cw ? H.w - c.x0 : H.cw;
    c.rows = H.h - c.y0 < H.ch ? H.h - c.y0 : H.ch;
    c.row_bytes = (uint32_t)H.cw * (uint32_t)H.spp;
    c.want = (uint32_t)(H.tiled ? H.ch : c.rows) * c.row_bytes;
    return c;
}
// Bytes of scratch the image needs.
ICX_TIFF_HD uint64_t tiff_scratch_need(const TiffHead& H) { return (uint64_t)H.nchunks * tiff_chunk_room(H); }
// Bytes of scratch a batch slot has for images of up to max_w x max_h.
ICX_TIFF_HD uint64_t tiff_scratch_slot(int64_t max_w, int64_t max_h) {
    const uint64_t px = (uint64_t)max_w * (uint64_t)max_h;
    return ((4 * px + 15) & ~(uint64_t)15) + 16 * (px < (uint64_t)kTiffMaxChunks ? px : (uint64_t)kTiffMaxChunks);
}

// LZW codes are numbered t = 0, 1, ... from the one after a Clear. Code t >= 1 adds table entry
// 257 + t, and ("early change") a code is read one bit wider once the next free entry is 2^w - 1:
// code t is wider than w bits from t = 2^w - 258 on (254, 766, 1790).
ICX_TIFF_HD int tiff_code_width(uint32_t t) { return 9 + (t >= 254u) + (t >= 766u) + (t >= 1790u); }
// Bits between the end of the Clear and the start of code t.
ICX_TIFF_HD uint64_t tiff_code_offset(uint32_t t) {
    return (uint64_t)t * 9 + (t > 254u ? t - 254u : 0u) + (t > 766u ? t - 766u : 0u) + (t > 1790u ? t - 1790u : 0u);
}
// `width` bits from bit `bit` of s, MSB first; bytes at or past cnt read as 0.
ICX_TIFF_HD int tiff_msb_bits(const uint8_t* s, int64_t cnt, uint64_t bit, int width) {
    const int64_t b = (int64_t)(bit >> 3);
    const uint32_t v = (b < cnt ? (uint32_t)s[b] << 16 : 0u) | (b + 1 < cnt ? (uint32_t)s[b + 1] << 8 : 0u) |
                       (b + 2 < cnt ? (uint32_t)s[b + 2] : 0u);
    return (int)((v >> (24 - (int)(bit & 7) - width)) & ((1u << width) - 1u));
}
ICX_TIFF_HD bool tiff_lzw_old_style(const uint8_t* s, int64_t cnt) { return cnt >= 2 && s[0] == 0 && (s[1] & 1); }

// ------------------------------------------------------------------ serial chunk decoders
// Each decodes exactly `want` bytes into dst or says why not.
ICX_TIFF_HD int tiff_lzw_serial(const uint8_t* s, int64_t cnt, uint8_t* dst, uint32_t want) {
    if (tiff_lzw_old_style(s, cnt)) return kTiffUnsupported;
    uint16_t prefix[4096], len[4096];
    uint8_t suffix[4096], first[4096];
    uint64_t bit = 0;
    uint32_t t = 0, out = 0;
    bool started = false;
    int prev = 0;
    while (out < want) {
        const int width = tiff_code_width(t);
        if (bit + width > (uint64_t)cnt * 8) return kTiffBadData;
        const int code = tiff_msb_bits(s, cnt, bit, width);
        bit += width;
        if (!started) {
            if (code != 256) return kTiffBadData;
            started = true;
            continue;
        }
        if (code == 256) { t = 0; continue; }
        if (code == 257) return kTiffBadData;  // the data ends before `want` bytes
        if (t == 0) {
            if (code >= 256) return kTiffBadData;
            dst[out++] = (uint8_t)code;
            prev = code;
            t = 1;
            continue;
        }
        const int entry = 257 + (int)t;
        if (t > (uint32_t)kTiffLzwLastT || code > entry) return kTiffBadData;
        const int pf = prev < 256 ? prev : first[prev], pl = prev < 256 ? 1 : len[prev];
        const int cf = code < 256 ? code : code == entry ? pf : first[code];
        prefix[entry] = (uint16_t)prev;
        suffix[entry] = (uint8_t)cf;
        first[entry] = (uint8_t)pf;
        len[entry] = (uint16_t)(pl + 1);
        const uint32_t L = code < 256 ? 1u : len[code];
        int c = code;
        for (uint32_t k = L; k-- > 0;) {
            const int b = c < 256 ? c : suffix[c];
            if (c >= 256) c = prefix[c];
            if (out + k < want) dst[out + k] = (uint8_t)b;
        }
        out = out + L < want ? out + L : want;
        prev = code;
        ++t;
    }
    return kTiffOk;
}

ICX_TIFF_HD int tiff_packbits_serial(const uint8_t* s, int64_t cnt, uint8_t* dst, uint32_t want) {
    int64_t p = 0;
    uint32_t out = 0;
    while (out < want) {
        if (p >= cnt) return kTiffBadData;
        const int hb = s[p];
        if (hb == 128) { ++p; continue; }
        const uint32_t m = hb < 128 ? (uint32_t)hb + 1u : 257u - (uint32_t)hb;
        const int64_t need = hb < 128 ? 1 + (int64_t)m : 2;
        if (p + need > cnt) return kTiffBadData;
        const uint32_t mm = m < want - out ? m : want - out;
        for (uint32_t k = 0; k < mm; ++k) dst[out + k] = hb < 128 ? s[p + 1 + k] : s[p + 1];
        out += mm;
        p += need;
    }
    return kTiffOk;
}

// The whole image: out holds w * h * d bytes, scratch tiff_chunk_room(H) bytes. The image's code
// is its lowest-numbered failing chunk's. inflate(src, n, dst, want) is true when the zlib stream
// src[0, n) gives exactly `want` bytes (refusing a longer one before it stores a byte past want).
template <class Inflate>
inline int tiff_decode_serial(const uint8_t* f, int64_t n, const TiffHead& H, uint8_t* out, uint8_t* scratch, Inflate&& inflate) {
    for (int k = 0; k < H.nchunks; ++k) {
        const TiffChunk c = tiff_chunk(H, k);
        const int64_t off = tiff_elem(f, H.off_at, H.off_type, H.be, k), cnt = tiff_elem(f, H.cnt_at, H.cnt_type, H.be, k);
        if (off + cnt > n) return kTiffTruncated;
        const uint8_t* src = f + off;
        const uint8_t* px = scratch;
        int rc = kTiffOk;
        if (H.comp == 1) {
            if (cnt < (int64_t)c.want) rc = kTiffBadData;
            px = src;
        } else if (H.comp == 5) {
            rc = tiff_lzw_serial(src, cnt, scratch, c.want);
        } else if (H.comp == 32773) {
            rc = tiff_packbits_serial(src, cnt, scratch, c.want);
        } else {
            if (!inflate(src, cnt, scratch, c.want)) rc = kTiffBadData;
        }
        if (rc != kTiffOk) return rc;
        for (int y = 0; y < c.rows; ++y) {
            const uint8_t* row = px + (uint64_t)y * c.row_bytes;
            uint8_t acc[4] = {0, 0, 0, 0};
            for (int x = 0; x < c.cols; ++x) {
                uint8_t v[4];
                for (int s = 0; s < H.spp; ++s) {
                    v[s] = row[x * H.spp + s];
                    if (H.pred == 2) v[s] = acc[s] = (uint8_t)(acc[s] + v[s]);
                }
                uint8_t* o = out + ((uint64_t)(c.y0 + y) * H.w + (c.x0 + x)) * H.d;
                if (H.photo == 3) {
                    for (int s = 0; s < 3; ++s) o[s] = (uint8_t)(tiff_u16(f + H.cmap_at + 2 * (256 * s + v[0]), H.be) >> 8);
                } else {
                    for (int s = 0; s < H.spp; ++s) o[s] = H.photo == 0 ? (uint8_t)(255 - v[s]) : v[s];
                }
            }
        }
    }
    return kTiffOk;
}

}  // namespace icx
