// icx_exrw_core.h -- the arithmetic of the OpenEXR write (Image::writeExr, codecs.cpp:495-505 ->
// tinyexr SaveEXR, tinyexr.h:9333-9480), host and device: float_to_half_full (:989-1026), the
// sample bytes of a scanline chunk (:7184-7232), CompressZip's reorder and predictor (:1326-1365)
// as a gather, and the file's header bytes (:7800-8024). Plain C++: the CPU test builds it with
// g++ (tests/test_exr_write_core.py), icx_exrw.hip with hipcc.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ICX_EXRW_HD __host__ __device__ inline
#else
#define ICX_EXRW_HD inline
#endif

namespace icx {

constexpr int kExrwZipLines = 16;  // NumScanlines(ZIP); NONE: 1

// One image as SaveEXR sees it. Channels in file order are the components in reverse (A,B,G,R /
// B,G,R / A), so file channel c reads component nch - 1 - c.
struct ExrwGeom {
    int32_t w, h, nch;
    int32_t s;      // bytes per sample: 4 (FLOAT, save_as_fp16 == 0) or 2 (HALF)
    int32_t lines;  // scanlines per chunk: 16 (ZIP) or 1 (NONE)
    int32_t zip;    // ZIP unless width < 16 && height < 16 (:9349-9355)
};

ICX_EXRW_HD ExrwGeom exrw_geom(int w, int h, int nch, int fp16) {
    ExrwGeom g;
    g.w = w;
    g.h = h;
    g.nch = nch;
    g.s = fp16 > 0 ? 2 : 4;
    g.zip = !(w < 16 && h < 16);
    g.lines = g.zip ? kExrwZipLines : 1;
    return g;
}
ICX_EXRW_HD int64_t exrw_nchunks(const ExrwGeom& g) { return ((int64_t)g.h + g.lines - 1) / g.lines; }
ICX_EXRW_HD int64_t exrw_line_bytes(const ExrwGeom& g) { return (int64_t)g.nch * g.w * g.s; }
// Sample bytes of chunk c (the last one may hold fewer lines).
ICX_EXRW_HD int64_t exrw_chunk_bytes(const ExrwGeom& g, int64_t c) {
    const int64_t y0 = c * g.lines, n = g.h - y0 < g.lines ? g.h - y0 : g.lines;
    return n * exrw_line_bytes(g);
}

// float_to_half_full on the bit patterns: denormals -> +-0, Inf / NaN -> exponent 31 (NaN:
// mantissa 0x200), overflow -> +-Inf, subnormal results from the shifted mantissa with its hidden
// bit, and rounding by adding the first dropped bit (it may carry into the exponent).
ICX_EXRW_HD uint16_t exrw_half(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u, fe = (f >> 23) & 255u, fm = f & 0x7FFFFFu;
    uint32_t o = 0;  // exponent << 10 | mantissa
    if (fe == 0) {
        o = 0;
    } else if (fe == 255) {
        o = (31u << 10) | (fm ? 0x200u : 0u);
    } else {
        const int newexp = (int)fe - 127 + 15;
        if (newexp >= 31) {
            o = 31u << 10;
        } else if (newexp <= 0) {
            if (14 - newexp <= 24) {
                const uint32_t mant = fm | 0x800000u;
                o = (mant >> (14 - newexp)) & 0x3FFu;
                if ((mant >> (13 - newexp)) & 1u) o += 1;
            }
        } else {
            o = ((uint32_t)newexp << 10) | (fm >> 13);
            if (fm & 0x1000u) o += 1;
        }
    }
    return (uint16_t)((o & 0x7FFFu) | sign);
}

// Byte i of the sample bytes of the chunk starting at line y0: per line, per file channel, w
// little-endian samples. px: the interleaved float pixels as bit patterns. A chunk's bytes are
// indexed with 32 bits (the host refuses a chunk of 2^31 bytes or more).
ICX_EXRW_HD uint32_t exrw_raw_byte(const uint32_t* px, const ExrwGeom& g, int64_t y0, uint32_t i) {
    const uint32_t ws = (uint32_t)g.w * (uint32_t)g.s, lb = ws * (uint32_t)g.nch, line = i / lb;
    const uint32_t r = i - line * lb;
    const uint32_t ch = r / ws, r2 = r - ch * ws;
    const uint32_t x = g.s == 2 ? r2 >> 1 : r2 >> 2;
    const uint32_t b = r2 & (uint32_t)(g.s - 1);
    uint32_t v = px[((y0 + line) * g.w + x) * g.nch + (g.nch - 1 - (int)ch)];
    if (g.s == 2) v = exrw_half(v);
    return (v >> (8 * b)) & 255u;
}
// Byte t after CompressZip's reorder: even-indexed bytes first, odd-indexed from (S + 1) / 2.
ICX_EXRW_HD uint32_t exrw_reordered_byte(const uint32_t* px, const ExrwGeom& g, int64_t y0, uint32_t S, uint32_t t) {
    const uint32_t half = (S + 1) / 2;
    return exrw_raw_byte(px, g, y0, t < half ? 2 * t : 2 * (t - half) + 1);
}
// Byte t of what tinyexr hands to zlib: t[i] - t[i-1] + 384, truncated; byte 0 as it is.
ICX_EXRW_HD uint32_t exrw_pred_byte(const uint32_t* px, const ExrwGeom& g, int64_t y0, uint32_t S, uint32_t t) {
    const uint32_t a = exrw_reordered_byte(px, g, y0, S, t);
    if (t == 0) return a;
    return (a - exrw_reordered_byte(px, g, y0, S, t - 1) + 384u) & 255u;
}

// ---- the file's bytes before the offset table (host)
inline void exrw_put_attr(std::vector<uint8_t>& m, const char* name, const char* type, const uint8_t* data, int len) {
    for (const char* p = name; *p; ++p) m.push_back((uint8_t)*p);
    m.push_back(0);
    for (const char* p = type; *p; ++p) m.push_back((uint8_t)*p);
    m.push_back(0);
    for (int k = 0; k < 4; ++k) m.push_back((uint8_t)((uint32_t)len >> (8 * k)));
    m.insert(m.end(), data, data + len);
}
inline void exrw_le32(uint8_t* p, uint32_t v) {
    for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
// Magic, version, and SaveEXRNPartImageToMemory's attributes in its order, then the 0.
inline std::vector<uint8_t> exrw_header(const ExrwGeom& g) {
    std::vector<uint8_t> m = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
    {
        static const char* const names[3] = {"A", "BGR", "ABGR"};
        const char* nm = names[g.nch == 1 ? 0 : g.nch == 3 ? 1 : 2];
        std::vector<uint8_t> d((size_t)g.nch * 18 + 1, 0);
        for (int c = 0; c < g.nch; ++c) {
            uint8_t* p = d.data() + (size_t)c * 18;
            p[0] = (uint8_t)nm[c];                  // name, 0
            exrw_le32(p + 2, g.s == 2 ? 1u : 2u);   // HALF / FLOAT
            exrw_le32(p + 10, 1);                   // (pLinear 0 + 3 pad bytes at p + 6) xSampling
            exrw_le32(p + 14, 1);                   // ySampling
        }
        exrw_put_attr(m, "channels", "chlist", d.data(), (int)d.size());
    }
    const uint8_t comp = g.zip ? 3 : 0;
    exrw_put_attr(m, "compression", "compression", &comp, 1);
    uint8_t box[16];
    exrw_le32(box, 0);
    exrw_le32(box + 4, 0);
    exrw_le32(box + 8, (uint32_t)(g.w - 1));
    exrw_le32(box + 12, (uint32_t)(g.h - 1));
    exrw_put_attr(m, "dataWindow", "box2i", box, 16);
    exrw_put_attr(m, "displayWindow", "box2i", box, 16);
    const uint8_t lo = 0;
    exrw_put_attr(m, "lineOrder", "lineOrder", &lo, 1);
    uint8_t one[4], zero2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    exrw_le32(one, 0x3F800000u);
    exrw_put_attr(m, "pixelAspectRatio", "float", one, 4);
    exrw_put_attr(m, "screenWindowCenter", "v2f", zero2, 8);
    exrw_put_attr(m, "screenWindowWidth", "float", one, 4);
    m.push_back(0);
    return m;
}
// Header + offset table + chunk headers + raw payloads: the largest file (a chunk whose stream
// is not smaller than its samples is stored raw).
inline uint64_t exrw_bound(const ExrwGeom& g) {
    const uint64_t nc = (uint64_t)exrw_nchunks(g);
    return exrw_header(g).size() + 16 * nc + (uint64_t)g.h * (uint64_t)exrw_line_bytes(g);
}

}  // namespace icx
