// icx_gif_core.h -- the arithmetic of the GIF read (Image::readGif, codecs.cpp:507-542; gd_open_gif /
// gd_get_frame / gd_render_frame, gif.cpp:43-524), host and device: the container walk to the
// first image descriptor with its result codes, the closed form for where the k-th code after a
// clear code starts and how wide it is, and the interlace row map with its inverse. Plain C++:
// the CPU test builds it with g++ (tests/test_gif_core.py), icx_gif.hip with hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_GIF_HD __host__ __device__ inline
#else
#define ICX_GIF_HD inline
#endif

namespace icx {

// include/icx.h ICX_GIF_*.
enum : int32_t {
    kGifOk = 0, kGifNotGif = 1, kGifBadHeader = 2, kGifMalformed = 3, kGifBadData = 4, kGifTruncated = 5, kGifTooLarge = 6
};

// What the container walk finds (the descriptor record of k_gif_parse).
struct GifHead {
    int32_t w, h;            // logical screen
    int32_t fx, fy, fw, fh;  // the first frame's rectangle as the descriptor states it (fw, fh unclipped)
    int32_t has_image;       // 0: ';' came first -- a background-only canvas
    int32_t interlace;
    int32_t pal_size;        // entries of the active table (local if present, else global)
    int32_t bg_index;        // the header's background index: what pixels the stream did not reach hold
    int32_t bg_rgb;          // R | G << 8 | B << 16 of the canvas (0: no global table, or the index is outside it)
    int32_t transparent;     // the transparent index, -1: none
    int32_t mcs;             // minimum code size, 2..8
    int32_t pad_;
    int64_t pal_at;          // file offset of the active table
    int64_t data_at;         // file offset of the first data sub-block's size byte
};

ICX_GIF_HD int gif_u16(const uint8_t* p) { return p[0] | p[1] << 8; }

// The container walk. Every byte read lies inside [0, n).
ICX_GIF_HD int gif_parse(const uint8_t* f, int64_t n, GifHead* H) {
    *H = GifHead{};
    H->transparent = -1;
    if (n >= 6 && !(f[0] == 'G' && f[1] == 'I' && f[2] == 'F' && f[3] == '8' && (f[4] == '7' || f[4] == '9') && f[5] == 'a'))
        return kGifNotGif;
    if (n < 13) return kGifBadHeader;
    H->w = gif_u16(f + 6);
    H->h = gif_u16(f + 8);
    if (H->w == 0 || H->h == 0) return kGifBadHeader;
    const int flags = f[10];
    H->bg_index = f[11];
    int64_t p = 13, gct_at = 0;
    int gct_size = 0;
    if (flags & 0x80) {
        gct_size = 1 << ((flags & 7) + 1);
        gct_at = p;
        p += 3 * gct_size;
        if (p > n) return kGifTruncated;
        if (H->bg_index < gct_size) {
            const uint8_t* c = f + gct_at + 3 * H->bg_index;
            H->bg_rgb = c[0] | c[1] << 8 | c[2] << 16;
        }
    }
    for (;;) {
        if (p >= n) return kGifTruncated;
        const int sep = f[p];
        if (sep == ';') return kGifOk;
        if (sep == '!') {
            if (p + 1 >= n) return kGifTruncated;
            const int label = f[p + 1];
            p += 2;
            for (bool first = true;; first = false) {  // the sub-block chain, whatever the label
                if (p >= n) return kGifTruncated;
                const int sz = f[p];
                if (sz == 0) { ++p; break; }
                if (p + 1 + sz > n) return kGifTruncated;
                if (first && label == 0xF9 && sz >= 4) H->transparent = (f[p + 1] & 1) ? f[p + 4] : -1;
                p += 1 + sz;
            }
            continue;
        }
        if (sep != ',') return kGifMalformed;
        if (p + 10 > n) return kGifTruncated;
        H->fx = gif_u16(f + p + 1);
        H->fy = gif_u16(f + p + 3);
        H->fw = gif_u16(f + p + 5);
        H->fh = gif_u16(f + p + 7);
        const int fl = f[p + 9];
        p += 10;
        if (H->fx >= H->w || H->fy >= H->h) return kGifMalformed;
        if (!(fl & 0x80) && !gct_size) return kGifMalformed;
        H->interlace = (fl >> 6) & 1;
        H->pal_size = gct_size;
        H->pal_at = gct_at;
        if (fl & 0x80) {
            H->pal_size = 1 << ((fl & 7) + 1);
            H->pal_at = p;
            p += 3 * H->pal_size;
            if (p > n) return kGifTruncated;
        }
        if (p >= n) return kGifTruncated;
        H->mcs = f[p];
        if (H->mcs < 2 || H->mcs > 8) return kGifBadData;
        H->data_at = p + 1;
        H->has_image = 1;
        return kGifOk;
    }
}

// Codes are numbered t = 0, 1, ... from the one after a clear code. Code t >= 1 adds table entry
// (1 << mcs) + 1 + t while the table has room, and a code is read one bit wider once the next free
// entry is a power of two, up to 12 bits: code t is wider than w bits from t = (1 << w) - (1 << mcs) - 1 on.
ICX_GIF_HD int gif_code_width(int mcs, uint32_t t) {
    int w = mcs + 1;
    for (int b = mcs + 1; b < 12; ++b) w += t >= (1u << b) - (1u << mcs) - 1u;
    return w;
}
// Bits between the end of the clear code and the start of code t.
ICX_GIF_HD uint64_t gif_code_offset(int mcs, uint32_t t) {
    uint64_t o = (uint64_t)t * (mcs + 1);
    for (int b = mcs + 1; b < 12; ++b) {
        const uint32_t s = (1u << b) - (1u << mcs) - 1u;
        if (t > s) o += t - s;
    }
    return o;
}

// Rows of the four passes (every 8th from 0, every 8th from 4, every 4th from 2, every 2nd from 1)
// before stream row r's pass, and the frame row of stream row r; h is the descriptor's height.
ICX_GIF_HD int gif_interlace_row(int h, int r) {
    const int p1 = (h + 7) / 8, p2 = (h + 3) / 8, p3 = (h + 1) / 4;
    if (r < p1) return r * 8;
    r -= p1;
    if (r < p2) return r * 8 + 4;
    r -= p2;
    if (r < p3) return r * 4 + 2;
    return (r - p3) * 2 + 1;
}
// Its inverse: the stream row that holds frame row y.
ICX_GIF_HD int gif_interlace_stream_row(int h, int y) {
    const int p1 = (h + 7) / 8, p2 = (h + 3) / 8, p3 = (h + 1) / 4;
    if ((y & 7) == 0) return y >> 3;
    if ((y & 7) == 4) return p1 + (y >> 3);
    if ((y & 3) == 2) return p1 + p2 + (y >> 2);
    return p1 + p2 + p3 + (y >> 1);
}

}  // namespace icx
