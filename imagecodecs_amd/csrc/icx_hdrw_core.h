// icx_hdrw_core.h -- the arithmetic of the Radiance .hdr write (Image::writeHdr, codecs.cpp:779-818,
// with invConvertComponent :604-608 taken by its evident intent), host and device: float -> RGBE
// for d = 4 (the read's inverse) and d = 3 (plain RGB), the header writer, the serial row packer
// that restates include/icx.h's rule, and a serial whole-file encode. Plain C++: the CPU test
// builds it with g++ (tests/test_hdr_write_core.py), icx_hdrw.hip with hipcc.
//
// Every step works on the floats' bits: 2^(136-E) is no binary32 number for E < 9 and a compile
// may flush subnormals, so no float product, ldexpf or frexpf is used.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define ICX_HDRW_HD __host__ __device__ inline
#else
#define ICX_HDRW_HD inline
#endif

namespace icx {

// include/icx.h ICX_HDR_* as the write uses them.
enum : int32_t { kHdrwOk = 0, kHdrwTooLarge = 5, kHdrwInvalidArgument = 6 };

constexpr int kHdrwHeadMax = 80;                  // room for the header: 52 up to "-Y ", 10 digits, " +X ", 10 digits, "\n" = 77
constexpr uint32_t kHdrwTinyBits = 0x0A4FB11Fu;   // 1e-32f, Radiance's setcolr threshold
constexpr uint32_t kHdrwFltMaxBits = 0x7F7FFFFFu;

ICX_HDRW_HD uint32_t hdrw_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

ICX_HDRW_HD bool hdrw_args_ok(int w, int h, int d) {
    return (d == 3 || d == 4) && w >= 1 && h >= 1 && (int64_t)w * h <= ((int64_t)1 << 30);
}

// A row is run-length coded when the caller asks for it and the width allows the 2, 2, hi, lo marker.
ICX_HDRW_HD bool hdrw_row_rle(int w, int rle) { return rle != 0 && w >= 8 && w <= 32767; }

// min(255, floor(v * 2^(136 - E))) of the float with these bits; 0 for NaN, negative values and
// +-0, 255 for +inf. v = sig * 2^e2 exactly, so the product is a shift of sig.
// (Written as selects, not branches: on the GPU every lane takes the same path.)
ICX_HDRW_HD uint32_t hdrw_mant(uint32_t bits, int E) {
    const int ex = (int)((bits >> 23) & 255u);
    const uint32_t frac = bits & 0x7FFFFFu;
    const uint32_t sig = ex ? frac | 0x800000u : frac;  // subnormal: frac * 2^-149
    const int sh = (ex ? ex : 1) - 150 + 136 - E;       // v * 2^(136 - E) = sig * 2^sh
    const int left = sh < 8 ? sh : 8, right = -sh < 31 ? -sh : 31;  // sig < 2^24: 8 left is >= 256 unless sig = 0
    uint32_t m = sh >= 0 ? sig << (left & 31) : sig >> (right & 31);
    m = m < 255u ? m : 255u;
    m = ex == 255 ? (frac ? 0u : 255u) : m;
    return (bits >> 31) ? 0u : m;
}

// E of d = 4: the fourth float truncated toward zero and clamped to 0..255; NaN gives 0.
// (Comparisons and a conversion only: a subnormal is 0 either way.)
ICX_HDRW_HD int hdrw_exp4(float ef) {
    const int t = (int)(ef >= 1.0f && ef < 255.0f ? ef : 0.0f);
    return ef >= 255.0f ? 255 : t;
}

ICX_HDRW_HD uint32_t hdrw_pack(uint32_t r, uint32_t g, uint32_t b, uint32_t e) { return r | g << 8 | b << 16 | e << 24; }

// d = 4: R, G, B, Ef -> the four bytes, R in the low byte.
ICX_HDRW_HD uint32_t hdrw_rgbe4(const float* p) {
    const int E = hdrw_exp4(p[3]);
    return hdrw_pack(hdrw_mant(hdrw_bits(p[0]), E), hdrw_mant(hdrw_bits(p[1]), E), hdrw_mant(hdrw_bits(p[2]), E), (uint32_t)E);
}

// d = 3: NaN and negative -> 0, +inf -> FLT_MAX; the largest component mx = f * 2^e, f in [0.5, 1),
// gives E = min(255, e + 128); below 1e-32f all four bytes are 0. Non-negative floats order as
// their bits do, and mx >= 1e-32f is a normal number whose e is its exponent field - 126.
ICX_HDRW_HD uint32_t hdrw_clean3(uint32_t bits) {
    const uint32_t v = (bits >> 23) == 255u ? ((bits & 0x7FFFFFu) ? 0u : kHdrwFltMaxBits) : bits;
    return (bits >> 31) ? 0u : v;
}
ICX_HDRW_HD uint32_t hdrw_rgbe3(const float* p) {
    const uint32_t r = hdrw_clean3(hdrw_bits(p[0])), g = hdrw_clean3(hdrw_bits(p[1])), b = hdrw_clean3(hdrw_bits(p[2]));
    uint32_t mx = r > g ? r : g;
    mx = mx > b ? mx : b;
    int E = (int)(mx >> 23) + 2;
    E = E < 255 ? E : 255;
    const uint32_t v = hdrw_pack(hdrw_mant(r, E), hdrw_mant(g, E), hdrw_mant(b, E), (uint32_t)E);
    return mx < kHdrwTinyBits ? 0u : v;
}
ICX_HDRW_HD uint32_t hdrw_rgbe(const float* p, int d) { return d == 4 ? hdrw_rgbe4(p) : hdrw_rgbe3(p); }

// The reference's header bytes (codecs.cpp:791) at o (room for kHdrwHeadMax); returns their number.
ICX_HDRW_HD int hdrw_put_int(uint8_t* o, int v) {
    char t[12];
    int k = 0;
    do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (int i = 0; i < k; ++i) o[i] = (uint8_t)t[k - 1 - i];
    return k;
}
ICX_HDRW_HD int hdrw_write_header(uint8_t* o, int w, int h) {
    const char a[] = "#?RADIANCE\nSOFTWARE=GEGL\nFORMAT=32-bit_rle_rgbe\n\n-Y ";
    int k = 0;
    for (; a[k]; ++k) o[k] = (uint8_t)a[k];
    k += hdrw_put_int(o + k, h);
    o[k++] = ' '; o[k++] = '+'; o[k++] = 'X'; o[k++] = ' ';
    k += hdrw_put_int(o + k, w);
    o[k++] = '\n';
    return k;
}
ICX_HDRW_HD int hdrw_header_len(int w, int h) {
    int k = 52 + 1 + 4 + 1 + 1;  // the text up to "-Y ", " +X ", the newline, one digit each
    for (int v = h; v >= 10; v /= 10) ++k;
    for (int v = w; v >= 10; v /= 10) ++k;
    return k;
}

ICX_HDRW_HD uint64_t hdrw_encode_bound(int w, int h, int d, int rle) {
    if (!hdrw_args_ok(w, h, d)) return 0;
    const uint64_t head = (uint64_t)hdrw_header_len(w, h);
    if (hdrw_row_rle(w, rle)) return head + (uint64_t)h * (4 + 4 * ((uint64_t)w + (w + 127) / 128));
    return head + 4 * (uint64_t)w * h;
}

// One component plane of a row (w bytes) packed by include/icx.h's rule, serial as stated: the
// bytes go to `out` (room for w + ceil(w/128)) and their number is returned.
ICX_HDRW_HD int hdrw_pack_plane(const uint8_t* p, int w, uint8_t* out) {
    int o = 0, i = 0;
    while (i < w) {
        int r = 1;
        while (r < 127 && i + r < w && p[i + r] == p[i]) ++r;
        if (r >= 4) {
            out[o++] = (uint8_t)(128 + r);
            out[o++] = p[i];
            i += r;
        } else {
            int n = 0;
            for (int k = i; k < w && k - i < 128; ++k) {
                if (k > i && k + 3 < w && p[k] == p[k + 1] && p[k] == p[k + 2] && p[k] == p[k + 3]) break;
                ++n;
            }
            out[o++] = (uint8_t)n;
            for (int k = 0; k < n; ++k) out[o++] = p[i + k];
            i += n;
        }
    }
    return o;
}

// The whole write, serial: the contract restated (and what a GPU result must equal). `out` has room
// for hdrw_encode_bound bytes; `tmp` for 4*w (the row's planes; unused when the file is flat).
// Returns the file's length.
ICX_HDRW_HD uint64_t hdrw_encode_serial(const float* px, int w, int h, int d, int rle, uint8_t* out, uint8_t* tmp) {
    uint64_t o = (uint64_t)hdrw_write_header(out, w, h);
    const bool packed = hdrw_row_rle(w, rle);
    for (int y = 0; y < h; ++y) {
        const float* row = px + (int64_t)y * w * d;
        if (!packed) {
            for (int x = 0; x < w; ++x) {
                const uint32_t v = hdrw_rgbe(row + (int64_t)x * d, d);
                out[o++] = (uint8_t)v;
                out[o++] = (uint8_t)(v >> 8);
                out[o++] = (uint8_t)(v >> 16);
                out[o++] = (uint8_t)(v >> 24);
            }
            continue;
        }
        for (int x = 0; x < w; ++x) {
            const uint32_t v = hdrw_rgbe(row + (int64_t)x * d, d);
            for (int c = 0; c < 4; ++c) tmp[(int64_t)c * w + x] = (uint8_t)(v >> (8 * c));
        }
        out[o++] = 2;
        out[o++] = 2;
        out[o++] = (uint8_t)(w >> 8);
        out[o++] = (uint8_t)(w & 255);
        for (int c = 0; c < 4; ++c) o += (uint64_t)hdrw_pack_plane(tmp + (int64_t)c * w, w, out + o);
    }
    return o;
}

}  // namespace icx
