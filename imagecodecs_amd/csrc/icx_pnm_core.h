// icx_pnm_core.h -- the arithmetic of the Netpbm read and write (Image::readPbm / writePbm,
// codecs.cpp:1034-1167), host and device: the byte classes, the header walk with its result
// codes (magic, width, height, maxval or scale), the length of a binary raster, a serial decode
// that restates the read contract of include/icx.h, the header writer and a serial encode that
// restates the write contract. Plain C++: the CPU test builds it with g++
// (tests/test_pnm_core.py), icx_pnm.hip with hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ICX_PNM_HD __host__ __device__ inline
#else
#define ICX_PNM_HD inline
#endif

namespace icx {

// Bytes of raster text per tile of the ASCII read (imagecodecs_amd.PNM_ASCII_TILE; the tests aim at
// its multiples).
constexpr int kPnmTile = 4096;

// include/icx.h ICX_PNM_*; kPnmPending is internal (the text of an ASCII file is still to be read).
enum : int32_t {
    kPnmOk = 0, kPnmNotPnm = 1, kPnmBadHeader = 2, kPnmUnsupported = 3, kPnmBadData = 4, kPnmTruncated = 5,
    kPnmTooLarge = 6, kPnmInvalidArgument = 7, kPnmPending = 8
};
enum : int32_t { kPnmUbyte = 0, kPnmUshort = 1, kPnmFloat = 2 };  // ImageCodecs::Type
enum : int32_t { kPnmP4 = 4, kPnmP5 = 5, kPnmP6 = 6, kPnmPF = 8 };  // ICX_PNM_P4 ... (write formats)
constexpr int64_t kPnmMaxPixels = (int64_t)1 << 30;

struct PnmHead {
    int32_t kind;    // the magic's second byte: '1' .. '6', 'f', 'F'
    int32_t w, h;
    int32_t d;       // 1, or 3 for P3, P6, PF
    int32_t type;    // kPnmUbyte / kPnmUshort / kPnmFloat
    int32_t maxval;  // P2, P3, P5, P6: the header's; P1, P4: 255 (the two values given out are 0 and 255); PF, Pf: 0
    int32_t ascii;   // P1, P2, P3
    int32_t le;      // PF, Pf: the scale is negative, the floats are little-endian
    int64_t rs;      // file offset of the raster
};

ICX_PNM_HD bool pnm_is_ws(int c) { return c == ' ' || (c >= 9 && c <= 13); }  // space, TAB, LF, VT, FF, CR
ICX_PNM_HD bool pnm_is_eol(int c) { return c == '\n' || c == '\r' ; }
ICX_PNM_HD bool pnm_is_digit(int c) { return c >= '0' && c <= '9'; }

// A byte of raster text outside a comment.
enum : int { kPnmClsWs = 0, kPnmClsDigit = 1, kPnmClsHash = 2, kPnmClsBad = 3 };
ICX_PNM_HD int pnm_class(int c, bool p1) {
    if (pnm_is_ws(c)) return kPnmClsWs;
    if (c == '#') return kPnmClsHash;
    if (p1 ? (c == '0' || c == '1') : pnm_is_digit(c)) return kPnmClsDigit;
    return kPnmClsBad;
}

// From pos over whitespace and comments ('#' up to and including the next LF or CR) to the first
// byte of a token, or to n.
ICX_PNM_HD int64_t pnm_skip(const uint8_t* f, int64_t n, int64_t pos) {
    while (pos < n) {
        const int c = f[pos];
        if (c == '#') {
            ++pos;
            while (pos < n && !pnm_is_eol(f[pos])) ++pos;
            if (pos < n) ++pos;
        } else if (pnm_is_ws(c)) {
            ++pos;
        } else {
            break;
        }
    }
    return pos;
}

// A token runs up to whitespace, a '#' or the end of the file.
ICX_PNM_HD int64_t pnm_token_end(const uint8_t* f, int64_t n, int64_t pos) {
    while (pos < n && !pnm_is_ws(f[pos]) && f[pos] != '#') ++pos;
    return pos;
}

// [a, b) as an unsigned number of 1 to 10 digits.
ICX_PNM_HD bool pnm_uint_token(const uint8_t* f, int64_t a, int64_t b, int64_t* v) {
    if (b - a < 1 || b - a > 10) return false;
    int64_t x = 0;
    for (int64_t p = a; p < b; ++p) {
        if (!pnm_is_digit(f[p])) return false;
        x = x * 10 + (f[p] - '0');
    }
    *v = x;
    return true;
}

// [a, b) as the scale of a PFM header: [+-]digits[.digits][e[+-]digits] ('e' or 'E'), not zero
// (some digit of the mantissa is not '0') and finite as a float. Decided on the decimal digits, with
// no floating-point arithmetic: the value is 0.S x 10^m, S the mantissa's digits from the first that
// is not '0'; it rounds to infinity exactly when it is at least 2^128 - 2^103, the 39 digits below.
ICX_PNM_HD bool pnm_scale_token(const uint8_t* f, int64_t a, int64_t b, int* negative) {
    const char* const kLimit = "340282356779733661637539395458142568448";
    int64_t p = a;
    *negative = 0;
    if (p < b && (f[p] == '+' || f[p] == '-')) {
        *negative = f[p] == '-';
        ++p;
    }
    const int64_t i0 = p;
    while (p < b && pnm_is_digit(f[p])) ++p;
    const int64_t ni = p - i0;
    if (ni == 0) return false;
    int64_t f0 = p, nf = 0;
    if (p < b && f[p] == '.') {
        f0 = ++p;
        while (p < b && pnm_is_digit(f[p])) ++p;
        nf = p - f0;
        if (nf == 0) return false;
    }
    int64_t ex = 0;
    if (p < b && (f[p] == 'e' || f[p] == 'E')) {
        ++p;
        bool eneg = false;
        if (p < b && (f[p] == '+' || f[p] == '-')) {
            eneg = f[p] == '-';
            ++p;
        }
        const int64_t e0 = p;
        while (p < b && pnm_is_digit(f[p])) {
            ex = ex * 10 + (f[p] - '0');
            if (ex > 1000000000) ex = 1000000000;
            ++p;
        }
        if (p == e0) return false;
        if (eneg) ex = -ex;
    }
    if (p != b) return false;
    const int64_t nd = ni + nf;  // the mantissa's digits: k < ni in the integer part, then the fraction
    int64_t k0 = 0;
    while (k0 < nd && f[k0 < ni ? i0 + k0 : f0 + (k0 - ni)] == '0') ++k0;
    if (k0 == nd) return false;  // zero
    const int64_t m = ni - k0 + ex;
    if (m != 39) return m < 39;
    for (int i = 0; i < 39; ++i) {
        const int64_t k = k0 + i;
        const int s = k < nd ? f[k < ni ? i0 + k : f0 + (k - ni)] : '0';
        if (s != kLimit[i]) return s < kLimit[i];
    }
    return false;
}

// The header walk: kPnmOk and *H, or NOT_PNM, UNSUPPORTED, BAD_HEADER, TOO_LARGE (more than 2^30
// pixels), in this order. The raster is not looked at.
ICX_PNM_HD int pnm_parse(const uint8_t* f, int64_t n, PnmHead* H) {
    if (n < 2 || f[0] != 'P') return kPnmNotPnm;
    const int c = f[1];
    if (!((c >= '1' && c <= '7') || c == 'F' || c == 'f')) return kPnmNotPnm;
    if (c == '7') return kPnmUnsupported;
    const bool flt = c == 'F' || c == 'f', bitmap = c == '1' || c == '4';
    H->kind = c;
    H->ascii = c >= '1' && c <= '3';
    H->d = (c == '3' || c == '6' || c == 'F') ? 3 : 1;
    H->le = 0;
    const int ntok = bitmap ? 2 : 3;
    int64_t v[3] = {0, 0, 0}, pos = 2;
    for (int k = 0; k < ntok; ++k) {
        pos = pnm_skip(f, n, pos);
        if (pos >= n) return kPnmBadHeader;
        const int64_t e = pnm_token_end(f, n, pos);
        if (k == 2 && flt) {
            int neg = 0;
            if (!pnm_scale_token(f, pos, e, &neg)) return kPnmBadHeader;
            H->le = neg;
        } else if (!pnm_uint_token(f, pos, e, &v[k])) {
            return kPnmBadHeader;
        }
        pos = e;
    }
    if (v[0] == 0 || v[1] == 0) return kPnmBadHeader;
    if (!bitmap && !flt && (v[2] < 1 || v[2] > 65535)) return kPnmBadHeader;
    if (!H->ascii) {  // exactly one whitespace byte, then the raster
        if (pos >= n || !pnm_is_ws(f[pos])) return kPnmBadHeader;
        ++pos;
    }
    H->rs = pos;
    H->maxval = flt ? 0 : bitmap ? 255 : (int32_t)v[2];
    H->type = flt ? kPnmFloat : H->maxval > 255 ? kPnmUshort : kPnmUbyte;
    if (v[0] > kPnmMaxPixels || v[1] > kPnmMaxPixels || v[0] * v[1] > kPnmMaxPixels) return kPnmTooLarge;
    H->w = (int32_t)v[0];
    H->h = (int32_t)v[1];
    return kPnmOk;
}

ICX_PNM_HD int pnm_elem_bytes(int type) { return type == kPnmFloat ? 4 : type == kPnmUshort ? 2 : 1; }
ICX_PNM_HD int64_t pnm_out_bytes(const PnmHead& H) { return (int64_t)H.w * H.h * H.d * pnm_elem_bytes(H.type); }
// The bytes of a binary raster (P4: rows padded to whole bytes).
ICX_PNM_HD int64_t pnm_raster_bytes(const PnmHead& H) {
    return H.kind == '4' ? (int64_t)H.h * ((H.w + 7) / 8) : pnm_out_bytes(H);
}

// What the probe says: the header walk, and for a binary type whether the raster is all there.
ICX_PNM_HD int pnm_check(const uint8_t* f, int64_t n, PnmHead* H) {
    const int rc = pnm_parse(f, n, H);
    if (rc != kPnmOk) return rc;
    if (!H->ascii && H->rs + pnm_raster_bytes(*H) > n) return kPnmTruncated;
    return kPnmOk;
}

// The whole read, one byte at a time: the contract restated (and what a GPU result must equal).
// `out` has room for cap bytes (too little -> kPnmTooLarge); USHORT samples are stored in host order.
ICX_PNM_HD int pnm_decode_serial(const uint8_t* f, int64_t n, PnmHead* H, uint8_t* out, int64_t cap) {
    const int rc = pnm_check(f, n, H);
    if (rc != kPnmOk) return rc;
    if (pnm_out_bytes(*H) > cap) return kPnmTooLarge;
    const int64_t N = (int64_t)H->w * H->h * H->d;
    const uint8_t* r = f + H->rs;
    if (H->kind == '4') {
        const int64_t rb = (H->w + 7) / 8;
        for (int64_t y = 0; y < H->h; ++y)
            for (int64_t x = 0; x < H->w; ++x) out[y * H->w + x] = (r[y * rb + (x >> 3)] >> (7 - (x & 7))) & 1 ? 0 : 255;
        return kPnmOk;
    }
    if (H->kind == '5' || H->kind == '6') {
        if (H->type == kPnmUbyte) {
            for (int64_t k = 0; k < N; ++k) out[k] = r[k];
        } else {
            uint16_t* o = reinterpret_cast<uint16_t*>(out);
            for (int64_t k = 0; k < N; ++k) o[k] = (uint16_t)(r[2 * k] << 8 | r[2 * k + 1]);
        }
        return kPnmOk;
    }
    if (!H->ascii) {  // PF, Pf: the file's rows run bottom-to-top
        const int64_t row = (int64_t)H->w * H->d * 4;
        for (int64_t y = 0; y < H->h; ++y) {
            const uint8_t* s = r + (H->h - 1 - y) * row;
            uint8_t* o = out + y * row;
            for (int64_t b = 0; b < row; ++b) o[b] = s[H->le ? b : b ^ 3];
        }
        return kPnmOk;
    }
    const bool p1 = H->kind == '1';
    int64_t pos = H->rs, cnt = 0;
    bool comment = false;
    while (pos < n && cnt < N) {
        const int c = f[pos];
        if (comment) {
            comment = !pnm_is_eol(c);
            ++pos;
            continue;
        }
        const int cls = pnm_class(c, p1);
        if (cls == kPnmClsBad) return kPnmBadData;
        if (cls != kPnmClsDigit) {
            comment = cls == kPnmClsHash;
            ++pos;
            continue;
        }
        int32_t v = 0;
        if (p1) {
            v = c == '0' ? 255 : 0;
            ++pos;
        } else {
            while (pos < n && pnm_is_digit(f[pos])) {
                v = v * 10 + (f[pos] - '0');
                if (v > 65535) v = 65536;
                ++pos;
            }
            if (v > H->maxval) return kPnmBadData;
        }
        if (H->type == kPnmUshort) reinterpret_cast<uint16_t*>(out)[cnt] = (uint16_t)v;
        else out[cnt] = (uint8_t)v;
        ++cnt;
    }
    return cnt < N ? kPnmTruncated : kPnmOk;
}

// ------------------------------------------------------------------------------------ write
// P4: UBYTE d = 1; P5: UBYTE / USHORT d = 1; P6: UBYTE / USHORT d = 3, 4; PF: FLOAT d = 1 (Pf), 3 (PF).
ICX_PNM_HD bool pnm_write_args_ok(int64_t w, int64_t h, int d, int type, int format) {
    if (w < 1 || h < 1 || w > kPnmMaxPixels || h > kPnmMaxPixels || w * h > kPnmMaxPixels) return false;
    if (format == kPnmP4) return type == kPnmUbyte && d == 1;
    if (format == kPnmP5) return (type == kPnmUbyte || type == kPnmUshort) && d == 1;
    if (format == kPnmP6) return (type == kPnmUbyte || type == kPnmUshort) && (d == 3 || d == 4);
    if (format == kPnmPF) return type == kPnmFloat && (d == 1 || d == 3);
    return false;
}

constexpr int kPnmMaxHeader = 32;  // "P6\n" + 10 + " " + 10 + "\n65535\n" = 31

ICX_PNM_HD int pnm_put_uint(uint8_t* o, int64_t v) {
    uint8_t t[20];
    int k = 0;
    do {
        t[k++] = (uint8_t)('0' + v % 10);
        v /= 10;
    } while (v);
    for (int i = 0; i < k; ++i) o[i] = t[k - 1 - i];
    return k;
}

// The reference's header bytes (codecs.cpp:1112, 1154, 1160) into o[kPnmMaxHeader]; their number.
ICX_PNM_HD int pnm_write_header(uint8_t* o, int w, int h, int d, int type, int format) {
    int k = 0;
    o[k++] = 'P';
    o[k++] = format == kPnmPF ? (d == 3 ? 'F' : 'f') : (uint8_t)('0' + format);
    o[k++] = '\n';
    k += pnm_put_uint(o + k, w);
    o[k++] = ' ';
    k += pnm_put_uint(o + k, h);
    o[k++] = '\n';
    if (format == kPnmPF) {
        const char* s = "-1.0\n";
        for (int i = 0; i < 5; ++i) o[k++] = (uint8_t)s[i];
    } else if (format != kPnmP4) {
        k += pnm_put_uint(o + k, type == kPnmUshort ? 65535 : 255);
        o[k++] = '\n';
    }
    return k;
}

ICX_PNM_HD int64_t pnm_payload_bytes(int w, int h, int d, int type, int format) {
    if (format == kPnmP4) return (int64_t)h * ((w + 7) / 8);
    return (int64_t)w * h * (format == kPnmP6 ? 3 : d) * pnm_elem_bytes(type);
}

// The file's exact length; 0 for arguments the writes refuse.
ICX_PNM_HD uint64_t pnm_encode_bound(int64_t w, int64_t h, int d, int type, int format) {
    if (!pnm_write_args_ok(w, h, d, type, format)) return 0;
    uint8_t hd[kPnmMaxHeader];
    return (uint64_t)pnm_write_header(hd, (int)w, (int)h, d, type, format) + (uint64_t)pnm_payload_bytes((int)w, (int)h, d, type, format);
}

// The whole write, one byte at a time (out has room for pnm_encode_bound bytes); the file's length,
// or 0 for arguments the writes refuse. `px`: w*h*d elements of the type, rows top-down, host order.
ICX_PNM_HD int64_t pnm_encode_serial(const uint8_t* px, int w, int h, int d, int type, int format, uint8_t* out) {
    if (!px || !out || !pnm_write_args_ok(w, h, d, type, format)) return 0;
    int64_t o = pnm_write_header(out, w, h, d, type, format);
    if (format == kPnmP4) {
        for (int64_t y = 0; y < h; ++y)
            for (int64_t x0 = 0; x0 < w; x0 += 8) {
                int b = 0;
                for (int k = 0; k < 8 && x0 + k < w; ++k) b |= (px[y * w + x0 + k] == 0) << (7 - k);
                out[o++] = (uint8_t)b;
            }
        return o;
    }
    if (format == kPnmPF) {  // rows bottom-to-top, little-endian as stored
        const int64_t row = (int64_t)w * d * 4;
        for (int64_t y = h - 1; y >= 0; --y)
            for (int64_t b = 0; b < row; ++b) out[o++] = px[y * row + b];
        return o;
    }
    const int es = pnm_elem_bytes(type), dd = format == kPnmP6 ? 3 : 1;
    for (int64_t p = 0; p < (int64_t)w * h; ++p)
        for (int c = 0; c < dd; ++c) {
            const uint8_t* s = px + (p * d + c) * es;
            if (es == 1) {
                out[o++] = s[0];
            } else {  // big-endian in the file
                out[o++] = s[1];
                out[o++] = s[0];
            }
        }
    return o;
}

}  // namespace icx
