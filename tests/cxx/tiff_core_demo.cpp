// icx_tiff_core.h as a program of its own (tests/test_tiff_core.py builds it with g++, plain and
// with -fsanitize=address,undefined):
//   tiff_core_demo decode <file>...   per file one line "code w h d"; an accepted file's pixels go
//                                     to <file>.px. Each file is read into a buffer of exactly its
//                                     size, the pixels into one of exactly w * h * d bytes.
//   tiff_core_demo codes <t0> <n>     "offset width" of codes t0 .. t0 + n - 1 after a Clear
// The serial decode takes its zlib inflate from the caller; here it is the system's zlib on the raw
// deflate stream, inside the contract's two header checks and Adler-32 (link with -lz).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <zlib.h>

#include "icx_tiff_core.h"

using namespace icx;

static bool inflate_exactly(const uint8_t* src, int64_t n, uint8_t* dst, uint32_t want) {
    if (n < 2 || (src[0] * 256u + src[1]) % 31u != 0 || (src[1] & 32u) || (src[0] & 15u) != 8) return false;
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    uint8_t extra = 0;  // (one byte of room past `want` tells a longer stream)
    z.next_in = const_cast<uint8_t*>(src + 2);
    z.avail_in = (uInt)(n - 2);
    z.next_out = dst;
    z.avail_out = want;
    int rc = inflate(&z, Z_FINISH);
    if (rc != Z_STREAM_END && z.avail_out == 0) {
        z.next_out = &extra;
        z.avail_out = 1;
        rc = inflate(&z, Z_FINISH);
    }
    const bool done = rc == Z_STREAM_END && z.total_out == want && z.avail_in >= 4;
    uint32_t adler = 0;
    if (done) adler = (uint32_t)z.next_in[0] << 24 | (uint32_t)z.next_in[1] << 16 | (uint32_t)z.next_in[2] << 8 | z.next_in[3];
    inflateEnd(&z);
    return done && adler == (uint32_t)adler32(adler32(0L, Z_NULL, 0), dst, want);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "codes" && argc == 4) {
        const uint32_t t0 = (uint32_t)std::strtoul(argv[2], nullptr, 10), n = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        for (uint32_t k = 0; k < n; ++k)
            std::printf("%llu %d\n", (unsigned long long)tiff_code_offset(t0 + k), tiff_code_width(t0 + k));
        return 0;
    }
    if (mode != "decode") return 2;
    for (int a = 2; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 3;
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        uint8_t* buf = (uint8_t*)std::malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && std::fread(buf, 1, (size_t)n, f) != (size_t)n) return 3;
        std::fclose(f);
        TiffHead H{};
        int rc = tiff_parse(buf, n, &H);
        if (rc == kTiffOk) {
            const size_t npx = (size_t)H.w * H.h * H.d;
            uint8_t* px = (uint8_t*)std::malloc(npx);
            uint8_t* scratch = (uint8_t*)std::malloc(tiff_chunk_room(H));
            rc = tiff_decode_serial(buf, n, H, px, scratch, inflate_exactly);
            if (rc == kTiffOk) {
                std::FILE* o = std::fopen((std::string(argv[a]) + ".px").c_str(), "wb");
                if (!o || std::fwrite(px, 1, npx, o) != npx) return 3;
                std::fclose(o);
            }
            std::free(scratch);
            std::free(px);
        }
        if (rc == kTiffOk) std::printf("0 %d %d %d\n", H.w, H.h, H.d);
        else std::printf("%d 0 0 0\n", rc);
        std::free(buf);
    }
    return 0;
}
