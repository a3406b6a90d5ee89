// icx_gif_core.h as a program of its own (tests/test_gif_core.py builds it with g++, and again with
// -fsanitize=address,undefined):
//   gif_core_demo parse <in.gif> ...          the container walk: code and every field, a line per file.
//                                             The file is read into a buffer of exactly its size, so
//                                             a read past the end is a heap overflow the sanitizer sees
//   gif_core_demo codes <mcs> <t0> <count>    "offset width" of codes t0 .. t0 + count - 1
//   gif_core_demo interlace <h>               the frame row of every stream row, then the inverse
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icx_gif_core.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    for (int a = 2; mode == "parse" && a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        uint8_t* buf = (uint8_t*)std::malloc(n ? (size_t)n : 1);  // (exactly n bytes; n = 0: never read)
        if (n && std::fread(buf, 1, (size_t)n, f) != (size_t)n) return 2;
        std::fclose(f);
        icx::GifHead H;
        const int rc = icx::gif_parse(buf, n, &H);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld\n", rc, H.w, H.h, H.has_image, H.fx, H.fy, H.fw, H.fh,
                    H.interlace, H.pal_size, H.bg_index, H.bg_rgb, H.transparent, H.mcs, (long long)H.pal_at,
                    (long long)H.data_at);
        std::free(buf);
    }
    if (mode == "parse") return 0;
    if (mode == "codes" && argc >= 5) {
        const int mcs = std::atoi(argv[2]);
        const uint32_t t0 = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        const int count = std::atoi(argv[4]);
        for (int k = 0; k < count; ++k)
            std::printf("%llu %d\n", (unsigned long long)icx::gif_code_offset(mcs, t0 + k), icx::gif_code_width(mcs, t0 + k));
        return 0;
    }
    if (mode == "interlace") {
        const int h = std::atoi(argv[2]);
        for (int r = 0; r < h; ++r) std::printf("%d ", icx::gif_interlace_row(h, r));
        std::printf("\n");
        for (int y = 0; y < h; ++y) std::printf("%d ", icx::gif_interlace_stream_row(h, y));
        std::printf("\n");
        return 0;
    }
    return 2;
}
