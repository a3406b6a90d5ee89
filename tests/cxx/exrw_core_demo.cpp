// The OpenEXR write's host/device arithmetic (imagecodecs_amd/csrc/icx_exrw_core.h) on the CPU:
//   exrw_core_demo half  IN        IN: uint32 float bit patterns -> one hex half per line
//   exrw_core_demo chunks IN W H C FP16   IN: W*H*C floats -> per chunk "header" (the file header's
//                                  hex, once), then "raw K hex" and "pred K hex" lines
// tests/test_exr_write_core.py builds it with g++ and compares with its numpy restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icx_exrw_core.h"

static std::vector<uint32_t> read_words(const char* path) {
    std::vector<uint32_t> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint32_t x;
    while (std::fread(&x, 4, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "half")) {
        for (uint32_t x : read_words(argv[2])) std::printf("%04x\n", icx::exrw_half(x));
        return 0;
    }
    if (argc >= 7 && !std::strcmp(argv[1], "chunks")) {
        const std::vector<uint32_t> px = read_words(argv[2]);
        const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), c = std::atoi(argv[5]), fp16 = std::atoi(argv[6]);
        if (px.size() != (size_t)w * h * c) return 2;
        const icx::ExrwGeom g = icx::exrw_geom(w, h, c, fp16);
        std::printf("header ");
        for (uint8_t b : icx::exrw_header(g)) std::printf("%02x", b);
        std::printf("\nbound %llu\n", (unsigned long long)icx::exrw_bound(g));
        for (int64_t k = 0; k < icx::exrw_nchunks(g); ++k) {
            const uint32_t S = (uint32_t)icx::exrw_chunk_bytes(g, k);
            const int64_t y0 = k * g.lines;
            std::printf("raw %lld ", (long long)k);
            for (uint32_t i = 0; i < S; ++i) std::printf("%02x", icx::exrw_raw_byte(px.data(), g, y0, i));
            std::printf("\npred %lld ", (long long)k);
            for (uint32_t t = 0; t < S; ++t) std::printf("%02x", icx::exrw_pred_byte(px.data(), g, y0, S, t));
            std::printf("\n");
        }
        return 0;
    }
    return 2;
}
