// TEST-ONLY sanitizer driver: the PNG read's chunk walk (imagecodecs_amd/csrc/icx_pngd_core.h, the
// code icx_png_probe runs on the host and k_pngd_parse / k_pngd_gather run on the device) under
// -fsanitize=address,undefined, host-only build. Every file named on the command line is walked
// as it is and under 500 damages (250 single-byte changes, 250 truncations), each copy in a heap
// block of exactly its size so that a read past the end is reported. A file the walk accepts
// also has its IDAT chain followed the way the gather kernel follows it: every payload byte is
// read and the lengths must add up to what the walk counted. Exit status 0 = no report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../imagecodecs_amd/csrc/icx_pngd_core.h"

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// returns the walk's code; aborts on an inconsistency between the walk and the IDAT chain
static int walk(const uint8_t* src, size_t n, unsigned* sink) {
    uint8_t* d = (uint8_t*)std::malloc(n ? n : 1);  // (exactly n bytes when n > 0)
    if (n) std::memcpy(d, src, n);
    icx::PngdInfo I;
    const int rc = icx::pngd_walk(n ? d : nullptr, (int64_t)n, I);
    if (rc == icx::kPngrOk) {
        int64_t total = 0;
        for (int64_t p = I.first_idat; p >= 0; p = icx::pngd_idat_next(d, (int64_t)n, p)) {
            const int64_t len = (int64_t)icx::pngd_be32(d + p);
            for (int64_t k = 0; k < len; ++k) *sink += d[p + 8 + k];
            total += len;
        }
        if (total != I.idat_bytes || I.w < 1 || I.h < 1 || I.lb < 1 || I.lb % I.bw != 0) {
            std::fprintf(stderr, "walk and IDAT chain disagree: %lld vs %lld\n", (long long)total, (long long)I.idat_bytes);
            std::abort();
        }
    }
    std::free(d);
    return rc;
}

int main(int argc, char** argv) {
    int files = 0, accepted = 0;
    unsigned sink = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        int c;
        while ((c = std::fgetc(f)) != EOF) d.push_back((uint8_t)c);
        std::fclose(f);
        if (walk(d.data(), d.size(), &sink) == icx::kPngrOk) ++accepted;
        for (int k = 0; k < 500 && !d.empty(); ++k) {
            if (k & 1) {
                walk(d.data(), rnd() % d.size(), &sink);  // cut short
            } else {
                std::vector<uint8_t> e = d;
                // (early bytes more often: the signature, IHDR, PLTE and tRNS are at the front)
                const size_t at = (k & 2) ? rnd() % d.size() : rnd() % (d.size() < 128 ? d.size() : 128);
                e[at] ^= (uint8_t)(1u + rnd() % 255u);
                walk(e.data(), e.size(), &sink);
            }
        }
        ++files;
    }
    std::printf("sanitized %d files (%d accepted, %u)\n", files, accepted, sink & 1u);
    return 0;
}
