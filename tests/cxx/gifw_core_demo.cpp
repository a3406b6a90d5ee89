// The serial core of the GIF write (imagecodecs_amd/csrc/icx_gifw_core.h) as a stand-alone
// program, for tests/test_gif_write_core.py (built plainly and with -fsanitize=address,undefined):
//   gifw_core_demo bound <w> <h> <segment_pixels>                     the bound, one line
//   gifw_core_demo args <w> <h> <d> <segment_pixels> <dither> <mode>  "ok" or "invalid"
//   gifw_core_demo file <w> <h> <d> <segment_pixels> <dither> <mode> <px.bin> <out.gif>
//       the whole file from the pixels by the core's serial writer; prints "ok <size>" and the
//       segments' bit offsets on a second line, or "invalid" for refused arguments. A file longer
//       than the bound is an error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../imagecodecs_amd/csrc/icx_gifw_core.h"

using namespace icx;

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string mode = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    if (mode == "bound") {
        std::printf("%llu\n", (unsigned long long)gifw_bound(w, h, std::atoi(argv[4])));
        return 0;
    }
    if (argc < 8) return 2;
    const int d = std::atoi(argv[4]), seg = std::atoi(argv[5]), dither = std::atoi(argv[6]), pal = std::atoi(argv[7]);
    GifwGeom g;
    if (!gifw_geom(w, h, d, seg, dither, pal, &g)) {
        std::puts("invalid");
        return 0;
    }
    if (mode == "args") {
        std::puts("ok");
        return 0;
    }
    if (mode != "file" || argc < 10) return 2;
    const std::vector<uint8_t> px = slurp(argv[8]);
    if (px.size() != (size_t)w * h * d) return 3;
    std::vector<uint64_t> seg_bits;
    const std::vector<uint8_t> file = gifw_write_serial(px.data(), g, &seg_bits);
    if (file.size() > gifw_bound(w, h, seg)) return 6;  // the proven bound
    std::FILE* f = std::fopen(argv[9], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) return 8;
    std::fclose(f);
    std::printf("ok %zu\n", file.size());
    for (uint64_t b : seg_bits) std::printf("%llu ", (unsigned long long)b);
    std::puts("");
    return 0;
}
