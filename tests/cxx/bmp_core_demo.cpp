// bmp_core_demo.cpp -- imagecodecs_amd/csrc/icx_bmp_core.h on the CPU (tests/test_bmp_core.py;
// built with g++, and again with -fsanitize=address,undefined).
//   bmp_core_demo decode <list.txt> <out.bin>    one file path per line; for each prints
//                                                "code w h d" and appends its pixels to out.bin
//   bmp_core_demo write <in.bin> <w> <h> <d> <out.bmp>   rows of R,G,B(,A) or grey pixels -> the file
//   bmp_core_demo moves                          checks that composing cursor transforms is associative
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icx_bmp_core.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    uint8_t chunk[1 << 14];
    size_t k;
    while ((k = std::fread(chunk, 1, sizeof chunk, f)) > 0) v.insert(v.end(), chunk, chunk + k);
    std::fclose(f);
    return v;
}

static void spill(const char* path, const std::vector<uint8_t>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f || (!v.empty() && std::fwrite(v.data(), 1, v.size(), f) != v.size()) || std::fclose(f) != 0) { std::perror(path); std::exit(2); }
}

int main(int argc, char** argv) {
    using namespace icx;
    if (argc == 4 && !std::strcmp(argv[1], "decode")) {
        const std::vector<uint8_t> list = slurp(argv[2]);
        std::vector<uint8_t> all;
        size_t a = 0;
        while (a < list.size()) {
            size_t b = a;
            while (b < list.size() && list[b] != '\n') ++b;
            const std::string path(list.begin() + a, list.begin() + b);
            a = b + 1;
            if (path.empty()) continue;
            // (an exact-size copy, so that the sanitizer sees a read past the file's last byte)
            const std::vector<uint8_t> in = slurp(path.c_str());
            uint8_t* file = (uint8_t*)std::malloc(in.size() ? in.size() : 1);
            if (!in.empty()) std::memcpy(file, in.data(), in.size());
            BmpHead H{};
            int rc = bmp_parse(file, (int64_t)in.size(), &H);
            std::vector<uint8_t> out;
            if (rc == kBmpOk) {
                out.resize((size_t)H.w * H.h * H.d);
                rc = bmp_decode_serial(file, (int64_t)in.size(), &H, out.data(), (int64_t)out.size());
            }
            std::free(file);
            if (rc != kBmpOk) out.clear();
            std::printf("%d %d %d %d\n", rc, rc == kBmpOk ? H.w : 0, rc == kBmpOk ? H.h : 0, rc == kBmpOk ? H.d : 0);
            all.insert(all.end(), out.begin(), out.end());
        }
        spill(argv[3], all);
        return 0;
    }
    if (argc == 7 && !std::strcmp(argv[1], "write")) {
        const std::vector<uint8_t> px = slurp(argv[2]);
        const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), d = std::atoi(argv[5]);
        if (!bmp_write_args_ok(w, h, d) || px.size() != (size_t)w * h * d) return 2;
        std::vector<uint8_t> out((size_t)bmp_encode_bound(w, h, d));
        bmp_write_header(out.data(), w, h, d);
        for (int r = 0; r < h; ++r)
            bmp_write_row(px.data() + (size_t)(h - 1 - r) * w * d, w, d, out.data() + bmp_write_offbits(d) + bmp_write_stride(w, d) * r);
        spill(argv[6], out);
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "moves")) {
        // (a o b) o c == a o (b o c), and applying the composition == applying one after the other,
        // clamping included
        const BmpMove m[] = {{0, 0, 0}, {0, 255, 0}, {1, 0, 1}, {0, 3, 255}, {1, 7, 2}, {0, kBmpFar, 0}, {0, kBmpFar - 1, kBmpFar - 3}, {1, kBmpFar, kBmpFar}};
        const int k = (int)(sizeof m / sizeof m[0]);
        int bad = 0;
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b)
                for (int c = 0; c < k; ++c) {
                    const BmpMove l = bmp_compose(bmp_compose(m[a], m[b]), m[c]), r = bmp_compose(m[a], bmp_compose(m[b], m[c]));
                    bad += l.reset != r.reset || l.dx != r.dx || l.dy != r.dy;
                    int32_t x1 = 5, y1 = 6, x2 = 5, y2 = 6;
                    bmp_apply(m[a], &x1, &y1);
                    bmp_apply(m[b], &x1, &y1);
                    bmp_apply(m[c], &x1, &y1);
                    bmp_apply(l, &x2, &y2);
                    bad += x1 != x2 || y1 != y2;
                }
        std::printf("%d\n", bad);
        return bad != 0;
    }
    std::fprintf(stderr, "usage: bmp_core_demo decode|write|moves ...\n");
    return 2;
}
