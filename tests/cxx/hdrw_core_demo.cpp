// icx_hdrw_core.h as a program of its own (g++; no GPU, no libicx.so):
//   hdrw_core_demo encode <jobs.bin> <out.bin>   jobs: records of int32 w, h, d, rle and w*h*d floats;
//                                                out: per record uint64 size, uint64 bound, the file
//   hdrw_core_demo planes <jobs.bin> <out.bin>   jobs: records of int32 w and w bytes (one component
//                                                plane); out: per record int32 n and the n packed bytes
//   hdrw_core_demo bound w h d rle               prints icx_hdr_encode_bound's value and the header length
//   hdrw_core_demo time <jobs.bin> reps          prints the milliseconds of one serial encode of the first
//                                                record and the file's size
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icx_hdrw_core.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t chunk[1 << 16];
    size_t k;
    while ((k = std::fread(chunk, 1, sizeof chunk, f)) > 0) v.insert(v.end(), chunk, chunk + k);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "bound" && argc == 6) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), d = std::atoi(argv[4]), rle = std::atoi(argv[5]);
        std::printf("%llu %d\n", (unsigned long long)icx::hdrw_encode_bound(w, h, d, rle),
                    icx::hdrw_args_ok(w, h, d) ? icx::hdrw_header_len(w, h) : 0);
        return 0;
    }
    if (mode == "time" && argc == 4) {  // the first record of a jobs file, encoded `reps` times on this core
        const std::vector<uint8_t> in = slurp(argv[2]);
        const int reps = std::atoi(argv[3]);
        int32_t a[4];
        if (in.size() < 16 || reps < 1) return 1;
        std::memcpy(a, in.data(), 16);
        const int w = a[0], h = a[1], d = a[2], rle = a[3];
        const uint64_t bound = icx::hdrw_encode_bound(w, h, d, rle);
        const size_t nfl = bound ? (size_t)w * h * d : 0;
        if (bound == 0 || 16 + nfl * 4 > in.size()) return 1;
        std::vector<float> px(nfl);
        std::memcpy(px.data(), in.data() + 16, nfl * 4);
        std::vector<uint8_t> file(bound), tmp((size_t)4 * w);
        uint64_t size = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r) size = icx::hdrw_encode_serial(px.data(), w, h, d, rle, file.data(), tmp.data());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
        std::printf("%.3f %llu\n", ms, (unsigned long long)size);
        return 0;
    }
    if (argc != 4) return 2;
    const std::vector<uint8_t> in = slurp(argv[2]);
    std::FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 1;
    size_t at = 0;
    if (mode == "encode") {
        while (at + 16 <= in.size()) {
            int32_t a[4];
            std::memcpy(a, in.data() + at, 16);
            at += 16;
            const int w = a[0], h = a[1], d = a[2], rle = a[3];
            const uint64_t bound = icx::hdrw_encode_bound(w, h, d, rle);
            const size_t nfl = (size_t)w * h * d;
            if (bound == 0 || at + nfl * 4 > in.size()) return 1;
            std::vector<float> px(nfl);
            std::memcpy(px.data(), in.data() + at, nfl * 4);
            at += nfl * 4;
            std::vector<uint8_t> file(bound), tmp((size_t)4 * w);
            uint8_t head[icx::kHdrwHeadMax];
            if (icx::hdrw_write_header(head, w, h) != icx::hdrw_header_len(w, h)) return 1;
            const uint64_t size = icx::hdrw_encode_serial(px.data(), w, h, d, rle, file.data(), tmp.data());
            if (size > bound) return 1;
            std::fwrite(&size, 8, 1, o);
            std::fwrite(&bound, 8, 1, o);
            std::fwrite(file.data(), 1, size, o);
        }
    } else if (mode == "planes") {
        while (at + 4 <= in.size()) {
            int32_t w;
            std::memcpy(&w, in.data() + at, 4);
            at += 4;
            if (w < 1 || at + (size_t)w > in.size()) return 1;
            std::vector<uint8_t> plane(in.begin() + at, in.begin() + at + w), out((size_t)w + (w + 127) / 128);
            at += (size_t)w;
            const int32_t n = icx::hdrw_pack_plane(plane.data(), w, out.data());
            if ((size_t)n > out.size()) return 1;
            std::fwrite(&n, 4, 1, o);
            std::fwrite(out.data(), 1, (size_t)n, o);
        }
    } else {
        return 2;
    }
    return std::fclose(o) == 0 ? 0 : 1;
}
