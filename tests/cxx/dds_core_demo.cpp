// dds_core_demo.cpp -- imagecodecs_amd/csrc/icx_dds_core.h on the CPU (tests/test_dds_core.py;
// built with g++, and again with -fsanitize=address,undefined).
//   dds_core_demo decode <list.txt> <out.bin>    one file path per line; for each prints
//                                                "code w h d type" and appends its elements to out.bin
//   dds_core_demo write <list.txt>               one "<in.bin> <w> <h> <d> <format> <out.dds>" per line:
//                                                rows of d-byte pixels -> the file (format 0 RAW, 1 BC)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icx_dds_core.h"

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
            DdsHead H{};
            int rc = dds_parse(file, (int64_t)in.size(), &H);
            std::vector<uint8_t> out;
            if (rc == kDdsOk) {
                out.resize((size_t)dds_out_bytes(H));
                rc = dds_decode_serial(file, (int64_t)in.size(), &H, out.data(), (int64_t)out.size());
            }
            std::free(file);
            const bool ok = rc == kDdsOk;
            if (!ok) out.clear();
            std::printf("%d %d %d %d %d\n", rc, ok ? H.w : 0, ok ? H.h : 0, ok ? H.d : 0, ok ? H.type : 0);
            all.insert(all.end(), out.begin(), out.end());
        }
        spill(argv[3], all);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "write")) {
        std::FILE* list = std::fopen(argv[2], "r");
        if (!list) { std::perror(argv[2]); return 2; }
        char in[1024], outp[1024];
        int w, h, d, format;
        while (std::fscanf(list, "%1023s %d %d %d %d %1023s", in, &w, &h, &d, &format, outp) == 6) {
            const std::vector<uint8_t> px = slurp(in);
            if (!dds_write_args_ok(w, h, d, format) || px.size() != (size_t)w * h * d) return 2;
            // (an exact-size copy of the pixels, and a file buffer of exactly the bound)
            uint8_t* src = (uint8_t*)std::malloc(px.size());
            std::memcpy(src, px.data(), px.size());
            std::vector<uint8_t> out((size_t)dds_encode_bound(w, h, d, format));
            dds_encode_serial(src, w, h, d, format, out.data());
            std::free(src);
            spill(outp, out);
        }
        std::fclose(list);
        return 0;
    }
    std::fprintf(stderr, "usage: dds_core_demo decode|write ...\n");
    return 2;
}
