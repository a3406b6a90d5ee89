// icx_pnm_core.h as a program of its own (g++ only; tests/test_pnm_core.py also builds it with
// -fsanitize=address,undefined): the serial decode and encode over a list of jobs.
//   pnm_core_demo <jobs.txt>
// One job per line, one line of output per job:
//   decode <in.pnm> <out.bin>                          -> "code w h d type maxval"; the pixels' bytes to out.bin
//   encode <in.bin> <w> <h> <d> <type> <format> <out>  -> "length bound"; the file to out (length 0: refused)
// Buffers are allocated at exactly the size the contract promises, so a sanitized build sees any
// byte read or written outside them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "icx_pnm_core.h"

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void spill(const std::string& path, const uint8_t* p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)n);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream jobs(argv[1]);
    std::string line;
    while (std::getline(jobs, line)) {
        std::istringstream in(line);
        std::string op, src, dst;
        in >> op >> src;
        if (op == "decode") {
            in >> dst;
            // (a copy of exactly the file's size: reads past its end are seen)
            const std::vector<uint8_t> file = slurp(src);
            uint8_t* exact = new uint8_t[file.size() ? file.size() : 1];
            if (!file.empty()) std::memcpy(exact, file.data(), file.size());
            icx::PnmHead H{};
            int rc = icx::pnm_check(exact, (int64_t)file.size(), &H);
            std::vector<uint8_t> out;
            if (rc == icx::kPnmOk) {
                out.resize((size_t)icx::pnm_out_bytes(H));
                rc = icx::pnm_decode_serial(exact, (int64_t)file.size(), &H, out.data(), (int64_t)out.size());
            }
            delete[] exact;
            if (rc != icx::kPnmOk) {
                out.clear();
                std::printf("%d 0 0 0 0 0\n", rc);
            } else {
                std::printf("%d %d %d %d %d %d\n", rc, H.w, H.h, H.d, H.type, H.maxval);
            }
            spill(dst, out.data(), out.size());
        } else if (op == "encode") {
            long long w, h;
            int d, type, format;
            in >> w >> h >> d >> type >> format >> dst;
            const std::vector<uint8_t> px = slurp(src);
            const uint64_t bound = icx::pnm_encode_bound(w, h, d, type, format);
            std::vector<uint8_t> out((size_t)bound);
            const int64_t n = bound ? icx::pnm_encode_serial(px.data(), (int)w, (int)h, d, type, format, out.data()) : 0;
            std::printf("%lld %llu\n", (long long)n, (unsigned long long)bound);
            spill(dst, out.data(), (size_t)n);
        } else {
            return 2;
        }
    }
    return 0;
}
