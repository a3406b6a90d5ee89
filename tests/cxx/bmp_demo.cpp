// The reference's ImageCodecs::Image usage for BMP files, against the drop-in header:
//   bmp_demo read <in.bmp> <a.bin>                 read; size, channels, type and pixels to a.bin
//   bmp_demo copy <in.bmp> <out.bmp> <a.bin> <b.bin>
//                                                  read, write, read back; both reads to files
//   bmp_demo load <out.bmp> [d]                    a 21x5 image of d (3) channels adopted with load(),
//                                                  written, read back: prints its size and channels
// read() of a file it cannot decode throws std::runtime_error. Files are written with the public
// extension writeBmp(path), which throws nothing: the line says whether it worked. (write("x.bmp")
// still throws std::invalid_argument; tests/test_cxx_dropin.py and others hold that.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>

#include "imagecodecs/codecs.h"

static void dump(ImageCodecs::Image& img, const char* path) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return;
    const int head[4] = {img.cols(), img.rows(), img.channels(), (int)img.type()};
    std::fwrite(head, sizeof head, 1, f);
    std::fwrite(*img.data(), 1, (size_t)img.totalBytes(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "read" && argc >= 4) {
            ImageCodecs::Image a;
            a.read(argv[2]);
            std::puts("read ok");
            dump(a, argv[3]);
            return 0;
        }
        if (mode == "copy" && argc >= 6) {
            ImageCodecs::Image a, b;
            a.read(argv[2]);
            a.writeBmp(argv[3]);
            std::printf("write %s\n", a.lastWriteOk() ? "ok" : "failed");
            if (!a.lastWriteOk()) return 1;
            b.read(argv[3]);
            dump(a, argv[4]);
            dump(b, argv[5]);
            return 0;
        }
        if (mode == "load") {
            const int d = argc >= 4 ? std::atoi(argv[3]) : 3;
            unsigned char* px = new unsigned char[21 * 5 * d];
            for (int i = 0; i < 21 * 5 * d; ++i) px[i] = (unsigned char)(i * 7);
            ImageCodecs::Image img;
            img.load(px, 21, 5, d);  // (~Image delete[]s it)
            img.writeBmp(argv[2]);
            std::printf("write %s: %s\n", img.lastWriteOk() ? "ok" : "failed", icx_last_error(nullptr));
            if (!img.lastWriteOk()) return 1;
            ImageCodecs::Image back;
            back.read(argv[2]);
            const bool same = back.totalBytes() == img.totalBytes() && !std::memcmp(*back.data(), *img.data(), (size_t)img.totalBytes());
            std::printf("%d %d %d %s\n", back.cols(), back.rows(), back.channels(), same ? "same" : "differs");
            return same ? 0 : 1;
        }
        return 2;
    } catch (const std::invalid_argument& e) {
        std::printf("invalid_argument: %s\n", e.what());
    } catch (const std::runtime_error& e) {
        std::printf("runtime_error: %s\n", e.what());
    }
    return 1;
}
