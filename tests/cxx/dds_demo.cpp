// The reference's ImageCodecs::Image usage for DDS files, against the drop-in header:
//   dds_demo read <in.dds> <a.bin>                 read; size, channels, type and pixels to a.bin
//   dds_demo load <out.dds> <d>                    a 21x5 image of d channels adopted with load(), written
//                                                  with write(), read back: prints its size and channels
//   dds_demo bc <in.bin> <w> <h> <d> <out.dds>     pixels from in.bin adopted with load(), written with
//                                                  the public extension writeDds(path, ICX_DDS_BC)
// read() of a file it cannot decode throws std::runtime_error. The writes throw nothing: the line
// says whether they worked.
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
        if (mode == "load" && argc >= 4) {
            const int d = std::atoi(argv[3]);
            unsigned char* px = new unsigned char[21 * 5 * d];
            for (int i = 0; i < 21 * 5 * d; ++i) px[i] = (unsigned char)(i * 7);
            ImageCodecs::Image img;
            img.load(px, 21, 5, d);  // (~Image delete[]s it)
            img.write(argv[2]);
            std::printf("write %s: %s\n", img.lastWriteOk() ? "ok" : "failed", icx_last_error(nullptr));
            if (!img.lastWriteOk()) return 1;
            ImageCodecs::Image back;
            back.read(argv[2]);
            const bool same = back.totalBytes() == img.totalBytes() && !std::memcmp(*back.data(), *img.data(), (size_t)img.totalBytes());
            std::printf("%d %d %d %s\n", back.cols(), back.rows(), back.channels(), same ? "same" : "differs");
            return same ? 0 : 1;
        }
        if (mode == "bc" && argc >= 7) {
            const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), d = std::atoi(argv[5]);
            const size_t n = (size_t)w * h * d;
            unsigned char* px = new unsigned char[n];
            std::FILE* f = std::fopen(argv[2], "rb");
            if (!f || std::fread(px, 1, n, f) != n) return 2;
            std::fclose(f);
            ImageCodecs::Image img;
            img.load(px, w, h, d);
            img.writeDds(argv[6], ICX_DDS_BC);
            std::printf("write %s\n", img.lastWriteOk() ? "ok" : "failed");
            return img.lastWriteOk() ? 0 : 1;
        }
        return 2;
    } catch (const std::invalid_argument& e) {
        std::printf("invalid_argument: %s\n", e.what());
    } catch (const std::runtime_error& e) {
        std::printf("runtime_error: %s\n", e.what());
    }
    return 1;
}
