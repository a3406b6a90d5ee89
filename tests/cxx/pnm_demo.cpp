// The reference's ImageCodecs::Image usage for Netpbm files, against the drop-in header:
//   pnm_demo read <in> <a.bin>                   read; size, channels, type and pixels to a.bin
//   pnm_demo copy <in> <out> <a.bin> <b.bin>     read, write, read back; both reads to files
//   pnm_demo load <out> <channels> <type>        a 20x5 image adopted with load() (type 0 through the
//                                                four-argument form, 1 / 2 through the five-argument one), written
// read() of a file it cannot decode throws std::runtime_error; write() throws only for ".pfm" of
// non-float data, as the reference's writePbm: otherwise the line says whether it worked.
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
            a.write(argv[3]);
            std::printf("write %s\n", a.lastWriteOk() ? "ok" : "failed");
            if (!a.lastWriteOk()) return 1;
            b.read(argv[3]);
            dump(a, argv[4]);
            dump(b, argv[5]);
            return 0;
        }
        if (mode == "load" && argc >= 5) {
            const int channels = std::atoi(argv[3]), type = std::atoi(argv[4]);
            const int es = type == 2 ? 4 : type == 1 ? 2 : 1, n = 20 * 5 * channels * es;
            unsigned char* px = new unsigned char[n];
            for (int i = 0; i < n; ++i) px[i] = (unsigned char)(i * 7);
            ImageCodecs::Image img;  // (~Image delete[]s px)
            if (type == 0) img.load(px, 20, 5, channels);
            else img.load(px, 20, 5, channels, type == 2 ? ImageCodecs::Type::FLOAT : ImageCodecs::Type::USHORT);
            img.write(argv[2]);
            std::printf("write %s: %s\n", img.lastWriteOk() ? "ok" : "failed", icx_last_error(nullptr));
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
