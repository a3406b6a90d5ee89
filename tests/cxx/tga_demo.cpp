// The reference's ImageCodecs::Image usage for Targa files, against the drop-in header:
//   tga_demo read <in.tga> <a.bin>                 read; size, channels, type and pixels to a.bin
//   tga_demo copy <in.tga> <out.tga> <a.bin> <b.bin>
//                                                  read, write, read back; both reads to files
//   tga_demo load <out.tga>                        a 20x5 RGB image adopted with load(), written
// read() of a file it cannot decode throws std::runtime_error; write(".tga") throws nothing (as
// the reference's writeTga): the line says whether it worked.
#include <cstdio>
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
        if (mode == "load") {
            unsigned char* px = new unsigned char[20 * 5 * 3];
            for (int i = 0; i < 20 * 5 * 3; ++i) px[i] = (unsigned char)(i * 7);
            ImageCodecs::Image img;
            img.load(px, 20, 5, 3);  // (~Image delete[]s it)
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
