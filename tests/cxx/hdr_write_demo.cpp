// The reference's ImageCodecs::Image usage for writing Radiance files, against the drop-in header:
//   hdr_write_demo load4 <out.hdr>                 a 20x5 image of 4 floats per pixel adopted with load(), written
//   hdr_write_demo load3 <out.hdr>                 the same with 3 floats per pixel: write() throws
//   hdr_write_demo copy <in.hdr> <out.hdr> <a.bin> <b.bin>
//                                                  read, write, read back; both reads to files
// write(".hdr") of an image without a 4th channel throws std::runtime_error (codecs.cpp:781-784);
// any other failure throws nothing: the line says whether it worked.
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
        if (mode == "load4" || mode == "load3") {
            const int d = mode == "load4" ? 4 : 3;
            float v[20 * 5 * 4] = {};
            for (int i = 0; i < 20 * 5 * d; ++i) v[i] = d == 4 && i % 4 == 3 ? 128.0f : (float)(i % 97) / 128.0f;
            unsigned char* px = new unsigned char[sizeof v];
            std::memcpy(px, v, sizeof v);
            ImageCodecs::Image img;
            img.load(px, 20, 5, d);  // (~Image delete[]s it)
            img.write(argv[2]);
            std::printf("write %s: %s\n", img.lastWriteOk() ? "ok" : "failed", icx_last_error(nullptr));
            return img.lastWriteOk() ? 0 : 1;
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
        return 2;
    } catch (const std::invalid_argument& e) {
        std::printf("invalid_argument: %s\n", e.what());
    } catch (const std::runtime_error& e) {
        std::printf("runtime_error: %s\n", e.what());
    }
    return 1;
}
