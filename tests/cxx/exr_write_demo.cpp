// The reference's ImageCodecs::Image usage for an OpenEXR write, against the drop-in header:
//   exr_write_demo load <out.exr>            a 20x5 RGBA float image adopted with load(), written
//   exr_write_demo copy <in.exr> <out.exr> <a.bin> <b.bin>
//                                            read, write, read back; both reads' floats to files
//   exr_write_demo bmp  <in.exr> <out.bmp>   read, then write to an extension outside the path
// write(".exr") throws nothing (as the reference's writeExr): the first line says whether it
// worked and what the library's last error is.
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
        if (mode == "load") {
            float* px = new float[20 * 5 * 4];
            for (int i = 0; i < 20 * 5 * 4; ++i) px[i] = 0.125f * (float)(i % 7);
            ImageCodecs::Image img;
            img.load(reinterpret_cast<unsigned char*>(px), 20, 5, 4);  // (~Image delete[]s it)
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
        if (mode == "bmp" && argc >= 4) {
            ImageCodecs::Image a;
            a.read(argv[2]);
            a.write(argv[3]);
            std::puts("write returned");
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
