// The reference's ImageCodecs::Image usage for TIFF files, against the drop-in header:
//   tiff_demo read <in.tif> <a.bin>    read; size, channels, type and pixels to a.bin
//   tiff_demo write <out.tif>          a 20x5 RGB image adopted with load(), written
// read() of a file it cannot decode throws std::runtime_error; write(".tif") is outside the
// drop-in and throws std::invalid_argument.
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
        if (mode == "write") {
            unsigned char* px = new unsigned char[20 * 5 * 3];
            for (int i = 0; i < 20 * 5 * 3; ++i) px[i] = (unsigned char)(i * 7);
            ImageCodecs::Image img;
            img.load(px, 20, 5, 3);  // (~Image delete[]s it)
            img.write(argv[2]);
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
