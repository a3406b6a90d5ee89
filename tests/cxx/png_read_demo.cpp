// The reference's ImageCodecs::Image usage for a PNG read, against the drop-in header:
//   png_read_demo <in.png> <out.bin>   read; write int32 w, h, d, type and the pixel bytes
// A failure prints the exception and exits 1 (no CPU fallback: without a GPU the read throws).
#include <cstdio>
#include <exception>
#include <stdexcept>

#include "imagecodecs/codecs.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        ImageCodecs::Image img;
        img.read(argv[1]);
        std::FILE* f = std::fopen(argv[2], "wb");
        if (!f) return 2;
        const int head[4] = {img.cols(), img.rows(), img.channels(), (int)img.type()};
        std::fwrite(head, sizeof head, 1, f);
        std::fwrite(*img.data(), 1, (size_t)img.totalBytes(), f);
        std::fclose(f);
        std::puts("read ok");
        return 0;
    } catch (const std::invalid_argument& e) {
        std::printf("invalid_argument: %s\n", e.what());
    } catch (const std::runtime_error& e) {
        std::printf("runtime_error: %s\n", e.what());
    }
    return 1;
}
