// The drop-in's GIF write, against include/imagecodecs/codecs.h and libicx.so:
//   gif_write_demo writeGif <px.bin> <w> <h> <d> <out.gif> [<segment_pixels> <dither>]
//       the pixels adopted with load() and written by name, with the defaults or the two arguments;
//       prints "write ok" or "write failed" (lastWriteOk()).
//   gif_write_demo abi <px.bin> <w> <h> <d> <out.gif> <segment_pixels> <dither>
//       the same through icx_gif_save_to_file.
//   gif_write_demo ushort <out.gif>       a USHORT image: writeGif prints a line and writes nothing
//   gif_write_demo write <out.gif>        write(".gif"): still std::invalid_argument
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "imagecodecs/codecs.h"

static unsigned char* pixels(const char* path, size_t n) {
    unsigned char* px = new unsigned char[n];
    std::FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(px, 1, n, f) == n;
    if (f) std::fclose(f);
    if (!ok) std::exit(3);
    return px;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    try {
        if ((mode == "writeGif" && argc >= 7) || (mode == "abi" && argc >= 9)) {
            const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), d = std::atoi(argv[5]);
            unsigned char* px = pixels(argv[2], (size_t)w * h * d);
            if (mode == "abi") {
                icx_ctx* c = icx_create(0);
                if (!c) {
                    std::printf("no context: %s\n", icx_last_error(nullptr));
                    return 1;
                }
                const int rc = icx_gif_save_to_file(c, argv[6], px, w, h, d, std::atoi(argv[7]), std::atoi(argv[8]), ICX_GIF_PALETTE_AUTO);
                icx_destroy(c);
                delete[] px;
                std::printf("abi %d\n", rc);
                return rc == ICX_GIF_OK ? 0 : 1;
            }
            ImageCodecs::Image img;
            img.load(px, w, h, d);  // (~Image delete[]s it)
            if (argc >= 9) img.writeGif(argv[6], std::atoi(argv[7]), std::atoi(argv[8]) != 0);
            else img.writeGif(argv[6]);
            std::puts(img.lastWriteOk() ? "write ok" : "write failed");
            return img.lastWriteOk() ? 0 : 1;
        }
        if (mode == "ushort") {
            unsigned char* px = new unsigned char[4 * 4 * 2]();
            ImageCodecs::Image img;
            img.load(px, 4, 4, 1, ImageCodecs::Type::USHORT);
            img.writeGif(argv[2]);
            std::puts(img.lastWriteOk() ? "write ok" : "write failed");
            return 0;
        }
        if (mode == "write") {
            unsigned char* px = new unsigned char[20 * 5 * 3]();
            ImageCodecs::Image img;
            img.load(px, 20, 5, 3);
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
