// The serial core of the TIFF write (imagecodecs_amd/csrc/icx_tiffw_core.h) as a stand-alone
// program, for tests/test_tiff_write_core.py (built plainly and with -fsanitize=address,undefined):
//   tiffw_core_demo bound <w> <h> <d> <comp> <pred> <rps>             the bound, one line
//   tiffw_core_demo file <w> <h> <d> <comp> <pred> <rps> <px.bin> <out.tif> [<payloads.bin>]
//       the whole file from the pixels: geometry, the strips' payloads (none, PackBits, LZW by the
//       core's serial coders; Deflate from payloads.bin: per strip a little-endian uint32 length
//       and the bytes), then header, arrays and IFD. Prints "invalid" for refused arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../imagecodecs_amd/csrc/icx_tiffw_core.h"

using namespace icx;

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const std::string mode = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), d = std::atoi(argv[4]), comp = std::atoi(argv[5]),
              pred = std::atoi(argv[6]), rps = std::atoi(argv[7]);
    if (mode == "bound") {
        std::printf("%llu\n", (unsigned long long)tiffw_bound(w, h, d, comp, pred, rps));
        return 0;
    }
    if (mode != "file" || argc < 10) return 2;
    TiffwGeom g;
    if (!tiffw_geom(w, h, d, comp, pred, rps, &g)) {
        std::puts("invalid");
        return 0;
    }
    const std::vector<uint8_t> px = slurp(argv[8]);
    if (px.size() != (size_t)w * h * d) return 3;
    std::vector<uint8_t> given;
    if (argc > 10) given = slurp(argv[10]);
    size_t gat = 0;
    std::vector<uint8_t> file(8);
    std::vector<uint32_t> offs, cnts;
    std::vector<uint32_t> dict(kTiffwLzwSlots);
    for (int k = 0; k < g.nstrips; ++k) {
        const int y0 = k * g.rps, rows = tiffw_strip_rows(g, k);
        const uint64_t S = (uint64_t)rows * g.rb;
        std::vector<uint8_t> pay;
        auto in = [&](uint64_t i) { return tiffw_strip_byte(px.data(), g, y0, (uint32_t)i); };
        auto out = [&](uint8_t v) { pay.push_back(v); };
        if (comp == kTiffwNone) {
            for (uint64_t i = 0; i < S; ++i) out((uint8_t)in(i));
        } else if (comp == kTiffwLzw) {
            const uint64_t n = tiffw_lzw_encode(dict.data(), S, in, out);
            if (n != pay.size()) return 4;
        } else if (comp == kTiffwPackBits) {
            for (int r = 0; r < rows; ++r) {
                const uint64_t r0 = (uint64_t)r * g.rb, before = pay.size();
                const uint64_t n = tiffw_packbits_row((uint32_t)g.rb, [&](uint32_t i) { return in(r0 + i); }, out);
                if (n != pay.size() - before) return 4;
            }
        } else {
            if (gat + 4 > given.size()) return 5;
            uint32_t len;
            std::memcpy(&len, given.data() + gat, 4);
            if (gat + 4 + len > given.size()) return 5;
            pay.assign(given.begin() + gat + 4, given.begin() + gat + 4 + len);
            gat += 4 + len;
        }
        if (comp != kTiffwDeflate && pay.size() > tiffw_payload_bound(g, rows)) return 6;  // the proven bounds
        offs.push_back((uint32_t)file.size());
        cnts.push_back((uint32_t)pay.size());
        file.insert(file.end(), pay.begin(), pay.end());
        if (file.size() & 1) file.push_back(0);
    }
    const TiffwLayout L = tiffw_layout(g, file.size());
    file.resize(L.total, 0);
    tiffw_header(file.data(), L);
    if (g.d >= 3)
        for (int c = 0; c < g.d; ++c) tiffw_le(file.data() + L.bps_at + 2 * c, 8, 2);
    if (g.nstrips > 1)
        for (int k = 0; k < g.nstrips; ++k) {
            tiffw_le(file.data() + L.so_at + 4 * k, offs[k], 4);
            tiffw_le(file.data() + L.sc_at + 4 * k, cnts[k], 4);
        }
    uint8_t ifd[kTiffwIfdMax];
    const int n = tiffw_ifd(ifd, g, L, offs[0], cnts[0]);
    if (L.ifd_at + n != L.total) return 7;
    std::memcpy(file.data() + L.ifd_at, ifd, n);
    std::FILE* f = std::fopen(argv[9], "wb");
    if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size()) return 8;
    std::fclose(f);
    std::printf("ok %zu\n", file.size());
    return 0;
}
