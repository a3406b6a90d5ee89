/*
 * imagecodecs/codecs.h -- drop-in ImageCodecs::Image (reference codecs.h:16-103) for the JPEG
 * path, implemented over the icx C ABI (include/icx.h, libicx.so, MI355X/gfx950).
 *
 * Same names, argument meaning and ownership as the reference class:
 *   read(path)  -- dispatch on the lower-cased extension (codecs.cpp:53-89); ".jpg"/".jpeg"
 *                  decode on the GPU (readJpg, codecs.cpp:821-849 -> icx_jpeg_decode).
 *               ".hdr" decodes Radiance RGBE to 4 floats per pixel on the GPU (readHdr,
 *               codecs.cpp:706-777 -> icx_hdr_decode; bit-identical floats).
 *               ".png" decodes to 8-bit RGBA, rows top-down, on the GPU (readPng,
 *               codecs.cpp:903-1020 -> icx_png_decode; the PNG specification's sample
 *               conversions where the reference calls libpng).
 *               ".exr" decodes OpenEXR to RGBA floats on the GPU (readExr, codecs.cpp:464-493 ->
 *               icx_exr_decode = tinyexr's LoadEXRFromMemory; scope in include/icx.h).
 *               ".tga" decodes Targa to 8-bit R,G,B(,A) or grey, rows top-down, on the GPU (readTga,
 *               codecs.cpp:1304-1407 -> icx_tga_decode): raw and run-length coded true colour (24 /
 *               32 bits), monochrome (8 bits) and paletted files (8- / 16-bit indices, 24- / 32-bit
 *               entries; type 9 included, which the reference leaves as a TODO). channels() is 3
 *               or 4 for colour and 1 for monochrome. A file the read refuses (codes in
 *               include/icx.h) leaves pixels_ null and read() throws "Could not read image data".
 *               ".bmp" decodes BMP to 8-bit R,G,B(,A) or grey, rows top-down, on the GPU (readBmp,
 *               codecs.cpp:255-320 -> icx_bmp_decode): core, 40-, 52-, 56-, 64-, 108- and 124-byte
 *               headers; raw files of 1, 4, 8, 16, 24 and 32 bits; RLE4 and RLE8 streams; BITFIELDS
 *               and ALPHABITFIELDS masks; bottom-up and top-down rows. channels() is 4 for 16- / 32-bit
 *               files with an alpha mask, 1 for 8-bit files with a grey-identity palette, else 3.
 *               A file the read refuses (codes in include/icx.h) leaves pixels_ null and read()
 *               throws "Could not read image data".
 *               ".gif" decodes the first frame of a GIF onto its logical screen, 8-bit R,G,B, rows
 *               top-down, on the GPU (readGif, codecs.cpp:507-542 -> icx_gif_decode): global and
 *               local palettes, transparency, interlace, frames smaller than or clipped by the
 *               canvas. A file the read refuses (codes in include/icx.h) leaves pixels_ null and
 *               read() throws "Could not read image data".
 *               writeGif(path, segment_pixels, dither) writes one GIF89a frame on the GPU (writeGif,
 *               codecs.cpp:544-594 -> icx_gif_save_to_file; the file is the contract of include/icx.h
 *               "GIF write", not the reference's grey ramp over planar bytes), called by name.
 *               write(".gif") still throws std::invalid_argument.
 *               ".tif"/".tiff" decode the first IFD of a TIFF, 8 bits per sample, rows top-down, on
 *               the GPU (readTiff, codecs.cpp:1439-1484 -> icx_tiff_decode): strips or tiles,
 *               uncompressed, LZW, zlib or PackBits, predictor 2, grey (either polarity), palette,
 *               RGB and RGBA. channels() is 1, 3 or 4. A file the read refuses (codes in
 *               include/icx.h) leaves pixels_ null and read() throws "Could not read image data".
 *               writeTiff(path, compression, predictor, rows_per_strip) writes strips on the GPU
 *               (writeTiff, codecs.cpp:1485-1513 -> icx_tiff_save_to_file; contract in include/icx.h),
 *               called by name. write(".tif") still throws: the dispatch by extension is left to a
 *               follow-up.
 *               ".pbm"/".pgm"/".ppm"/".pnm"/".pfm" decode Netpbm on the GPU (readPbm, codecs.cpp:1034-1100
 *               -> icx_pnm_decode): P1 .. P6, Pf and PF, told apart by the magic, not by the name.
 *               channels() is 1 or 3; type() is UBYTE (bitmaps: 0 -> 255, 1 -> 0; maxval <= 255),
 *               USHORT (maxval 256 .. 65535, host byte order) or FLOAT (PFM: rows turned top-down,
 *               big-endian files byte-swapped, bits otherwise untouched). Samples are not rescaled.
 *               A file the read refuses (codes in include/icx.h) leaves pixels_ null and read()
 *               throws "Could not read image data".
 *               ".dds" decodes DDS on the GPU (readDds -> icx_dds_decode; contract in include/icx.h,
 *               where the reference copies compressed blocks out as if they were pixels): BC1 .. BC5
 *               (DXT1 .. DXT5, ATI1 / ATI2, BC4U / BC5U and their DXGI formats) to 8-bit pixels,
 *               uncompressed files by their masks, float and 16-bit forms as stored. channels() is
 *               1 .. 4 (3 for BC1 and for an X8 form); type() is UBYTE, USHORT or FLOAT; rows are
 *               top-down. Cubemaps, volumes, arrays, BC6H, BC7, signed and half-float forms are
 *               refused; a file the read refuses leaves pixels_ null and read() throws "Could not
 *               read image data".
 *   write(path) -- ".jpg"/".jpeg" encode with tiny_jpeg quality 3 semantics (writeJpg,
 *                  codecs.cpp:851-854 -> icx_tje_encode_to_file, byte-identical stream).
 *               ".png" encodes with png_encoder::saveToFile semantics (writePng,
 *               codecs.cpp:1022-1025 -> icx_png_save_to_file: lodepng's colour type and
 *               filter bytes, GPU deflate).
 *               ".exr" writes pixels_ as w*h*d floats with tinyexr's SaveEXR semantics (writeExr,
 *               codecs.cpp:495-505 -> icx_exr_save_to_file: FLOAT samples, ZIP chunks of 16
 *               lines with a GPU deflate, tinyexr's bytes everywhere else); as in the reference a
 *               failure throws nothing (lastWriteOk() tells).
 *               ".tga" writes the reference's 18 header bytes and the rows top-down, uncompressed
 *               (writeTga, codecs.cpp:1410-1437 -> icx_tga_save_to_file), for d = 1, 3, 4; as in
 *               the reference nothing is thrown (lastWriteOk() tells).
 *               ".bmp" is not dispatched: write("x.bmp") throws std::invalid_argument like any unknown
 *               extension, as it did before the BMP codec was added. The public extension
 *               writeBmp(path) writes the rows bottom-up, padded to 4 bytes (writeBmp,
 *               codecs.cpp:324-375 -> icx_bmp_save_to_file): d = 3 as 24-bit BI_RGB under a 40-byte
 *               header, d = 4 as 32-bit BI_BITFIELDS under a 108-byte V4 header, d = 1 as 8 bits
 *               with a grey palette; nothing is thrown (lastWriteOk() tells). Run-length coded
 *               files are not written.
 *               ".hdr" writes pixels_ as w*h*4 floats R, G, B, E -- what read(".hdr") returns -- as
 *               the reference's header and four RGBE bytes per pixel (writeHdr, codecs.cpp:779-818
 *               -> icx_hdr_save_to_file, rle = 0); writing what was read reproduces every RGBE
 *               byte. d != 4 throws std::runtime_error("HDR data must contain a 4th channel of
 *               exposure values") (:781-784); any other failure throws nothing (lastWriteOk() tells).
 *               ".pbm" writes P4 (UBYTE, d = 1: bit 1 where the byte is 0), ".pgm" P5 (d = 1), ".ppm" P6
 *               (d = 3, or 4 with the fourth sample dropped), ".pnm" P5 for d = 1 and P6 otherwise,
 *               ".pfm" PF (d = 3) or Pf (d = 1), with the reference's header bytes (writePbm,
 *               codecs.cpp:1102-1167 -> icx_pnm_save_to_file). P5 / P6 take UBYTE (maxval 255) and
 *               USHORT (maxval 65535, big-endian). ".pfm" of non-float data throws
 *               std::runtime_error("Cannot write non-float data to .pfm") (:1149-1152); any other
 *               failure -- a d or type the format does not take included -- throws nothing
 *               (lastWriteOk() tells).
 *               ".dds" writes an uncompressed file, rows top-down and unpadded (writeDds ->
 *               icx_dds_save_to_file, ICX_DDS_RAW): d = 3 as 24-bit B,G,R, d = 4 as 32-bit B,G,R,A,
 *               d = 1 as 8-bit luminance, d = 2 as luminance and alpha, each read back with the
 *               same d; UBYTE only; nothing is thrown (lastWriteOk() tells). The public extension
 *               writeDds(path, ICX_DDS_BC) writes DXT1 / DXT5 / BC4U / BC5U by d.
 *   pixels_ is new[]-owned and delete[]-d by ~Image (codecs.h:102); load() adopts a buffer;
 *   load(pixels, w, h, channels, Type) is an extension that also states the element type.
 * Every other extension is outside this path: it throws std::invalid_argument exactly like the
 * reference's unknown-extension branch (codecs.cpp:80-83), so a build that needs those codecs
 * keeps the reference's codecs.cpp for them.
 *
 *   flip() / swapBR() / idx<T>() -- the reference's public pixel utilities (codecs.h:80, 82-88,
 *                  98; bodies codecs.cpp:162-251) on the host buffer: rows reversed; channels 0 and
 *                  2 exchanged; a row-major element read.
 * Deliberate deviations (DESIGN.md "Boundary"): a grayscale JPEG yields channels() == 1 (the
 * reference reports 3 and over-reads the 1-channel buffer, codecs.cpp:840-844); errors throw
 * std::runtime_error (the reference's std::exception(const char*) is MSVC-only, :836). There is
 * no CPU fallback: without a usable GPU, read()/write() of a JPEG throw. The pixel utilities
 * follow the reference's evident intent where its code is broken: idx<T> copies into its result
 * (the reference's memcpy(&T, ...) does not compile, codecs.h:86); flip / swapBR move whole
 * elements of byteSize() bytes (the reference copies one byte per USHORT element and leaves the
 * other uninitialised, codecs.cpp:180-185, and swaps FLOAT bytes at offsets 0 and 2,
 * :213-224); swapBR of an image with fewer than 3 channels is a no-op (the reference reads
 * past the end of the buffer there). For UBYTE images with 3 or 4 channels -- every JPEG --
 * the results equal the reference's byte for byte.
 * Targa read: the header is 18 bytes (the reference subtracts a padded sizeof(Header) of 20 and
 * reads two bytes too few, codecs.cpp:1343); the ID field is *ID length* bytes (the reference
 * skips *descriptor* bytes, :1335-1336); palette index i selects entry i - origin and an index
 * outside the map gives zero bytes (the reference reads outside its buffer, :1177); descriptor
 * bit 5 (top-left origin) is honoured, so the output is always top-down (the reference always
 * flips, :1403, right only for bottom-left files), and bit 4 (right-to-left) is refused;
 * packets may cross row ends, as in the reference; a packet with more pixels than are missing
 * is refused (the reference writes past its buffer); bytes after the image data are ignored.
 * Targa write, by evident intent: the payload is B,G,R(,A) (the reference stores R,G,B, :1429-1434,
 * which every TGA reader, its own included, shows with red and blue exchanged), and d = 1 is
 * written as image type 3 (the reference's type 2 with 8 bits is not a TGA form).
 * BMP read (contract in include/icx.h): the pixels are R,G,B as every other read here gives them
 * (the reference copies the file's B,G,R bytes as they are, and its write stores pixels_ as they
 * are: its own round trip holds, a BMP read and written as .png has red and blue exchanged); rows are padded to a multiple of 4 bytes (the reference
 * skips w % 4 bytes, codecs.cpp:255-320, right only where w % 4 is 0 or 2: its own test.bmp, 499
 * wide, happens to need the 3 it skips); a negative height means top-down rows and gives a positive
 * rows() (the reference returns a negative h); every depth and form beyond 24-bit BITMAPINFOHEADER
 * files is read where the reference reads the bytes as if they were 24-bit. A file that cannot be
 * opened or is no BMP leaves pixels_ null, so read() throws "Could not read image data" (the
 * reference throws "Could not open .bmp file").
 * BMP write: bfSize is the file's size (the reference stores the payload size without the 54
 * header bytes, :324-375); by evident intent d = 4 is a 32-bit BI_BITFIELDS file under a V4 header
 * (the reference writes 4-byte pixels under a 24-bit header) and d = 1 an 8-bit file with a grey
 * palette (the reference writes 1-byte pixels under a 24-bit header). A file that cannot be opened
 * leaves lastWriteOk() false (the reference throws "Could not open .bmp file").
 * Radiance write, by evident intent: the mantissas are floor(v * 2^(136 - E)) clamped to 0..255, the
 * exact inverse of the read (the reference calls invConvertComponent with its arguments swapped,
 * :810, and its out-of-range casts are undefined); NaN, negative values and zero write 0, +inf 255,
 * and E is the fourth float truncated and clamped to 0..255 (contract in include/icx.h). A file
 * that cannot be opened leaves lastWriteOk() false (the reference throws "Cannot open output file.").
 * GIF read (full list in include/icx.h): GIF87a is accepted (the reference demands 89a); a file
 * without a global table is accepted when the frame has a local one (black background), and is
 * refused with neither; a stream that does not begin with a clear code is decoded as if it did
 * (the reference uses an uninitialised length); a code above the next free entry, or a first code
 * after a clear that is not a literal, is refused (the reference reads outside its table); a
 * string running past the frame is cut there (the reference writes past the frame); a frame wider
 * or taller than the canvas is clipped by column and row, stream rows keeping the descriptor's
 * width (the reference re-wraps at the clipped width); the interlace passes of a frame lower than
 * 5 rows are empty where they have no row (the reference's pass sizes put rows outside it); every
 * extension is walked as a sub-block chain, the graphic control values coming from its first
 * sub-block when that has at least 4 bytes; a file that ends inside a header, table, extension or
 * data sub-block the decode still needs is refused (the reference ignores short reads).
 * TIFF read (contract in include/icx.h): a palette file gives channels() == 3, the ColorMap's
 * entries >> 8 as libtiff maps them (the reference would report 1 for its SamplesPerPixel over
 * TIFFReadRGBAImage's packed pixels); a fourth sample passes through as stored, without
 * TIFFReadRGBAImage's premultiply; and the bytes of a pixel are R, G, B, A in this order (the
 * reference's (currPix >> j) & 0xff shifts by j bits where 8 * j was meant, codecs.cpp:1471-1477).
 * Only 8-bit samples are read.
 * Netpbm read (contract in include/icx.h): the type is the magic's (the reference decides by
 * filepath.find(".pbm") / (".pfm"): a P4 file named .pnm comes back as packed bits, and its
 * ".pbm" branch throws for any other magic); maxval decides between UBYTE and USHORT and bounds the
 * ASCII samples (the reference ignores it: it reads half of a 16-bit raster and truncates larger
 * ASCII values to a byte); in a P1 file every '0' / '1' is a sample, as the specification says (the
 * reference reads "0101" as the number 101); a PFM's positive scale means big-endian floats, which
 * are byte-swapped (the reference copies them as they are). Netpbm write, by evident intent: a PFM's
 * rows are written bottom-to-top (the reference writes them unflipped but flips on read, so its own
 * round trip turns the picture over); ".pnm" of a d = 1 image is P5 (the reference writes "P6" over
 * one sample per pixel); USHORT and d = 4 are accepted as described above.
 *
 * DDS (contract in include/icx.h): block-compressed files are decoded (the reference's readDds hands
 * out w*h*d bytes of the compressed blocks); the pixels are R,G,B(,A) by the file's masks (the
 * reference copies stored bytes) and an X8 file has 3 channels (nv_dds says 4); rows are top-down
 * (the reference's two flips cancel). The write stores the pitch of the unpadded rows it writes (the
 * reference stores a dword-aligned one) and d = 1 as luminance (the reference writes it under RGB
 * masks that cannot hold it).
 *
 * Header-only; link with -L<repo>/imagecodecs_amd/lib -licx. One icx context per process
 * (device ICX_DEVICE, default 0), created on first use and serialised by a mutex -- the
 * reference's NanoJPEG state is a process global too (jpeg_dec.h:332).
 */
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../icx.h"

namespace ImageCodecs {

enum class Type { UBYTE, USHORT, FLOAT };

namespace detail {
struct IcxProcess {
    std::mutex mu;
    icx_ctx* ctx = nullptr;
    icx_ctx* get() {  // call with mu held
        if (!ctx) {
            const char* dev = std::getenv("ICX_DEVICE");
            ctx = icx_create(dev ? std::atoi(dev) : 0);
            if (!ctx) throw std::runtime_error(std::string("icx_create failed: ") + icx_last_error(nullptr));
        }
        return ctx;
    }
    ~IcxProcess() {
        if (ctx) icx_destroy(ctx);
    }
};
inline IcxProcess& icx_process() {
    static IcxProcess p;
    return p;
}
inline std::string lower_ext(const std::string& path) {
    std::string e = std::filesystem::path(path).extension().string();
    for (auto& c : e) c = (char)std::tolower((unsigned char)c);
    return e;
}
// The file's bytes; false (and none) when it cannot be opened.
inline bool read_file(const std::string& path, std::vector<uint8_t>& buf) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t k;
    while ((k = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + k);
    std::fclose(f);
    return true;
}
inline bool is_pnm_ext(const std::string& e) {
    return e == ".pbm" || e == ".pgm" || e == ".ppm" || e == ".pnm" || e == ".pfm";
}
}  // namespace detail

class Image {
    int h_ = 0, w_ = 0, d_ = 0;
    unsigned char* pixels_ = nullptr;
    Type type_ = Type::UBYTE;
    bool last_write_ok_ = false;

    int byteSize(Type t) const { return t == Type::FLOAT ? 4 : t == Type::USHORT ? 2 : 1; }

    // The byte readers' body (png, tga, bmp, gif, tiff): decode(ctx, data, size, &out, &w, &h, &d)
    // sets d or leaves the `d` given here. As in the reference a failure -- a file that cannot be
    // opened included -- leaves pixels_ null; only an internal error throws, with the library's message.
    template <class Decode>
    void readBytes(const std::string& path, const char* entry, int ok, int internal, int d, Decode decode) {
        std::vector<uint8_t> buf;
        detail::read_file(path, buf);
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        uint8_t* out = nullptr;
        int w = 0, h = 0;
        const int rc = decode(P.get(), buf.data(), buf.size(), &out, &w, &h, &d);
        delete[] pixels_;
        pixels_ = nullptr;
        w_ = h_ = d_ = 0;
        if (rc == internal) throw std::runtime_error(std::string(entry) + ": " + icx_last_error(P.get()));
        if (rc != ok) return;
        const size_t n = (size_t)w * h * d;
        pixels_ = new unsigned char[n ? n : 1];
        if (n) std::memcpy(pixels_, out, n);
        icx_free(out);
        w_ = w;
        h_ = h;
        d_ = d;
        type_ = Type::UBYTE;
    }

    void readJpg(const std::string& path) {
        std::vector<uint8_t> buf;
        if (!detail::read_file(path, buf)) throw std::runtime_error("Could not open " + path);
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        uint8_t* out = nullptr;
        int w = 0, h = 0, d = 0;
        const int rc = icx_jpeg_decode(P.get(), buf.data(), buf.size(), &out, &w, &h, &d);
        if (rc != ICX_OK) {
            icx_free(out);
            throw std::runtime_error("Error decoding the input file (nj_result_t " + std::to_string(rc) + ").");
        }
        const size_t n = (size_t)w * h * d;
        unsigned char* px = new unsigned char[n ? n : 1];
        if (n) std::memcpy(px, out, n);
        icx_free(out);
        delete[] pixels_;
        pixels_ = px;
        w_ = w;
        h_ = h;
        d_ = d;
        type_ = Type::UBYTE;
    }

    // readHdr (codecs.cpp:706-777): d = 4, Type::FLOAT, R, G, B = v * 2^(E-136) and E per pixel,
    // decoded on the GPU (icx_hdr_decode). A truncated file keeps its decoded rows and zeroes the
    // rest (the reference leaves them uninitialised); header errors and run-length data the
    // reference cannot decode throw "Invalid file format" (:719, :748).
    void readHdr(const std::string& path) {
        std::vector<uint8_t> buf;
        if (!detail::read_file(path, buf)) throw std::runtime_error("Cannot open file");  // codecs.cpp:713-714
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        float* out = nullptr;
        int w = 0, h = 0, rows = 0;
        const int rc = icx_hdr_decode(P.get(), buf.data(), buf.size(), &out, &w, &h, &rows);
        if (rc != ICX_HDR_OK && rc != ICX_HDR_TRUNCATED) {
            icx_free(out);
            if (rc == ICX_HDR_INTERNAL_ERR) throw std::runtime_error(std::string("icx_hdr_decode: ") + icx_last_error(P.get()));
            throw std::runtime_error("Invalid file format");
        }
        const size_t n = (size_t)w * h * 4 * sizeof(float);
        unsigned char* px = new unsigned char[n ? n : 1];
        if (n) std::memcpy(px, out, n);
        icx_free(out);
        delete[] pixels_;
        pixels_ = px;
        w_ = w;
        h_ = h;
        d_ = 4;
        type_ = Type::FLOAT;
    }

    // readExr (codecs.cpp:464-493): LoadEXRFromMemory -> d = 4, Type::FLOAT. The reference's read
    // loop stores one byte more than the file holds (ifile.get()'s EOF as 0xFF, :468-471); it is
    // passed on the same way. A failure throws "Could not load .exr" (:489).
    void readExr(const std::string& path) {
        std::vector<uint8_t> buf;
        detail::read_file(path, buf);
        buf.push_back(0xFF);
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        float* out = nullptr;
        int w = 0, h = 0;
        const int rc = icx_exr_decode(P.get(), buf.data(), buf.size(), &out, &w, &h);
        if (rc != ICX_EXR_SUCCESS) {
            icx_free(out);
            if (rc == ICX_EXR_INTERNAL_ERR) throw std::runtime_error(std::string("icx_exr_decode: ") + icx_last_error(P.get()));
            throw std::runtime_error("Could not load .exr");
        }
        const size_t n = (size_t)w * h * 4 * sizeof(float);
        unsigned char* px = new unsigned char[n ? n : 1];
        if (n) std::memcpy(px, out, n);
        icx_free(out);
        delete[] pixels_;
        pixels_ = px;
        w_ = w;
        h_ = h;
        d_ = 4;
        type_ = Type::FLOAT;
    }

    // readPng (codecs.cpp:903-1020): d = 4, Type::UBYTE, 8-bit RGBA, rows top-down (the reference
    // fills them bottom-up and flips). As in the reference a failure leaves pixels_ null, and
    // read() throws "Could not read image data" (:85-88).
    void readPng(const std::string& path) {
        readBytes(path, "icx_png_decode", ICX_PNGR_OK, ICX_PNGR_INTERNAL_ERR, 4,
                  [](icx_ctx* c, const uint8_t* p, size_t n, uint8_t** out, int* w, int* h, int*) {
                      return icx_png_decode(c, p, n, out, w, h);
                  });
    }

    // readTga (codecs.cpp:1304-1407): d = 1, 3 or 4, Type::UBYTE, rows top-down, decoded on the GPU
    // (icx_tga_decode). As in the reference a failure (type 0 included) leaves pixels_ null, and
    // read() throws "Could not read image data" (:85-88).
    void readTga(const std::string& path) {
        readBytes(path, "icx_tga_decode", ICX_TGA_OK, ICX_TGA_INTERNAL_ERR, 0, icx_tga_decode);
    }

    // readBmp (codecs.cpp:255-320): d = 1, 3 or 4, Type::UBYTE, rows top-down, decoded on the GPU
    // (icx_bmp_decode). A failure -- a file that cannot be opened included -- leaves pixels_ null, and
    // read() throws "Could not read image data" (:85-88).
    void readBmp(const std::string& path) {
        readBytes(path, "icx_bmp_decode", ICX_BMP_OK, ICX_BMP_INTERNAL_ERR, 0, icx_bmp_decode);
    }

    void writeJpg(const std::string& path) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        // as in the reference, the encoder's 0/1 result is not acted on (codecs.cpp:853; e.g.
        // d not in {3,4} leaves no image, jpeg_enc.h:954-956); it stays queryable afterwards
        last_write_ok_ = icx_tje_encode_to_file(P.get(), path.c_str(), w_, h_, d_, pixels_) == 1;
    }

    void writePng(const std::string& path) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        // saveToFile returns nothing (png_encoder.h:7); the result stays queryable
        last_write_ok_ = icx_png_save_to_file(P.get(), path.c_str(), pixels_, w_, h_, d_) == ICX_OK;
    }

    // writeExr (codecs.cpp:495-505): SaveEXR(float*, w, h, d, fp16 = false, path). As in the
    // reference, type_ is not consulted (pixels_ is read as w*h*d floats) and nothing is thrown:
    // a failure -- no usable GPU included -- only prints the message; the result stays queryable.
    void writeExr(const std::string& path) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_exr_save_to_file(c, path.c_str(), reinterpret_cast<const float*>(pixels_), w_, h_, d_, 0);
        last_write_ok_ = rc == ICX_EXR_SUCCESS;
        if (!last_write_ok_) std::fprintf(stderr, "icx_exr_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }

    // readGif (codecs.cpp:507-542): the first frame on the logical screen, d = 3, Type::UBYTE, rows
    // top-down, decoded on the GPU (icx_gif_decode). A failure leaves pixels_ null, and read() throws
    // "Could not read image data" (:85-88).
    void readGif(const std::string& path) {
        readBytes(path, "icx_gif_decode", ICX_GIF_OK, ICX_GIF_INTERNAL_ERR, 3,
                  [](icx_ctx* c, const uint8_t* p, size_t n, uint8_t** out, int* w, int* h, int*) {
                      return icx_gif_decode(c, p, n, out, w, h);
                  });
    }

    // readTiff (codecs.cpp:1439-1484): the first IFD, d = 1, 3 or 4, Type::UBYTE, rows top-down,
    // decoded on the GPU (icx_tiff_decode). A failure leaves pixels_ null, and read() throws "Could
    // not read image data" (:85-88).
    void readTiff(const std::string& path) {
        readBytes(path, "icx_tiff_decode", ICX_TIFF_OK, ICX_TIFF_INTERNAL_ERR, 0, icx_tiff_decode);
    }

    // writeTga (codecs.cpp:1410-1437): uncompressed, d = 1, 3, 4. As in the reference nothing is
    // thrown: a failure -- no usable GPU included -- only prints the message; the result stays
    // queryable.
    void writeTga(const std::string& path) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_tga_save_to_file(c, path.c_str(), pixels_, w_, h_, d_, 0);
        last_write_ok_ = rc == ICX_TGA_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_tga_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }

    // readPbm (codecs.cpp:1034-1100): P1 .. P6, Pf and PF by the file's magic, whatever its name;
    // d = 1 or 3, Type::UBYTE, USHORT or FLOAT, rows top-down, decoded on the GPU (icx_pnm_decode). A
    // failure leaves pixels_ null, and read() throws "Could not read image data" (:85-88).
    void readPnm(const std::string& path) {
        std::vector<uint8_t> buf;
        detail::read_file(path, buf);
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        void* out = nullptr;
        int w = 0, h = 0, d = 0, type = 0, maxval = 0;
        const int rc = icx_pnm_decode(P.get(), buf.data(), buf.size(), &out, &w, &h, &d, &type, &maxval);
        delete[] pixels_;
        pixels_ = nullptr;
        w_ = h_ = d_ = 0;
        if (rc == ICX_PNM_INTERNAL_ERR) throw std::runtime_error(std::string("icx_pnm_decode: ") + icx_last_error(P.get()));
        if (rc != ICX_PNM_OK) return;
        const Type t = type == ICX_PNM_FLOAT ? Type::FLOAT : type == ICX_PNM_USHORT ? Type::USHORT : Type::UBYTE;
        const size_t n = (size_t)w * h * d * byteSize(t);
        pixels_ = new unsigned char[n ? n : 1];
        if (n) std::memcpy(pixels_, out, n);
        icx_free(out);
        w_ = w;
        h_ = h;
        d_ = d;
        type_ = t;
    }

    // readDds (contract in include/icx.h): BC1 .. BC5 decoded, masked and copied uncompressed forms;
    // d = 1 .. 4, Type::UBYTE, USHORT or FLOAT, rows top-down, decoded on the GPU (icx_dds_decode). A
    // failure leaves pixels_ null, and read() throws "Could not read image data".
    void readDds(const std::string& path) {
        std::vector<uint8_t> buf;
        detail::read_file(path, buf);
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        void* out = nullptr;
        int w = 0, h = 0, d = 0, type = 0;
        const int rc = icx_dds_decode(P.get(), buf.data(), buf.size(), &out, &w, &h, &d, &type);
        delete[] pixels_;
        pixels_ = nullptr;
        w_ = h_ = d_ = 0;
        if (rc == ICX_DDS_INTERNAL_ERR) throw std::runtime_error(std::string("icx_dds_decode: ") + icx_last_error(P.get()));
        if (rc != ICX_DDS_OK) return;
        const Type t = type == ICX_PNM_FLOAT ? Type::FLOAT : type == ICX_PNM_USHORT ? Type::USHORT : Type::UBYTE;
        const size_t n = (size_t)w * h * d * byteSize(t);
        pixels_ = new unsigned char[n ? n : 1];
        if (n) std::memcpy(pixels_, out, n);
        icx_free(out);
        w_ = w;
        h_ = h;
        d_ = d;
        type_ = t;
    }

    // writePbm (codecs.cpp:1102-1167): ".pbm" P4, ".pgm" P5, ".ppm" P6, ".pnm" P5 for d = 1 and P6
    // otherwise, ".pfm" PF / Pf. ".pfm" of non-float data throws (:1149-1152); as for the other
    // writers any other failure -- no usable GPU included -- only prints the message; the result
    // stays queryable.
    void writePnm(const std::string& path, const std::string& ext) {
        last_write_ok_ = false;
        if (ext == ".pfm" && type_ != Type::FLOAT) throw std::runtime_error("Cannot write non-float data to .pfm");
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int format = ext == ".pbm" ? ICX_PNM_P4 : ext == ".pgm" ? ICX_PNM_P5 : ext == ".ppm" ? ICX_PNM_P6
                         : ext == ".pfm" ? ICX_PNM_PF : d_ == 1 ? ICX_PNM_P5 : ICX_PNM_P6;
        const int type = type_ == Type::FLOAT ? ICX_PNM_FLOAT : type_ == Type::USHORT ? ICX_PNM_USHORT : ICX_PNM_UBYTE;
        const int rc = icx_pnm_save_to_file(c, path.c_str(), pixels_, w_, h_, d_, type, format);
        last_write_ok_ = rc == ICX_PNM_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_pnm_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }

    // writeHdr (codecs.cpp:779-818): the reference's header and four RGBE bytes per pixel. As in the
    // reference d != 4 throws (:781-784) and type_ is not consulted (pixels_ is read as w*h*4
    // floats). Any other failure -- no usable GPU included -- only prints the message; the result
    // stays queryable.
    void writeHdr(const std::string& path) {
        if (d_ != 4) throw std::runtime_error("HDR data must contain a 4th channel of exposure values");
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_hdr_save_to_file(c, path.c_str(), reinterpret_cast<const float*>(pixels_), w_, h_, 4, 0);
        last_write_ok_ = rc == ICX_HDR_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_hdr_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }

public:
    Image() = default;
    Image(const Image&) = delete;  // the reference's implicit copy double-frees pixels_
    Image& operator=(const Image&) = delete;
    ~Image() { delete[] pixels_; }

    int byteSize() const { return byteSize(type_); }
    int channels() const { return d_; }
    int cols() const { return w_; }
    int rows() const { return h_; }
    unsigned char** data() { return &pixels_; }
    bool empty() const { return h_ == 0 || w_ == 0 || d_ == 0 || pixels_ == nullptr; }
    int totalBytes() const { return w_ * h_ * d_ * byteSize(); }
    Type type() const { return type_; }
    bool lastWriteOk() const { return last_write_ok_; }  // extension: tje's result of the last write()
    // Extension: writeBmp (codecs.cpp:324-375; private in the reference) called by name, d = 1, 3, 4,
    // whatever the path's extension. write() does not dispatch ".bmp" to it: that name still reaches
    // the unknown-extension branch there. Nothing is thrown: a failure -- no usable GPU or a path
    // that cannot be opened included -- only prints the message; lastWriteOk() tells.
    void writeBmp(const std::string& path) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_bmp_save_to_file(c, path.c_str(), pixels_, w_, h_, d_);
        last_write_ok_ = rc == ICX_BMP_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_bmp_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }
    // writeDds (private in the reference) called by name, whatever the path's extension: d = 1 .. 4,
    // Type::UBYTE only. ICX_DDS_RAW is what write(".dds") writes; ICX_DDS_BC is an extension: DXT1,
    // DXT5, BC4U or BC5U by d, from the range-fit encoder of include/icx.h. Nothing is thrown: a
    // failure -- no usable GPU, another element type or a path that cannot be opened included -- only
    // prints the message; lastWriteOk() tells.
    void writeDds(const std::string& path, int format = ICX_DDS_RAW) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        if (type_ != Type::UBYTE) {
            std::fprintf(stderr, "writeDds: only UBYTE images are written\n");
            return;
        }
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_dds_save_to_file(c, path.c_str(), pixels_, w_, h_, d_, format);
        last_write_ok_ = rc == ICX_DDS_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_dds_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }
    // writeTiff (private in the reference, codecs.cpp:1485-1513) called by name, whatever the path's
    // extension: d = 1, 3, 4, Type::UBYTE only. The defaults are the reference's layout: one Deflate
    // strip; more strips (rows_per_strip) give the GPU more to do at once. write() does not dispatch
    // ".tif" to it yet: that name still throws there. Nothing is thrown here: a failure -- no usable
    // GPU, another element type or a path that cannot be opened included -- only prints the
    // message; lastWriteOk() tells.
    void writeTiff(const std::string& path, int compression = ICX_TIFF_COMPRESSION_DEFLATE, int predictor = 1,
                   int rows_per_strip = 0) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        if (type_ != Type::UBYTE) {
            std::fprintf(stderr, "writeTiff: only UBYTE images are written\n");
            return;
        }
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_tiff_save_to_file(c, path.c_str(), pixels_, w_, h_, d_, compression, predictor, rows_per_strip);
        last_write_ok_ = rc == ICX_TIFF_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_tiff_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }
    // writeGif (private in the reference, codecs.cpp:544-594) called by name, whatever the path's
    // extension: d = 1, 3, 4, Type::UBYTE only; the file is the one of include/icx.h "GIF write" (the
    // image's own colours when there are 256 or fewer, else a 6 x 7 x 6 cube, ordered dithering on
    // request). write() does not dispatch ".gif" to it: that name still throws there. Nothing is
    // thrown here: a failure -- no usable GPU, another element type or a path that cannot be opened
    // included -- only prints the message; lastWriteOk() tells.
    void writeGif(const std::string& path, int segment_pixels = 0, bool dither = false) {
        auto& P = detail::icx_process();
        std::lock_guard<std::mutex> lock(P.mu);
        last_write_ok_ = false;
        if (type_ != Type::UBYTE) {
            std::fprintf(stderr, "writeGif: only UBYTE images are written\n");
            return;
        }
        icx_ctx* c = nullptr;
        try {
            c = P.get();
        } catch (const std::runtime_error& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return;
        }
        const int rc = icx_gif_save_to_file(c, path.c_str(), pixels_, w_, h_, d_, segment_pixels, dither ? 1 : 0, ICX_GIF_PALETTE_AUTO);
        last_write_ok_ = rc == ICX_GIF_OK;
        if (!last_write_ok_) std::fprintf(stderr, "icx_gif_save_to_file -> %d %s\n", rc, icx_last_error(c));
    }
    // flip (codecs.h:80, codecs.cpp:162-196): reverse the row order in place.
    void flip() {
        if (empty()) return;
        const size_t row = (size_t)w_ * d_ * byteSize();
        std::vector<unsigned char> tmp(row);
        for (int i = 0, j = h_ - 1; i < j; ++i, --j) {
            unsigned char* a = pixels_ + (size_t)i * row;
            unsigned char* b = pixels_ + (size_t)j * row;
            std::memcpy(tmp.data(), a, row);
            std::memcpy(a, b, row);
            std::memcpy(b, tmp.data(), row);
        }
    }
    // swapBR (codecs.h:98, codecs.cpp:198-251): exchange channels 0 and 2 of every pixel.
    void swapBR() {
        if (empty() || d_ < 3) return;
        const int bs = byteSize();
        const size_t px = (size_t)w_ * h_, step = (size_t)d_ * bs;
        unsigned char t[4];
        for (size_t p = 0; p < px; ++p) {
            unsigned char* q = pixels_ + p * step;
            std::memcpy(t, q, bs);
            std::memmove(q, q + 2 * bs, bs);
            std::memcpy(q + 2 * bs, t, bs);
        }
    }
    // idx (codecs.h:82-88): element (row i, column j, channel k) of a row-major T array.
    template <typename T>
    T idx(int i, int j, int k) const {
        T ret;
        std::memcpy(&ret, pixels_ + ((size_t)i * w_ * d_ + (size_t)j * d_ + (size_t)k) * sizeof(T), sizeof(T));
        return ret;
    }
    void load(unsigned char* pixels, int w, int h, int channels) {
        d_ = channels;
        w_ = w;
        h_ = h;
        pixels_ = pixels;
    }
    // Extension: the same with the element type stated (the reference's load cannot say that a
    // buffer holds USHORT or FLOAT elements, which write(".pgm") / write(".pfm") need to know).
    void load(unsigned char* pixels, int w, int h, int channels, Type type) {
        load(pixels, w, h, channels);
        type_ = type;
    }

    void read(const std::string& filepath) {
        const std::string ext = detail::lower_ext(filepath);
        if (ext == ".jpg" || ext == ".jpeg") readJpg(filepath);
        else if (ext == ".png") readPng(filepath);
        else if (ext == ".hdr") readHdr(filepath);
        else if (ext == ".exr") readExr(filepath);
        else if (ext == ".tga") readTga(filepath);
        else if (ext == ".bmp") readBmp(filepath);
        else if (ext == ".gif") readGif(filepath);
        else if (ext == ".tif" || ext == ".tiff") readTiff(filepath);
        else if (detail::is_pnm_ext(ext)) readPnm(filepath);
        else if (ext == ".dds") readDds(filepath);
        else throw std::invalid_argument("Cannot parse filetype");
        if (pixels_ == nullptr) throw std::runtime_error("Could not read image data");
    }

    void write(const std::string& filepath) {
        const std::string ext = detail::lower_ext(filepath);
        if (ext == ".jpg" || ext == ".jpeg") writeJpg(filepath);
        else if (ext == ".png") writePng(filepath);
        else if (ext == ".exr") writeExr(filepath);
        else if (ext == ".tga") writeTga(filepath);
        else if (ext == ".hdr") writeHdr(filepath);
        else if (detail::is_pnm_ext(ext)) writePnm(filepath, ext);
        else if (ext == ".dds") writeDds(filepath, ICX_DDS_RAW);
        else throw std::invalid_argument("Cannot parse filetype");
    }
};

}  // namespace ImageCodecs
