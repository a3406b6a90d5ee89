/*
 * icx.h -- C ABI of libicx.so, the MI355X-native JPEG codec behind ImageCodecs' codecs.h.
 *
 * Plain pointers and sizes only (no torch / HIP types in signatures). Every function is
 * extern "C", never throws, and is reentrant per icx_ctx. Each entry point names the
 * reference interface it replaces (paths relative to the jstrom2002/ImageCodecs tree):
 *
 *   NanoJPEG (jpeg_dec.h:117-171): njInit/njDecode/njGetWidth/njGetHeight/njIsColor/
 *       njGetImage/njGetImageSize/njDone  -> icx_nj_* below, with the decoder state held
 *       in an icx_ctx instead of NanoJPEG's process-global `nj` (jpeg_dec.h:332).
 *   tiny_jpeg (jpeg_enc.h:114-160): tje_encode_to_file/_at_quality/tje_encode_with_func
 *       -> icx_tje_* below (same quality 1..3 contract and byte stream).
 *   Image::readJpg (codecs.cpp:821-849) -> icx_jpeg_decode (one call, host in/host out).
 *   Batch decode (new) -> icx_jpeg_batch_* (device-resident in and out).
 *
 * Result codes are NanoJPEG's nj_result_t values (jpeg_dec.h:117-125).
 */
#ifndef ICX_H
#define ICX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum icx_result {
    ICX_OK = 0,              /* NJ_OK            */
    ICX_NO_JPEG = 1,         /* NJ_NO_JPEG       */
    ICX_UNSUPPORTED = 2,     /* NJ_UNSUPPORTED   */
    ICX_OUT_OF_MEM = 3,      /* NJ_OUT_OF_MEM    */
    ICX_INTERNAL_ERR = 4,    /* NJ_INTERNAL_ERR  */
    ICX_SYNTAX_ERROR = 5     /* NJ_SYNTAX_ERROR  */
};

typedef struct icx_ctx icx_ctx;

/* ---- context ------------------------------------------------------------------- */
/* One context per (device, HIP stream). `device` is a HIP device ordinal. Returns NULL
 * if the device cannot be opened (see icx_last_error(NULL)). */
icx_ctx* icx_create(int device);
void icx_destroy(icx_ctx* ctx);
/* Last error message for this context (or the last icx_create failure when ctx==NULL). */
const char* icx_last_error(const icx_ctx* ctx);
/* Library version string, e.g. "icx 0.1.0 gfx950". */
const char* icx_version(void);

/* ---- header probe (host only; no device work) ------------------------------------ */
/* Parses markers up to the first SOS exactly as njDecode does (jpeg_dec.h:880-903).
 * Returns ICX_OK when the stream is well-formed up to the entropy-coded data (decode may
 * still fail later) and fills width/height/ncomp (ncomp: 1 gray, 3 colour); otherwise the
 * code njDecode would return. */
int icx_jpeg_probe(const uint8_t* jpeg, size_t size, int* width, int* height, int* ncomp);

/* ---- NanoJPEG-compatible stateful API (jpeg_dec.h:130-171) ------------------------- */
/* njInit (jpeg_dec.h:130) / njDone (:171): reset the context's decoder state. */
void icx_nj_init(icx_ctx* ctx);
void icx_nj_done(icx_ctx* ctx);
/* njDecode (jpeg_dec.h:138): decodes on the GPU; returns an icx_result. */
int icx_nj_decode(icx_ctx* ctx, const void* jpeg, int size);
int icx_nj_get_width(const icx_ctx* ctx);         /* njGetWidth     (:142) */
int icx_nj_get_height(const icx_ctx* ctx);        /* njGetHeight    (:146) */
int icx_nj_is_color(const icx_ctx* ctx);          /* njIsColor      (:151) */
unsigned char* icx_nj_get_image(icx_ctx* ctx);    /* njGetImage     (:160) host memory owned by ctx */
int icx_nj_get_image_size(const icx_ctx* ctx);    /* njGetImageSize (:165) */

/* ---- one-shot decode (Image::readJpg, codecs.cpp:821-849) ------------------------- */
/* Decodes on the GPU; *out receives a malloc()'d W*H*ncomp buffer (free with icx_free).
 * ncomp is 3 for colour and 1 for gray (the reference adapter's d=3-for-gray over-read,
 * codecs.cpp:840-844, is not reproduced). */
int icx_jpeg_decode(icx_ctx* ctx, const uint8_t* jpeg, size_t size, uint8_t** out, int* width,
                    int* height, int* ncomp);
void icx_free(void* p);

/* ---- batch decode, device-resident (the throughput path) ------------------------- */
typedef struct icx_batch icx_batch;

/* Workspace for up to `max_images` images per call, each at most max_width x max_height
 * (any sampling NanoJPEG accepts). At most `group` images (0 = auto: 80% of free HBM) are in
 * flight at once, split over up to two decode pipelines (a workspace and a HIP stream each;
 * env ICX_PIPES=1 keeps one): consecutive groups alternate between the pipelines so their
 * kernels overlap, and the call's stream waits for both. Returns NULL on allocation failure. */
icx_batch* icx_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height, int group);
void icx_batch_destroy(icx_batch* b);

/* Decode n images. All pointers are DEVICE pointers on the context's device:
 *   d_data      concatenated JPEG files; image i is d_data[d_offsets[i] .. + d_sizes[i])
 *   d_out       output; image i is written at d_out + i*out_stride, packed W*H*ncomp bytes
 *   d_status    n int32 icx_result codes (per image; one bad image never fails the batch)
 *   d_dims      n*3 int32 {width, height, ncomp} (ncomp 3 colour / 1 gray; 0s on error)
 * An image larger than the batch limits, or whose pixels exceed out_stride, gets
 * ICX_OUT_OF_MEM. Work is enqueued on `stream` (a hipStream_t; NULL = the context's
 * stream). The call does not wait for the decode, but when the stream is not capturing it does
 * wait on the host for each group's entropy planning, and so for all work enqueued on `stream`
 * before the call (it reads how many images a group's planning deferred to a further entropy
 * round, and enqueues that round only when there are any): do not make `stream` wait on an
 * event the caller records only after this call. Under stream capture (hipStreamBeginCapture,
 * e.g. to build a hipGraph of the decode) the call never waits: every entropy round and every
 * layout's back half is enqueued unconditionally (rounds with nothing to do find no work), so the
 * captured graph is complete; ICX_HOST_WAIT=0 selects that form without capture. Returns ICX_OK
 * or a call-level error. */
int icx_jpeg_batch_decode(icx_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                          const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride,
                          int32_t* d_status, int32_t* d_dims, void* stream);

/* Host-buffer convenience: copies inputs to the device, decodes, copies results back.
 * outs[i] must hold out_stride bytes. */
int icx_jpeg_batch_decode_host(icx_batch* b, int n, const uint8_t* const* jpegs, const size_t* sizes,
                               uint8_t* const* outs, uint64_t out_stride, int32_t* status, int32_t* dims);

/* Images per workspace group (each kernel of the pipeline launches once per group). */
int icx_batch_group(const icx_batch* b); /* images per group (one pipeline's workspace) */
int icx_batch_groups(const icx_batch* b, int n); /* groups (launches of each per-group kernel) a call of n images takes */

/* Per-stage timings (ms) of the most recent batch call, measured with HIP events on the
 * stream the kernels ran on. Fills up to `cap` entries; returns the number of stages. */
int icx_batch_stage_times(const icx_batch* b, const char** names, float* ms, int cap);

/* Which entropy path the images of the most recent batch call took: the parallel
 * self-synchronising decoder, the parallel decoder falling back to the sequential one
 * (unverified chain), or the sequential decoder only (restart intervals, exotic sampling).
 * Synchronizes with the device. */
int icx_batch_path_stats(const icx_batch* b, int32_t* parallel, int32_t* fallback, int32_t* sequential);
/* Of the `parallel` images of the most recent batch call, the restart-interval images planned onto
 * the interval-aligned guess-write lanes: those the lanes decided (gw), and those sent back to one
 * lane per interval because the lanes could not decide them exactly (gw_fallback).
 * Synchronizes with the device. */
int icx_batch_dri_stats(const icx_batch* b, int32_t* gw, int32_t* gw_fallback);

/* ---- per-image result records and multi-GPU decode ------------- */
/* The record each device computes for every image it decoded; ranks (or devices) exchange
 * these 24 bytes per image instead of pixels. checksum = sum of the decoded bytes' little-
 * endian 32-bit words w_k (last one zero-padded) times (2k + 1), mod 2^64 (icx_checksum64). */
typedef struct icx_record {
    int32_t status, width, height, ncomp; /* icx_result; dims as d_dims (0s on error) */
    uint64_t checksum;                    /* 0 for a failed image */
} icx_record;

/* Records of a batch call's outputs (device pointers, enqueued on `stream`, NULL = the
 * context's stream): d_status / d_dims / d_out as icx_jpeg_batch_decode wrote them. */
int icx_jpeg_records(icx_ctx* ctx, int n, const uint8_t* d_out, uint64_t out_stride, const int32_t* d_status,
                     const int32_t* d_dims, int max_width, int max_height, icx_record* d_records, void* stream);
/* The same checksum on the host (a reference for tests and callers). */
uint64_t icx_checksum64(const uint8_t* data, size_t size);
int icx_ctx_device(const icx_ctx* ctx);   /* the context's HIP device ordinal */
void* icx_ctx_stream(const icx_ctx* ctx); /* the context's hipStream_t */

/* Multi-GPU batch decode in one process: the batch is split over `ndev` devices by
 * compressed size (greedy longest-first, icx_multi_shard), one host thread per device decodes
 * its shard with its own context, workspace and stream, and computes its per-image records on
 * the device. The records are gathered over RCCL (one communicator per device, ncclCommInitAll;
 * one grouped ncclAllGather of every shard's records padded to the largest shard) when the
 * devices are distinct and librccl.so loads, else through host memory (ICX_MULTI_RCCL=0 forces
 * that); each device copies its images' pixels to the caller's host buffers. Every image of
 * every device may be up to max_width x max_height. */
typedef struct icx_multi icx_multi;
icx_multi* icx_multi_create(const int* devices, int ndev, int max_width, int max_height);
void icx_multi_destroy(icx_multi* m);
/* outs[i] (may be NULL, or outs itself NULL: records only) receives image i's packed pixels,
 * at most out_stride bytes; records[i] its record; shard_of[i] (optional) the index into
 * `devices` that decoded it. Returns ICX_OK or the first device's call-level error. */
int icx_multi_decode_host(icx_multi* m, int n, const uint8_t* const* jpegs, const size_t* sizes,
                          uint8_t* const* outs, uint64_t out_stride, icx_record* records, int32_t* shard_of);
const char* icx_multi_last_error(const icx_multi* m);
/* How the records are gathered: "rccl", or "host (<reason>)". */
const char* icx_multi_gather(const icx_multi* m);
/* The split: shard_of[i] in [0, ndev) for n images of the given compressed sizes. */
int icx_multi_shard(const size_t* sizes, int n, int ndev, int32_t* shard_of);

/* ---- encode (tiny_jpeg, jpeg_enc.h:114-160) --------------------------------------- */
typedef void icx_write_func(void* context, void* data, int size); /* = tje_write_func */

/* tje_encode_with_func (jpeg_enc.h:154): quality 1..3, comps 3 (RGB) or 4 (RGBA);
 * returns 1 on success, 0 on error. The byte stream is identical to tiny_jpeg's. */
int icx_tje_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, int quality,
                             int width, int height, int num_components, const unsigned char* src);
/* tje_encode_to_file_at_quality (jpeg_enc.h:137) / tje_encode_to_file (:114, quality 3). */
int icx_tje_encode_to_file_at_quality(icx_ctx* ctx, const char* dest_path, int quality, int width,
                                      int height, int num_components, const unsigned char* src);
int icx_tje_encode_to_file(icx_ctx* ctx, const char* dest_path, int width, int height,
                           int num_components, const unsigned char* src);

/* ---- encode extension (IJG quality 1..100, 4:4:4 or 4:2:0) ----------
 * tiny_jpeg only offers quality 1..3 at 4:4:4 (jpeg_enc.h:1223-1256). The extension keeps its
 * entropy coder and float AAN DCT (jpeg_enc.h:980-1100) and adds IJG-scaled tables (luma =
 * tiny_jpeg's, chroma = JPEG spec K.2) and 2x2-mean 4:2:0 chroma. The byte stream is defined by
 * oracle/tje_oracle.c or_jpeg_encode and decodes with NanoJPEG. */
/* Host image -> file bytes through `func`; returns 1 on success, 0 on error. */
int icx_jpeg_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, int quality,
                              int subsampling, int width, int height, int num_components,
                              const unsigned char* src);

typedef struct icx_encoder icx_encoder;
/* Reusable device workspace for device-resident encodes on ctx's device. */
icx_encoder* icx_encoder_create(icx_ctx* ctx);
void icx_encoder_destroy(icx_encoder* enc);
/* Device image d_src (width*height*num_components bytes) -> whole JPEG file at d_out.
 * Synchronous on `hip_stream` (NULL = the context's stream). *out_size receives the file size.
 * Returns ICX_OK, ICX_OUT_OF_MEM when out_cap < *out_size (nothing written),
 * ICX_UNSUPPORTED for bad arguments, ICX_INTERNAL_ERR on a HIP failure. */
int icx_jpeg_encode_device(icx_encoder* enc, int quality, int subsampling, int width, int height,
                           int num_components, const uint8_t* d_src, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* out_size, void* hip_stream);
/* A batch of n device images of one geometry and setting (d_srcs: host array of device
 * pointers) -> JPEG files at d_out + i*out_stride; out_sizes[i] and status[i] (ICX_OK, or
 * ICX_OUT_OF_MEM when out_stride < out_sizes[i]: nothing written) on the host. Images alternate
 * between two workspaces on two streams (hip_stream and an internal one), so each image's host
 * wait overlaps the next image's kernels. Synchronous; returns ICX_OK, ICX_UNSUPPORTED or
 * ICX_INTERNAL_ERR. Replaces a loop of icx_jpeg_encode_device calls (same bytes). */
int icx_jpeg_encode_device_batch(icx_encoder* enc, int n, int quality, int subsampling, int width, int height,
                                 int num_components, const uint8_t* const* d_srcs, uint8_t* d_out,
                                 uint64_t out_stride, uint64_t* out_sizes, int32_t* status, void* hip_stream);
/* Per-stage GPU time (HIP events) of the encodes since the previous call, summed: units
 * (DCT+quantise), count, scan, emit, stuff. Returns the number of stages filled (<= cap). */
int icx_encoder_stage_times(icx_encoder* enc, const char** names, float* ms, int cap);

/* ---- PNG encode (png_encoder::saveToFile, png_encoder.h:7 / png_encoder.cpp:4474-4486) ------
 * d = 3 (RGB8) or 4 (RGBA8) like saveToFile. lodepng's automatic colour type (palette / grey /
 * grey+alpha / RGB / RGBA, tRNS key) and its MINSUM filter bytes are reproduced exactly; the IDAT
 * is our GPU deflate (valid zlib, inflates to lodepng's filtered stream; bytes differ). */
/* Host image -> PNG bytes through `func` (<= 1023-byte chunks); returns 1 on success, 0 on error. */
int icx_png_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, const unsigned char* pixels,
                             int width, int height, int d);
/* png_encoder::saveToFile: returns ICX_OK or an error code (the reference returns nothing). */
int icx_png_save_to_file(icx_ctx* ctx, const char* path, const unsigned char* pixels, int width, int height,
                         int d);

typedef struct icx_png_encoder icx_png_encoder;
icx_png_encoder* icx_png_encoder_create(icx_ctx* ctx);
void icx_png_encoder_destroy(icx_png_encoder* enc);
/* Device image d_src (width*height*d bytes) -> whole PNG file at d_out; synchronous on
 * hip_stream (NULL = the context's stream). Returns ICX_OK, ICX_OUT_OF_MEM when out_cap <
 * *out_size (nothing written), ICX_UNSUPPORTED for bad arguments, ICX_INTERNAL_ERR on a HIP
 * failure. */
int icx_png_encode_device(icx_png_encoder* enc, int width, int height, int d, const uint8_t* d_src,
                          uint8_t* d_out, uint64_t out_cap, uint64_t* out_size, void* hip_stream);
/* n images (width x height x d each, at d_srcs[i] on the context's device) into d_out + i *
 * out_stride; out_sizes[i] = file size (or the bytes needed), status[i] = ICX_OK, ICX_OUT_OF_MEM
 * (the slot is too small) or ICX_INTERNAL_ERR (that image's own job failed: every other image still
 * gets its status and size). Returns ICX_INTERNAL_ERR only when a stream failed. The batch form
 * of png_encoder::saveToFile for device-resident images: several images in flight
 * (ICX_PNG_INFLIGHT, default 8), each on its own workspace and stream. The host reads back one
 * thing per image, its colour statistics (the colour mode and palette are chosen on the host);
 * the file layout, IDAT length, Adler-32, CRC-32 and IEND are computed and written on the device,
 * and every image's size is read once, after the last image. Returns when every file is
 * written. */
int icx_png_encode_device_batch(icx_png_encoder* enc, int n, int width, int height, int d,
                                const uint8_t* const* d_srcs, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* out_sizes, int32_t* status, void* hip_stream);
/* Milliseconds per stage summed over the icx_png_encode_device calls since the previous read
 * ("stats", "filter", "lz77", "huff", "emit", "crc"; HIP events on the launch stream). Returns
 * the number of stages. */
int icx_png_encoder_stage_times(icx_png_encoder* enc, const char** names, float* ms, int cap);

/* ---- PNG read (Image::readPng, codecs.cpp:903-1020) --------------------------------------------
 * Output as readPng returns it (d = 4, Type::UBYTE): 8-bit RGBA, rows top-down. The reference
 * decodes through libpng; here the sample conversions are the PNG specification's (unpinned
 * parity): 16-bit samples keep their high byte, grey of 1 / 2 / 4 bits is scaled by
 * 255 / (2^depth - 1), a palette index takes PLTE's colour and tRNS's alpha (255 without one;
 * (0, 0, 0, 255) past the end of PLTE), grey is replicated to R, G, B, and alpha is the file's
 * (colour types 4 and 6), 0 where a tRNS key equals the samples at file precision (colour types
 * 0 and 2), else 255. Non-interlaced files of every colour type and bit depth. The CRCs of IHDR,
 * PLTE and tRNS are verified; an IDAT CRC is not (the zlib stream's Adler-32 is). A zlib stream
 * that inflates to anything but height * (1 + row bytes) is BAD_DATA (libpng only warns about
 * excess data). */
enum icx_png_read_result {
    ICX_PNGR_OK = 0,
    ICX_PNGR_NOT_PNG = 1,       /* no PNG signature                                              */
    ICX_PNGR_BAD_HEADER = 2,    /* IHDR missing, damaged (CRC) or with illegal values            */
    ICX_PNGR_UNSUPPORTED = 3,   /* interlaced, or an unknown critical chunk                      */
    ICX_PNGR_MALFORMED = 4,     /* a chunk runs past the file; bad PLTE / tRNS; no PLTE; no IDAT */
    ICX_PNGR_BAD_DATA = 5,      /* the zlib stream or a filter byte                              */
    ICX_PNGR_TOO_LARGE = 6,     /* above the reference's 0x1000000 pixel limit, or the batch's   */
    ICX_PNGR_INTERNAL_ERR = -1  /* HIP failure (see icx_last_error)                              */
};
/* Chunk walk only (host): width/height of a file the decoder would start on, else the code. */
int icx_png_probe(const uint8_t* data, size_t size, int* width, int* height);
/* One image, host in / host out: *out receives a malloc()'d width*height*4 byte buffer (free with
 * icx_free). A code the probe gives is returned without touching the GPU. */
int icx_png_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* width, int* height);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), RGBA8 at d_out +
 * i*out_stride bytes (d_out and out_stride multiples of 4; out_stride >= 4*max_width*max_height),
 * per-image status in d_status[i] and {width, height, 4} in d_dims[3i..] (zeros unless OK). An
 * image wider or taller than the batch's maxima is TOO_LARGE; a failed image does not disturb the
 * others and its pixels are unspecified. Asynchronous on hip_stream (NULL = the context's
 * stream), no host read-back. Returns ICX_PNGR_OK or ICX_PNGR_INTERNAL_ERR. */
typedef struct icx_png_batch icx_png_batch;
icx_png_batch* icx_png_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_png_batch_destroy(icx_png_batch* b);
int icx_png_batch_decode(icx_png_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_png_batch_decode ("parse", "gather", "inflate",
 * "unfilter", "expand"; synchronises). Returns the number of stages. */
int icx_png_batch_stage_times(const icx_png_batch* b, const char** names, float* ms, int cap);

/* ---- Radiance .hdr read (Image::readHdr, codecs.cpp:706-777) -----------------------------------
 * Output as readHdr returns it (d = 4, Type::FLOAT): 4 floats per pixel, rows in file order,
 * R, G, B = convertComponent(E - 128, v) = v * 2^(E - 136) (codecs.cpp:610-615; exact, so the
 * GPU result equals the reference's bit for bit) and the fourth float = E (:624).
 * Where the reference's behaviour is undefined (runs past the scanline, a run on a scanline's first
 * pixel, a header without an empty line, a partial resolution line) the result is MALFORMED or
 * BAD_HEADER; rows after a scanline the reference stops at (it leaves them uninitialised,
 * :765-769) are zero and counted out of *rows. */
enum icx_hdr_result {
    ICX_HDR_OK = 0,            /* all rows decoded                                   */
    ICX_HDR_NOT_RADIANCE = 1,  /* "Invalid file format": no "#?RADIANCE" (:717-720)  */
    ICX_HDR_BAD_HEADER = 2,    /* header / resolution line not as readHdr parses it   */
    ICX_HDR_MALFORMED = 3,     /* run-length data the reference cannot decode (UB)     */
    ICX_HDR_TRUNCATED = 4,     /* the file ends first: rows < height                   */
    ICX_HDR_TOO_LARGE = 5,     /* larger than the batch workspace / the write's slot   */
    ICX_HDR_INVALID_ARGUMENT = 6, /* the write refuses these arguments (below)          */
    ICX_HDR_INTERNAL_ERR = -1  /* HIP failure (see icx_last_error)                     */
};
/* Header only (host): width/height of a well-formed header, else the error code. */
int icx_hdr_probe(const uint8_t* data, size_t size, int* width, int* height);
/* One image, host in / host out: *out receives a malloc()'d width*height*4 float buffer (free
 * with icx_free); *rows = decoded rows. */
int icx_hdr_decode(icx_ctx* ctx, const uint8_t* data, size_t size, float** out, int* width, int* height,
                   int* rows);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output floats at
 * d_out + i*out_stride (out_stride >= 4*width*height of every image), per-image status in
 * d_status[i] and {width, height, rows} in d_dims[3i..]. Asynchronous on hip_stream (NULL = the
 * context's stream). Returns ICX_HDR_OK or ICX_HDR_INTERNAL_ERR. */
typedef struct icx_hdr_batch icx_hdr_batch;
icx_hdr_batch* icx_hdr_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_hdr_batch_destroy(icx_hdr_batch* b);
int icx_hdr_batch_decode(icx_hdr_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, float* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_hdr_batch_decode ("parse", "locate", "unpack",
 * "convert"; synchronises). Returns the number of stages. */
int icx_hdr_batch_stage_times(const icx_hdr_batch* b, const char** names, float* ms, int cap);
/* How each image of the last icx_hdr_batch_decode was located (waits for that call's work, on
 * whichever stream it ran). modes[i]: 0 the file failed before its scanlines were looked for (a
 * header error, TOO_LARGE), 1 every row is a plain RGBE row at data start + 4*width*i, 2 the
 * new-style scanline starts found in parallel chain from the data start over all rows, 3 one lane
 * walked the scanlines serially (any other file; the same pixels). ncand[i]: the aligned or
 * unaligned occurrences of "2 2 width>>8 width&255" in the pixel data (0 for widths outside
 * 8..32767 and for mode 0). Either array may be NULL; at most cap entries are written. Returns the
 * number of images of that call (0 before the first), or ICX_HDR_INTERNAL_ERR. */
int icx_hdr_batch_locate_stats(const icx_hdr_batch* b, int32_t* modes, int32_t* ncand, int cap);

/* ---- Radiance .hdr write (Image::writeHdr, codecs.cpp:779-818) ----------------------------------
 * The file: the reference's header bytes (:791),
 *     "#?RADIANCE\nSOFTWARE=GEGL\nFORMAT=32-bit_rle_rgbe\n\n-Y <h> +X <w>\n",
 * then the rows in the order of the input. icx_hdr_decode and the reference's readHdr both parse it.
 *
 * d = 4 (the reference's form; what the read returns): per pixel four floats R, G, B, Ef. In exact
 * arithmetic,
 *     E   = Ef truncated toward zero and clamped to 0..255 (NaN gives 0)
 *     m_c = min(255, floor(v_c * 2^(136 - E)))   for finite v_c > 0
 *     m_c = 255 for +inf;  m_c = 0 for NaN, negative values and +-0
 * and the bytes written are m_R, m_G, m_B, E. This is the reference's
 * (unsigned char)(val * 256.0f * pow(0.5f, E - 128)) with invConvertComponent's arguments in the
 * intended order (the reference swaps them, :810) and the out-of-range casts, undefined there,
 * defined. It is the exact inverse of the read (v = m * 2^(E - 136), bit for bit): writing what the
 * read returned reproduces every RGBE byte of every pixel. The values hold whatever the denormal
 * mode: they are taken from the floats' exponent and mantissa bits (subnormal inputs included).
 *
 * d = 3 (extension: plain float R, G, B, no exponent channel): NaN and negative components count
 * as 0 and +inf as FLT_MAX; mx = the largest component. mx < 1e-32f (Radiance's setcolr threshold)
 * writes 0, 0, 0, 0. Otherwise mx = f * 2^e with f in [0.5, 1), E = min(255, e + 128), and the
 * mantissas follow the d = 4 formula with that E, so the largest mantissa is in 128..255 whenever
 * e + 128 <= 255. The scale is the power of two 2^(136 - E), not setcolr's frexp(d) * 256 / d: it
 * is exact and cannot produce 256.
 *
 * Pixel data, rle == 0: four bytes per pixel, what the reference writes. One property is shared
 * with the reference: a flat row whose first pixel is (2, 2, B < 128, .) is taken by every reader
 * for a run-length coded row, and a flat pixel (1, 1, 1, .) for an old-style repeat. Only d = 4
 * input with unnormalised mantissas can produce these; d = 3 output never does (its largest
 * mantissa is >= 128).
 *
 * Pixel data, rle != 0 (extension): when 8 <= w <= 32767 each row is 2, 2, w>>8, w&255 followed by
 * its four component planes (all R, then all G, all B, all E), each packed by this rule (serial as
 * stated; the kernels give the same bytes); outside that width range the file is flat.
 *     i = 0
 *     while i < w:
 *         r = length of the longest stretch p[i..i+r) of equal bytes, r <= min(127, w - i)
 *         if r >= 4:  emit 128 + r, p[i];                               i += r
 *         else:       n = number of bytes k = i, i+1, ... taken while k < w, k - i < 128 and
 *                         not (k > i and p[k] == p[k+1] == p[k+2] == p[k+3], all four inside the row)
 *                     emit n, then the n bytes;                          i += n
 * Run codes are 129..255 (1..127 repeats), literal codes 1..128: what decrunchHDR (:686-700) reads.
 * A plane never exceeds w + ceil(w/128) bytes.
 *
 * Any other d, a width or height < 1, w*h > 2^30 or a null pointer -> ICX_HDR_INVALID_ARGUMENT
 * (checked before any device work). */
/* The largest file a write can give: the header + h*(4 + 4*(w + ceil(w/128))) for the run-length
 * form, the header + 4*w*h (the exact size) for flat; 0 for arguments the writes refuse. Host only. */
size_t icx_hdr_encode_bound(int width, int height, int d, int rle);
/* Host pixels in (width*height*d floats), *out receives the malloc()'d file (free with icx_free).
 * Returns an icx_hdr_result. */
int icx_hdr_save_to_memory(icx_ctx* ctx, const float* pixels, int width, int height, int d, int rle, uint8_t** out,
                           size_t* size);
/* The same file written to `path` (ICX_HDR_INTERNAL_ERR when it cannot be written). */
int icx_hdr_save_to_file(icx_ctx* ctx, const char* path, const float* pixels, int width, int height, int d, int rle);
/* n writes with pixels and files resident on the device: image i's pixels at d_src[i] (a host
 * array of device pointers; widths / heights are host arrays), its file to d_out + i*out_stride
 * (any alignment), the file's length to d_sizes[i] and an icx_hdr_result to d_status[i] (device
 * arrays): INVALID_ARGUMENT for a bad size or null source, TOO_LARGE (nothing of the file
 * written, d_sizes[i] says what it needs) when it is longer than out_stride. d not 3 or 4, n < 0,
 * n > 65535 (one call's limit: split larger batches) or a null array with n > 0 -> the call returns
 * ICX_HDR_INVALID_ARGUMENT and writes nothing. Runs on hip_stream (NULL = the context's stream) and
 * synchronises with it. */
int icx_hdr_encode_device_batch(icx_ctx* ctx, int n, const float* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream);

/* ---- OpenEXR read (Image::readExr, codecs.cpp:464-493 -> tinyexr LoadEXRFromMemory, tinyexr.h:6645) ----
 * Output as LoadEXRFromMemory returns it: width*height*4 floats (R, G, B, A by channel name; a
 * one-channel image repeats its channel in all four; no A channel -> 1.0), data-window rows in
 * tinyexr's order. HALF samples are converted bit for bit (half_to_float), FLOAT copied, UINT
 * sample bits copied unconverted (tinyexr reads them through its float** view).
 * Scope: single-part scanline or tiled files, NONE / RLE / ZIPS / ZIP / PIZ compression (the
 * reference builds tinyexr with TINYEXR_USE_PIZ 1, tinyexr.h:126-128); mip- and rip-mapped tiled
 * files decode every level's tiles as DecodeChunk does (a failure in any level fails the read) and
 * return level 0; a broken offset table is reconstructed from the chunk headers
 * (ReconstructTileOffsets, where the multi-part and deep version bits change the chunk walk;
 * LoadEXRFromMemory does not reject them, only LoadEXR does, tinyexr.h:6268-6270). Pixels no
 * chunk wrote (tinyexr leaves them uninitialised) are 0. */
enum icx_exr_result {
    ICX_EXR_SUCCESS = 0,                /* TINYEXR_SUCCESS                          */
    ICX_EXR_INVALID_MAGIC_NUMBER = -1,  /* TINYEXR_ERROR_INVALID_MAGIC_NUMBER       */
    ICX_EXR_INVALID_EXR_VERSION = -2,   /* TINYEXR_ERROR_INVALID_EXR_VERSION        */
    ICX_EXR_INVALID_ARGUMENT = -3,      /* TINYEXR_ERROR_INVALID_ARGUMENT           */
    ICX_EXR_INVALID_DATA = -4,          /* TINYEXR_ERROR_INVALID_DATA               */
    ICX_EXR_UNSUPPORTED_FORMAT = -8,    /* TINYEXR_ERROR_UNSUPPORTED_FORMAT         */
    ICX_EXR_INVALID_HEADER = -9,        /* TINYEXR_ERROR_INVALID_HEADER             */
    ICX_EXR_UNSUPPORTED_FEATURE = -10,  /* TINYEXR_ERROR_UNSUPPORTED_FEATURE        */
    ICX_EXR_INTERNAL_ERR = -100         /* HIP failure (see icx_last_error)         */
};
/* Header, offset table and chunk headers only (host): the data window size, or the error code
 * LoadEXRFromMemory would return before decoding pixels. */
int icx_exr_probe(const uint8_t* data, size_t size, int* width, int* height);
/* One image, host in / host out: *out_rgba receives a malloc()'d width*height*4 float buffer
 * (free with icx_free). Returns an icx_exr_result. */
int icx_exr_decode(icx_ctx* ctx, const uint8_t* data, size_t size, float** out_rgba, int* width, int* height);
/* The same read with the file already resident on the device (batch pipelines, benchmarks): the
 * header and offset table are planned from the host copy `data`; the kernels read the device copy
 * `d_data` (the same `size` bytes followed by 16 zero bytes; 16-byte aligned, since the chunk
 * readers load 16-byte words: a misaligned pointer is ICX_EXR_INVALID_ARGUMENT) and write
 * width*height*4 floats to
 * `d_out` (room for `out_floats`; too little -> ICX_EXR_INTERNAL_ERR). Synchronises with the
 * context's stream; returns an icx_exr_result. */
int icx_exr_decode_device(icx_ctx* ctx, const uint8_t* data, const uint8_t* d_data, size_t size, float* d_out,
                          size_t out_floats, int* width, int* height);
/* n such reads in one call: every file is planned on the host, then the compressed chunks of all
 * n files are decompressed by one launch (a workgroup per chunk) before each file is converted --
 * one 2048^2 ZIP file has 128 chunks, a batch keeps thousands in flight. codes[i] gets file i's
 * icx_exr_result, widths[i] / heights[i] its size (0 when it fails). Returns ICX_EXR_SUCCESS when
 * the call ran (per-file results in codes), ICX_EXR_INVALID_ARGUMENT for a null pointer, or
 * ICX_EXR_INTERNAL_ERR (HIP failure, an output buffer too small; see icx_last_error). */
int icx_exr_decode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* data, const uint8_t* const* d_data,
                                const size_t* sizes, float* const* d_out, const size_t* out_floats, int32_t* codes,
                                int32_t* widths, int32_t* heights);

/* ---- OpenEXR write (Image::writeExr, codecs.cpp:495-505 -> tinyexr SaveEXR, tinyexr.h:9333) ----
 * `data`: width*height*components interleaved floats, components 1, 3 or 4 (file channels A /
 * B,G,R / A,B,G,R). save_as_fp16 > 0 stores HALF samples (float_to_half_full), otherwise FLOAT.
 * Single-part scanline file; NONE when width < 16 && height < 16, else ZIP in chunks of 16 lines.
 * Header, offset table, chunk headers, NONE payloads and ZIP chunks stored raw are tinyexr's bytes;
 * a compressed ZIP chunk is a zlib stream of our own that inflates to exactly the bytes tinyexr
 * compresses (and is stored raw exactly when that stream is not smaller than the samples).
 * components not in {1, 3, 4}, width or height < 1, a null pointer, or a chunk of 2 GiB or more
 * -> ICX_EXR_INVALID_ARGUMENT. */
/* Host pixels in, *out receives the malloc()'d file (free with icx_free). Returns an icx_exr_result. */
int icx_exr_save_to_memory(icx_ctx* ctx, const float* data, int width, int height, int components, int save_as_fp16,
                           uint8_t** out, size_t* size);
/* SaveEXR with a context: the same file written to `path` (ICX_EXR_INTERNAL_ERR when it cannot
 * be written; see icx_last_error). */
int icx_exr_save_to_file(icx_ctx* ctx, const char* path, const float* data, int width, int height, int components,
                         int save_as_fp16);
/* The largest file such a write can give (header + offset table + chunk headers + raw payloads);
 * 0 for arguments the writes refuse. Host only. */
size_t icx_exr_encode_bound(int width, int height, int components, int save_as_fp16);
/* The write with pixels and file resident on the device: `d_src` floats in, the file to `d_out`
 * (room for `cap` bytes, any alignment), its length to *size. A file longer than `cap` is
 * ICX_EXR_INTERNAL_ERR: nothing of it is written, *size says what it needs. Synchronises with
 * the context's stream. */
int icx_exr_encode_device(icx_ctx* ctx, const float* d_src, int width, int height, int components, int save_as_fp16,
                          uint8_t* d_out, size_t cap, size_t* size);
/* n such writes in one call: the chunks of all n images go through every kernel in one launch
 * (a 2048^2 image has 128 independent chunks). codes[i] gets image i's icx_exr_result, sizes[i]
 * its file length. Returns ICX_EXR_SUCCESS when the call ran (per-image results in codes),
 * ICX_EXR_INVALID_ARGUMENT for a null array, or ICX_EXR_INTERNAL_ERR (HIP failure). */
int icx_exr_encode_device_batch(icx_ctx* ctx, int n, const float* const* d_src, const int32_t* widths,
                                const int32_t* heights, int components, int save_as_fp16, uint8_t* const* d_out,
                                const size_t* caps, int32_t* codes, size_t* sizes);

/* ---- Targa read (Image::readTga, codecs.cpp:1304-1407) -------------------------------------------
 * Output as readTga returns it: Type::UBYTE, rows top-down, channels R,G,B(,A); channels is 3 or 4
 * for colour (the map's entry size for paletted files, bits / 8 otherwise) and 1 for monochrome.
 * Accepted: types 2 / 10 (true colour raw / RLE) at 24 or 32 bits, file order B,G,R(,A), alpha as
 * stored; types 3 / 11 (monochrome) at 8 bits; types 1 / 9 (paletted; colour-map type 1) with map
 * entries of 24 or 32 bits and indices of 8 or 16 bits. Type 9 is decoded (the reference leaves
 * it as a TODO and returns zeros).
 * Deliberate deviations: the header is 18 bytes (the reference subtracts a padded
 * sizeof(Header) of 20 and reads two bytes too few); the ID field is *ID length* bytes (the
 * reference skips *descriptor* bytes); palette index i selects entry i - origin, and an index
 * outside the map gives zero bytes (the reference reads outside its buffer); descriptor bit 5
 * (top-left origin) is honoured, so the output is always top-down (the reference always flips);
 * bit 4 (right-to-left) is UNSUPPORTED; run-length packets may cross row ends, as in the
 * reference; bytes after the image data (footer, extension area) are ignored.
 * Packets are examined in stream order and the first that fails decides: its header byte or
 * payload not wholly inside the file -> TRUNCATED, otherwise more pixels than are still missing ->
 * MALFORMED (the reference writes past its buffer). Raw data or a colour map that run past the
 * file are TRUNCATED. A failed image yields no pixels. */
enum icx_tga_result {
    ICX_TGA_OK = 0,
    ICX_TGA_BAD_HEADER = 1,        /* < 18 bytes, zero width / height, colour-map type > 1, a paletted
                                      type without a map, an image type not in 0-3, 9-11            */
    ICX_TGA_UNSUPPORTED = 2,       /* 15/16-bit colour, map entries or monochrome, any other depth,
                                      descriptor bit 4                                              */
    ICX_TGA_NO_IMAGE = 3,          /* type 0: the reference leaves pixels_ null                      */
    ICX_TGA_MALFORMED = 4,         /* a packet holds more pixels than are still missing             */
    ICX_TGA_TRUNCATED = 5,         /* the file ends first                                           */
    ICX_TGA_TOO_LARGE = 6,         /* larger than the batch workspace / the output slot             */
    ICX_TGA_INVALID_ARGUMENT = 7,  /* write: channels not 1, 3, 4; width / height not 1..65535; null */
    ICX_TGA_INTERNAL_ERR = -1      /* HIP failure (see icx_last_error)                              */
};
/* Header only (host): size and channels, or the code the header (for raw types: and the file's
 * length) gives. The packets of an RLE file are checked by the decode. */
int icx_tga_probe(const uint8_t* data, size_t size, int* width, int* height, int* channels);
/* One image, host in / host out: *out receives a malloc()'d width*height*channels byte buffer
 * (free with icx_free), null unless ICX_TGA_OK. A code the probe gives returns without touching
 * the GPU; an image of more than 2^30 pixels is ICX_TGA_TOO_LARGE (a batch workspace holds
 * max_width * max_height <= 2^30). The header checks run in the order BAD_HEADER, NO_IMAGE,
 * UNSUPPORTED, TRUNCATED (ID field, colour map, raw data). */
int icx_tga_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* width, int* height,
                   int* channels);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output bytes at
 * d_out + i*out_stride (out_stride >= 4*max_width*max_height), per-image status in d_status[i]
 * and {width, height, channels} in d_dims[3i..] (zero for a failed image, whose slot is
 * unspecified). Asynchronous on hip_stream (NULL = the context's stream), no host read-back.
 * Returns ICX_TGA_OK or ICX_TGA_INTERNAL_ERR. */
typedef struct icx_tga_batch icx_tga_batch;
icx_tga_batch* icx_tga_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_tga_batch_destroy(icx_tga_batch* b);
int icx_tga_batch_decode(icx_tga_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_tga_batch_decode ("parse", "locate", "expand", "raw";
 * synchronises). Returns the number of stages. */
int icx_tga_batch_stage_times(const icx_tga_batch* b, const char** names, float* ms, int cap);

/* ---- Targa write (Image::writeTga, codecs.cpp:1410-1437) -----------------------------------------
 * `pixels`: width*height*d bytes, rows top-down, R,G,B(,A) or one grey byte; d = 1, 3 or 4.
 * The reference's 18 header bytes (0,0,2,0...0, w, h, d*8, 0x20) and the rows top-down.
 * Two deviations, by evident intent: the payload is B,G,R(,A) (the reference stores R,G,B, which
 * every TGA reader, its own included, shows with red and blue exchanged), and d = 1 is written as
 * image type 3 (the reference writes type 2 with 8 bits, which is not a TGA form).
 * Extension (rle != 0): type 10 (d = 3, 4) or 11 (d = 1); packets never cross a row; each row is
 * packed by this greedy rule (serial as stated; the kernels give the same bytes):
 *     i = 0
 *     while i < w:
 *         r = length of the longest stretch p[i..i+r) of equal pixels, r <= min(128, w - i)
 *         if r >= 2:  emit 0x80 | (r-1), one pixel;             i += r
 *         else:       n = number of pixels k = i, i+1, ... taken while k < w, k - i < 128 and
 *                         not (k+1 < w and p[k] == p[k+1])
 *                     emit n-1, n pixels;                        i += n
 * Any other d, width or height outside 1..65535, or a null pointer -> ICX_TGA_INVALID_ARGUMENT. */
/* The largest file a write can give, 18 + w*h*(d+1); 0 for arguments the writes refuse. Host only. */
size_t icx_tga_encode_bound(int width, int height, int d);
/* Host pixels in, *out receives the malloc()'d file (free with icx_free). Returns an icx_tga_result. */
int icx_tga_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int rle, uint8_t** out,
                           size_t* size);
/* The same file written to `path` (ICX_TGA_INTERNAL_ERR when it cannot be written). */
int icx_tga_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d, int rle);
/* n writes with pixels and files resident on the device: image i's pixels at d_src[i] (a host
 * array of device pointers; widths / heights are host arrays), its file to d_out + i*out_stride
 * (any alignment), the file's length to d_sizes[i] and an icx_tga_result to d_status[i] (device
 * arrays): INVALID_ARGUMENT for a bad size or null source, TOO_LARGE (nothing of the file
 * written, d_sizes[i] says what it needs) when it is longer than out_stride. d not in 1, 3, 4,
 * n < 0, n > 65535 (one call's limit: split larger batches) or a null array with n > 0 ->
 * the call returns ICX_TGA_INVALID_ARGUMENT. Runs on hip_stream (NULL = the context's stream)
 * and synchronises with it. */
int icx_tga_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream);

/* ---- BMP read (Image::readBmp, codecs.cpp:255-320) -------------------------------------------------
 * Output: Type::UBYTE, rows top-down whatever the sign of the height, channels R,G,B(,A).
 * Container: 14 bytes ("BM", bfSize, reserved, bfOffBits), then a DIB header of 12 (core: unsigned
 * 16-bit width and height, 3-byte palette entries), 40, 52, 56, 64 (OS/2 v2: read as its first 40
 * bytes, accepted only with compression 0), 108 or 124 bytes. biPlanes is ignored.
 * Compression: 0 raw (any bit count); 1 RLE8 (8 bits); 2 RLE4 (4 bits); 3 BITFIELDS and
 * 6 ALPHABITFIELDS (16 and 32 bits): three (3) or four (6) masks follow a 40-byte header, in a 52-byte
 * header three and in larger ones four masks are inside the header, whichever of the two values
 * the compression has (a 52-byte header has no alpha mask; with compression 0 the masks are
 * ignored). Defaults with compression 0: 16 bits is 5-5-5, 32 bits is B,G,R,X with the fourth byte
 * dropped. A field value v of n <= 8 bits maps to (v * 510 + m) / (2 * m), m = 2^n - 1 (exact
 * rounding of v * 255 / m); a wider field gives its top 8 bits; a zero colour mask gives 0.
 * Channels: 4 only for 16- or 32-bit files with a nonzero alpha mask; 1 only for an 8-bit file whose
 * every palette entry i is (i, i, i) (the index is then the grey value); 3 otherwise. The palette
 * has biClrUsed entries (0: 2^bits) of B,G,R(,x); an index at or past that number gives zero bytes.
 * Raw rasters: rows of ((w * bits + 31) / 32) * 4 bytes from bfOffBits, for 1 and 4 bits the most
 * significant bits first; the file's first row is the bottom row unless the height is negative.
 * Bytes after the raster are ignored.
 * Run-length streams (serial as stated; the kernels give the same bytes). The cursor starts at
 * x = 0, y = 0, the bottom row; the output starts as palette entry 0 everywhere; packets are
 * 2-byte aligned from bfOffBits:
 *     n v   (n >= 1)   n pixels of v (RLE4: the high and the low nibble alternate, high first); x += n
 *     0 0              x = 0, y += 1
 *     0 1              end of bitmap
 *     0 2 dx dy        x += dx, y += dy
 *     0 n p... (n >= 3)  n literal pixels, n bytes (RLE4: (n + 1) / 2), padded to an even length; x += n
 * The walk ends at the end-of-bitmap packet or where fewer than 2 bytes remain (also OK). A packet
 * whose payload, pad byte included, is not wholly inside the file is TRUNCATED, and the image then
 * yields no pixels. Pixels that land at x >= w or y >= h are dropped and the cursor keeps counting:
 * no saturation, no wrap into the next row.
 * Deliberate deviations from the reference: the output is R,G,B (the reference copies the file's
 * B,G,R bytes as they are, and its write stores them as they are); rows are padded to 4 bytes (the reference skips w % 4
 * bytes, right only where w % 4 is 0 or 2); a negative height gives top-down rows and a positive h
 * (the reference returns h < 0); every form beyond 24-bit BITMAPINFOHEADER files is read. */
enum icx_bmp_result {
    ICX_BMP_OK = 0,
    ICX_BMP_NOT_BMP = 1,           /* fewer than 18 bytes, or no "BM"                                */
    ICX_BMP_BAD_HEADER = 2,        /* a header size not listed or past the file; width <= 0, height 0
                                      or INT_MIN; a bit count not in 1, 4, 8, 16, 24, 32; a wrong bit
                                      count for compression 1, 2, 3, 6; biClrUsed > 2^bits; masks past
                                      the file; bfOffBits before the end of the palette or masks     */
    ICX_BMP_UNSUPPORTED = 3,       /* compression 4, 5 or unknown; a 64-byte header with compression;
                                      RLE with a negative height; a mask whose set bits are not
                                      contiguous; masks that overlap                                 */
    ICX_BMP_TRUNCATED = 4,         /* palette, raster or a run-length packet past the file's end     */
    ICX_BMP_TOO_LARGE = 5,         /* more than 2^30 pixels; larger than the batch workspace or slot */
    ICX_BMP_INVALID_ARGUMENT = 6,  /* write: channels not 1, 3, 4; width / height not 1..65535; null */
    ICX_BMP_INTERNAL_ERR = -1      /* HIP failure (see icx_last_error)                               */
};
/* Header only (host): size and channels, or the code the header (for raw files: and the file's
 * length) gives, checked in the order NOT_BMP, BAD_HEADER, UNSUPPORTED, TOO_LARGE, TRUNCATED. The
 * packets of an RLE file are walked by the decode. Null data is NOT_BMP. */
int icx_bmp_probe(const uint8_t* data, size_t size, int* width, int* height, int* channels);
/* One image, host in / host out: *out receives a malloc()'d width*height*channels byte buffer
 * (free with icx_free), null unless ICX_BMP_OK. A code the probe gives returns without touching
 * the GPU. */
int icx_bmp_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* width, int* height,
                   int* channels);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output bytes at
 * d_out + i*out_stride (out_stride >= 4*max_width*max_height, any alignment), per-image status in
 * d_status[i] and {width, height, channels} in d_dims[3i..] (zero for a failed image, whose slot is
 * unspecified). The workspace covers run-length streams of up to 2*max_width*max_height +
 * 2*max_height + 2 bytes (every pixel its own packet, an end-of-line per row); a longer stream whose
 * walk has not ended by then is ICX_BMP_TOO_LARGE (icx_bmp_decode sizes its workspace by the file).
 * The tile tables for that bound are allocated at creation, whatever the files turn out to be:
 * 132 x 16 bytes per 4096 stream bytes, about 1.03 x max_width x max_height bytes per image
 * (1.1 MB at 1024 x 1024, 277 MB for a batch of 256) beside the caller's output slots.
 * Asynchronous on hip_stream (NULL = the context's stream), no host read-back.
 * Returns ICX_BMP_OK or ICX_BMP_INTERNAL_ERR. */
typedef struct icx_bmp_batch icx_bmp_batch;
icx_bmp_batch* icx_bmp_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_bmp_batch_destroy(icx_bmp_batch* b);
int icx_bmp_batch_decode(icx_bmp_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_bmp_batch_decode ("parse", "locate", "fill", "expand",
 * "raw"; synchronises). Returns the number of stages. */
int icx_bmp_batch_stage_times(const icx_bmp_batch* b, const char** names, float* ms, int cap);

/* ---- BMP write (Image::writeBmp, codecs.cpp:324-375) -----------------------------------------------
 * `pixels`: width*height*d bytes, rows top-down, R,G,B(,A) or one grey byte; d = 1, 3 or 4. The
 * 14-byte file header carries a correct bfSize (the reference stores the payload size without the
 * 54 header bytes). Rows are written bottom-up and padded to 4 bytes with zeros; biSizeImage is
 * set; the pels-per-metre fields are 0, as in the reference.
 *     d = 3   a 40-byte header, 24 bits, BI_RGB, rows B,G,R
 *     d = 4   by evident intent (the reference writes 4-byte pixels under a 24-bit header): a
 *             108-byte V4 header, 32 bits, BI_BITFIELDS, masks 00FF0000, 0000FF00, 000000FF,
 *             FF000000, colour space LCS_sRGB ("BGRs"), the other V4 fields zero; rows B,G,R,A.
 *             The read returns such a file with 4 channels
 *     d = 1   by evident intent: 8 bits with a 256-entry grey palette (biClrUsed 256); the read
 *             returns it with 1 channel
 * Any other d, width or height outside 1..65535, or a null pointer -> ICX_BMP_INVALID_ARGUMENT.
 * Run-length coded files are not written. */
/* The file's size, bfOffBits + row bytes * height; 0 for arguments the writes refuse. Host only. */
size_t icx_bmp_encode_bound(int width, int height, int d);
/* Host pixels in, *out receives the malloc()'d file (free with icx_free). Returns an icx_bmp_result. */
int icx_bmp_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, uint8_t** out,
                           size_t* size);
/* The same file written to `path` (ICX_BMP_INTERNAL_ERR when it cannot be written). */
int icx_bmp_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d);
/* n writes with pixels and files resident on the device: image i's pixels at d_src[i] (a host
 * array of device pointers; widths / heights are host arrays), its file to d_out + i*out_stride
 * (any alignment), the file's length to d_sizes[i] and an icx_bmp_result to d_status[i] (device
 * arrays): INVALID_ARGUMENT for a bad size or null source, TOO_LARGE (nothing of the file
 * written, d_sizes[i] says what it needs) when it is longer than out_stride. d not in 1, 3, 4,
 * n < 0, n > 65535 (one call's limit: split larger batches) or a null array with n > 0 ->
 * the call returns ICX_BMP_INVALID_ARGUMENT. Runs on hip_stream (NULL = the context's stream)
 * and synchronises with it. */
int icx_bmp_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream);

/* ---- DDS read and write (Image::readDds / writeDds over nv_dds) -------------------------------------
 * The reference never decompresses: for a DXT file it copies width*height*d bytes out of a buffer
 * of compressed blocks. The contract is therefore written out here and pinned by an independent
 * restatement (tests/ddsutil.py) and by PIL, not by the reference's output.
 * Output: rows top-down (the file's order; the reference's two flips cancel), channels R,G,B(,A),
 * `type` UBYTE, USHORT or FLOAT with the values of icx_pnm_type.
 * Container: "DDS ", a 124-byte header (dwSize 124, ddspf.dwSize 32, width and height nonzero), then
 * a 20-byte DX10 header when ddspf.dwFlags & 4 and the FourCC is "DX10". dwFlags,
 * dwPitchOrLinearSize and dwMipMapCount are not trusted: rows and blocks are tightly packed, only
 * the top level is read, and it must lie wholly inside the file; bytes after it are ignored.
 * Block formats (UBYTE), by FourCC or DXGI format:
 *     DXT1                 71, 72   BC1   3 channels (the count nv_dds reports; the transparent entry
 *                                         of a 3-colour block gives 0,0,0)
 *     DXT2, DXT3           74, 75   BC2   4
 *     DXT4, DXT5, BC3U     77, 78   BC3   4
 *     ATI1, BC4U           80       BC4   1
 *     ATI2, BC5U           83       BC5   2 (the red block first)
 * Block arithmetic, all integer with truncating divisions. Colour: c0, c1 little-endian 5-6-5,
 * r8 = r<<3 | r>>2, g8 = g<<2 | g>>4, b8 = b<<3 | b>>2; with c0 > c1 (BC2, BC3: always) the palette
 * is p0, p1, (2p0+p1)/3, (p0+2p1)/3, otherwise p0, p1, (p0+p1)/2, 0; pixel i = 4y + x takes bits
 * 2i..2i+1 of the 32-bit index word. BC2 alpha: the first 8 bytes hold 4-bit values, little-endian,
 * a = a4 * 17. BC3 alpha, BC4 and each half of BC5: bytes a0, a1, then 48 bits of 3-bit indices,
 * little-endian; with a0 > a1 entries 2..7 are ((7-k)a0 + k a1)/7 for k = 1..6, otherwise entries
 * 2..5 are ((5-k)a0 + k a1)/5 for k = 1..4, entry 6 is 0 and entry 7 is 255. Blocks cover
 * ceil(w/4) x ceil(h/4); pixels outside the image are dropped.
 * Uncompressed files (no FourCC flag): dwRGBBitCount 8, 16, 24 or 32; each of the masks R, G, B, A
 * zero or contiguous, inside the bit count and disjoint from the others. With ddspf.dwFlags &
 * 0x20000 (luminance): 1 channel from the R mask, 2 with a nonzero A mask. Otherwise by the masks:
 * only A: 1 channel, the alpha; only R: 1; R and G: 2; R, G, B: 3, or 4 with A (an X8 form gives 3,
 * the fourth byte dropped; nv_dds says 4). Field scaling is BMP's, above.
 * Copied forms, samples as stored (little-endian, the host's order): FLOAT DXGI 2 / FourCC number
 * 116 (4 channels), 6 (3), 16 / 115 (2), 41 / 114 (1); USHORT 11 / 36 (4), 35 (2), 56 (1).
 * DX10 8-bit forms: 28, 29 R,G,B,A; 87, 91 B,G,R,A -> 4 channels; 88, 93 B,G,R,X -> 3; 61 -> 1; 49 -> 2. */
enum icx_dds_result {
    ICX_DDS_OK = 0,
    ICX_DDS_NOT_DDS = 1,           /* fewer than 4 bytes, or no "DDS "                                */
    ICX_DDS_BAD_HEADER = 2,        /* fewer than 128 bytes (148 with a DX10 header); dwSize not 124;
                                      ddspf.dwSize not 32; width or height 0; an uncompressed file's
                                      bit count not 8, 16, 24 or 32                                  */
    ICX_DDS_UNSUPPORTED = 3,       /* cubemap (dwCaps2 & 0x200) or volume (0x200000); DX10 arraySize
                                      not 1, the cube flag, a resourceDimension other than 3; BC4S,
                                      BC5S, BC6H, BC7, RGBG, GRGB, half floats and any other FourCC or
                                      DXGI value; masks not contiguous, past the bit count, overlapping
                                      or in a combination not listed                                 */
    ICX_DDS_TRUNCATED = 4,         /* the top level ends past the file's end                         */
    ICX_DDS_TOO_LARGE = 5,         /* more than 2^30 pixels; larger than the batch's maxima or slot  */
    ICX_DDS_INVALID_ARGUMENT = 6,  /* write: d not 1..4, width / height not 1..65535, a type other
                                      than UBYTE, an unknown format, null; batch read: d_out or
                                      out_stride not a multiple of 16                                */
    ICX_DDS_INTERNAL_ERR = -1      /* HIP failure (see icx_last_error)                               */
};
enum icx_dds_format { ICX_DDS_RAW = 0, ICX_DDS_BC = 1 };
/* Header only (host): size, channels and type, or the code, checked in the order NOT_DDS,
 * BAD_HEADER, UNSUPPORTED, TOO_LARGE, TRUNCATED. Null data is NOT_DDS. */
int icx_dds_probe(const uint8_t* data, size_t size, int* width, int* height, int* channels, int* type);
/* One image, host in / host out: *out receives a malloc()'d buffer of width*height*channels
 * elements of `type` (free with icx_free), null unless ICX_DDS_OK. A code the probe gives returns
 * without touching the GPU. */
int icx_dds_decode(icx_ctx* ctx, const uint8_t* data, size_t size, void** out, int* width, int* height, int* channels,
                   int* type);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]) (any alignment), its
 * elements at d_out + i*out_stride bytes (d_out 16-byte aligned and out_stride a multiple of 16,
 * else the call returns ICX_DDS_INVALID_ARGUMENT), per-image status in d_status[i] and {width,
 * height, channels, type} in d_dims[4i..] (zero for a failed image). An image wider or taller than
 * the batch's maxima, or whose elements take more than out_stride bytes, is ICX_DDS_TOO_LARGE. A
 * failed image leaves the others alone; nothing is written outside the slots, nor inside a slot
 * past its image's last byte, and nothing at all for a failed image. Asynchronous on hip_stream
 * (NULL = the context's stream), no host read-back. */
typedef struct icx_dds_batch icx_dds_batch;
icx_dds_batch* icx_dds_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_dds_batch_destroy(icx_dds_batch* b);
int icx_dds_batch_decode(icx_dds_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, void* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_dds_batch_decode ("parse", "blocks", "raw"; synchronises).
 * Returns the number of stages. */
int icx_dds_batch_stage_times(const icx_dds_batch* b, const char** names, float* ms, int cap);

/* DDS write: `pixels` is width*height*d bytes, rows top-down, d = 1..4, width and height 1..65535.
 * Header, both formats: dwFlags 0x1007, dwCaps 0x1000, mip count, depth and the reserved words 0.
 * ICX_DDS_RAW is what writeDds does, made well formed: dwFlags |= 0x8 with pitch width*d (the
 * reference stores a dword-aligned pitch for rows it writes unpadded);
 *     d = 3   24 bits, ddspf flags 0x40, masks FF0000, FF00, FF: rows B,G,R
 *     d = 4   32 bits, flags 0x41, plus A FF000000: rows B,G,R,A
 *     d = 1   8 bits, flags 0x20000 (luminance), R mask FF (the reference writes d = 1 under RGB
 *             masks that cannot hold it)
 *     d = 2   16 bits, flags 0x20001, R 00FF, A FF00
 * and the read returns each of these with the same d. ICX_DDS_BC is an extension: dwFlags |=
 * 0x80000 with linear size = blocks x block bytes, ddspf flags 4, d = 3 -> DXT1, 4 -> DXT5,
 * 1 -> BC4U, 2 -> BC5U. The encoder is deterministic and integer. A block's 16 pixels are taken
 * with coordinates clamped to the image. Colour: hi[c], lo[c] the per-channel maximum and minimum
 * (no inset), q5(v) = (31v+127)/255, q6(v) = (63v+127)/255, c0 = 565(q(hi)), c1 = 565(q(lo)); each
 * pixel takes the entry of the decoder's 4-entry palette of least squared R,G,B distance, ties to
 * the lowest index; with c0 == c1 all indices are 0 (a DXT1 block is then in 3-colour mode with
 * every pixel on entry 0, so it stays opaque). Alpha, BC4 and the halves of BC5: a0 = maximum,
 * a1 = minimum; equal: all indices 0; otherwise the nearest of the 8-entry palette by absolute
 * difference, ties to the lowest index. */
/* The file's size, 128 + the top level; 0 for arguments the writes refuse. Host only. */
size_t icx_dds_encode_bound(int width, int height, int d, int format);
/* Host pixels in, *out receives the malloc()'d file (free with icx_free). Returns an icx_dds_result. */
int icx_dds_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int format, uint8_t** out,
                           size_t* size);
/* The same file written to `path` (ICX_DDS_INTERNAL_ERR when it cannot be written). */
int icx_dds_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d, int format);
/* n writes with pixels and files resident on the device, as icx_bmp_encode_device_batch: image i's
 * pixels at d_src[i] (any alignment), its file to d_out + i*out_stride (any alignment), the file's
 * length to d_sizes[i] and an icx_dds_result to d_status[i]: INVALID_ARGUMENT for a bad size or null
 * source, TOO_LARGE (nothing of the file written, d_sizes[i] says what it needs) when it is longer
 * than out_stride. d not in 1..4, an unknown format, n < 0, n > 65535 or a null array with n > 0 ->
 * the call returns ICX_DDS_INVALID_ARGUMENT. Runs on hip_stream (NULL = the context's stream) and
 * synchronises with it. */
int icx_dds_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int format, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream);

/* ---- Netpbm read (Image::readPbm, codecs.cpp:1034-1100; PNM::load, pnm.h) ---------------------------
 * PBM, PGM, PPM and PFM. The type comes from the magic, never from a file name:
 *     P1, P4   channels 1, UBYTE: bit 0 -> 255, bit 1 -> 0 (codecs.cpp:1078-1079); maxval reads 255
 *     P2, P5   channels 1; UBYTE when maxval <= 255, USHORT (host byte order) when 256 <= maxval <= 65535
 *     P3, P6   channels 3; the same types
 *     Pf, PF   channels 1 / 3, FLOAT; maxval reads 0
 * Rows are top-down in the output. Samples are passed as stored, not rescaled to the type's range;
 * maxval is returned. Binary 16-bit samples are big-endian in the file. P4 rows are padded to whole
 * bytes. PFM rows are bottom-to-top in the file (codecs.cpp:1096-1099); a negative scale means
 * little-endian floats, a positive one big-endian floats, which are byte-swapped; the scale's
 * magnitude is not applied and the bits are otherwise copied (NaN payloads survive).
 * Header: the two magic bytes, then width, height and -- P2, P3, P5, P6 -- maxval or -- PF, Pf -- the
 * scale. A token is a run of bytes other than whitespace (space, TAB, LF, VT, FF, CR) and '#';
 * tokens are separated by any run of whitespace and comments, a comment being a '#' and everything
 * up to and including the next LF or CR (nothing need stand between the magic and the width). For
 * P4, P5, P6, PF, Pf exactly one whitespace byte follows the last token and the raster starts at
 * the next byte; for P1, P2, P3 the text starts right after the last token. Only the first image
 * is read; bytes after its raster are ignored.
 * Text rasters: outside comments a byte is a digit, whitespace, '#' or illegal. In P2 / P3 a sample
 * is a maximal run of digits (leading zeros allowed, any length); a value above maxval is
 * BAD_DATA. In P1 every '0' or '1' is one sample, separated or not, and any other digit is
 * illegal. With E the end of the last needed sample's token, or the end of the file if there are
 * too few: an illegal byte or an oversize value before E gives BAD_DATA; otherwise fewer samples
 * than width*height*channels give TRUNCATED; nothing after E is examined. A binary raster shorter
 * than it must be is TRUNCATED. A failed image yields no pixels. (Speed, not contract: a token is
 * walked by one GPU lane, a byte at a time, so a file with a very long run of leading zeros in one
 * sample decodes correctly but slowly.)
 * Deliberate deviations: the reference picks the conversion by filepath.find(".pbm") / (".pfm")
 * (a P4 file named .pnm comes back as packed bits, a P5 file named .pbm throws); it ignores maxval
 * (a 16-bit file makes it read half the raster, and an ASCII value above 255 is truncated to a
 * byte); it reads the digits "0101" of a P1 file as the number 101. */
enum icx_pnm_result {
    ICX_PNM_OK = 0,
    ICX_PNM_NOT_PNM = 1,           /* fewer than 2 bytes, or not 'P' followed by '1'-'7', 'F' or 'f' */
    ICX_PNM_BAD_HEADER = 2,        /* a missing or non-numeric token or one of more than 10 digits; zero
                                      width or height; maxval 0 or above 65535; a scale that is zero
                                      (no mantissa digit other than '0'), not finite as a float, or not of
                                      the form [+-]digits[.digits][e[+-]digits]; no whitespace byte after
                                      the last token of a binary type; the file ends inside the header */
    ICX_PNM_UNSUPPORTED = 3,       /* P7 (PAM)                                                      */
    ICX_PNM_BAD_DATA = 4,          /* text rasters: see above                                       */
    ICX_PNM_TRUNCATED = 5,         /* the raster ends first                                         */
    ICX_PNM_TOO_LARGE = 6,         /* more than 2^30 pixels; larger than the batch workspace / the output slot */
    ICX_PNM_INVALID_ARGUMENT = 7,  /* write: see below; batch read: d_out or out_stride not 16-byte aligned */
    ICX_PNM_INTERNAL_ERR = -1      /* HIP failure (see icx_last_error)                              */
};
/* `type` values: ImageCodecs::Type. */
enum icx_pnm_type { ICX_PNM_UBYTE = 0, ICX_PNM_USHORT = 1, ICX_PNM_FLOAT = 2 };
/* Header only (host): the header's values, or the code it gives (in the order NOT_PNM, UNSUPPORTED,
 * BAD_HEADER, TOO_LARGE for more than 2^30 pixels); for a binary type also TRUNCATED. The text of
 * an ASCII file is checked by the decode. Outputs are zero unless ICX_PNM_OK. */
int icx_pnm_probe(const uint8_t* data, size_t size, int* width, int* height, int* channels, int* type, int* maxval);
/* One image, host in / host out: *out receives a malloc()'d buffer of width*height*channels
 * elements of 1, 2 or 4 bytes (free with icx_free), null unless ICX_PNM_OK. A code the probe gives
 * returns without touching the GPU. */
int icx_pnm_decode(icx_ctx* ctx, const uint8_t* data, size_t size, void** out, int* width, int* height, int* channels,
                   int* type, int* maxval);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output at
 * d_out + i*out_stride, per-image status in d_status[i] and {width, height, channels, type,
 * maxval} in d_dims[5i..] (all zero for a failed image, whose slot is unspecified; nothing is
 * written outside the slots). d_out must be 16-byte aligned and out_stride a multiple of 16, else
 * the call returns ICX_PNM_INVALID_ARGUMENT. An image whose output is longer than out_stride, wider
 * than max_width or higher than max_height is TOO_LARGE; so is a text file whose needed samples do
 * not end within the workspace's 8 bytes of text per sample of a max_width x max_height RGB image.
 * Asynchronous on hip_stream (NULL = the context's stream), no host read-back. Returns ICX_PNM_OK,
 * ICX_PNM_INVALID_ARGUMENT or ICX_PNM_INTERNAL_ERR. */
typedef struct icx_pnm_batch icx_pnm_batch;
icx_pnm_batch* icx_pnm_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_pnm_batch_destroy(icx_pnm_batch* b);
int icx_pnm_batch_decode(icx_pnm_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, void* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims,
                         void* hip_stream);
/* Milliseconds per stage of the last icx_pnm_batch_decode ("parse", "locate", "text", "stream";
 * synchronises). Returns the number of stages. */
int icx_pnm_batch_stage_times(const icx_pnm_batch* b, const char** names, float* ms, int cap);

/* ---- Netpbm write (Image::writePbm, codecs.cpp:1102-1167) -----------------------------------------
 * `pixels`: width*height*d elements of `type`, rows top-down, host byte order. The headers are the
 * reference's bytes (codecs.cpp:1112, 1154, 1160):
 *     ICX_PNM_P4   "P4\n<w> <h>\n"            UBYTE, d = 1: rows packed MSB first and padded to a byte,
 *                                             bit = 1 exactly where the pixel byte is 0 (:1139)
 *     ICX_PNM_P5   "P5\n<w> <h>\n<maxval>\n"  UBYTE / USHORT, d = 1: as stored; maxval 255 / 65535
 *     ICX_PNM_P6   "P6\n<w> <h>\n<maxval>\n"  UBYTE / USHORT, d = 3 or 4: R,G,B; with d = 4 the fourth
 *                                             sample is dropped
 *     ICX_PNM_PF   "PF\n<w> <h>\n-1.0\n" (d = 3) or "Pf..." (d = 1), FLOAT: little-endian floats, rows
 *                                             bottom-to-top
 * Extensions: USHORT (written big-endian, as the format demands) and d = 4 (what read(".png")
 * returns can be written). Deviation, by evident intent: the reference writes the rows of a PFM
 * unflipped but flips on read, so its own round trip turns the picture over; here decode(encode(x))
 * is x. Any other combination of format, type and d, a width or height below 1, more than 2^30
 * pixels or a null pointer -> ICX_PNM_INVALID_ARGUMENT. Plain (ASCII) files are not written. */
enum icx_pnm_format { ICX_PNM_P4 = 4, ICX_PNM_P5 = 5, ICX_PNM_P6 = 6, ICX_PNM_PF = 8 };
/* The file's length; 0 for arguments the writes refuse. Host only. */
size_t icx_pnm_encode_bound(int width, int height, int d, int type, int format);
/* Host pixels in, *out receives the malloc()'d file (free with icx_free). Returns an icx_pnm_result. */
int icx_pnm_save_to_memory(icx_ctx* ctx, const void* pixels, int width, int height, int d, int type, int format,
                           uint8_t** out, size_t* size);
/* The same file written to `path` (ICX_PNM_INTERNAL_ERR when it cannot be written). */
int icx_pnm_save_to_file(icx_ctx* ctx, const char* path, const void* pixels, int width, int height, int d, int type,
                         int format);
/* n writes with pixels and files resident on the device: image i's pixels at d_src[i] (a host
 * array of device pointers, any alignment; widths / heights are host arrays), its file to
 * d_out + i*out_stride (any alignment), the file's length to d_sizes[i] and an icx_pnm_result to
 * d_status[i] (device arrays): INVALID_ARGUMENT for a bad size or null source (length 0),
 * TOO_LARGE (nothing of the file written, d_sizes[i] says what it needs) when it is longer than
 * out_stride. A d, type and format that do not go together, n < 0, n > 65535 (one call's limit:
 * split larger batches) or a null array with n > 0 -> the call returns ICX_PNM_INVALID_ARGUMENT.
 * Runs on hip_stream (NULL = the context's stream) and synchronises with it. */
int icx_pnm_encode_device_batch(icx_ctx* ctx, int n, const void* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int type, int format, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream);

/* ---- GIF read (Image::readGif, codecs.cpp:507-542; gd_open_gif / gd_get_frame / gd_render_frame,
 * gif.cpp:43-524) -----------------------------------------------------------------------------------
 * Output as readGif returns it for a well-formed file: Type::UBYTE, 3 channels, the logical
 * screen's width x height, rows top-down, R,G,B, the first frame only.
 * Canvas and palette: the canvas starts as the global colour table's entry `bgindex`; the frame
 * rectangle is drawn over it through the active palette (the local table if present, else the
 * global one); a pixel whose index equals the transparent index of the last graphic control
 * extension before the first image descriptor (flag bit 0 set) is skipped and leaves background.
 * Interlaced frames (descriptor bit 6) use the 8/8/4/2 row order. A palette index or bgindex at or
 * beyond its table's size gives (0,0,0) (the reference's arrays are zero there). The data ends at
 * the stop code, at the block terminator or when fw*fh pixels have been produced, whichever comes
 * first; pixels the stream did not reach hold index bgindex, drawn and skipped like any other, and
 * that is a success, as in the reference; anything after the stop code is ignored. At 4096 entries
 * the table freezes and codes stay 12 bits until a clear code. A second frame and everything after
 * it are not examined. A ';' before any image descriptor is OK with a background-only canvas.
 * Deliberate deviations:
 *  - GIF87a is accepted (the reference demands 89a).
 *  - No global table is accepted when the frame has a local one; the background is then black.
 *    With neither table the file is MALFORMED.
 *  - A stream that does not begin with a clear code is decoded as if it did (the reference uses an
 *    uninitialised length).
 *  - A code above the next free entry, or a first code after a clear that is not a literal, is
 *    BAD_DATA (the reference reads outside its table).
 *  - A string running past fw*fh is cut there (the reference writes past the frame).
 *  - A frame wider or taller than the canvas is clipped by column and row, stream rows keeping the
 *    descriptor's width and the interlace order the descriptor's height (the reference re-wraps at
 *    the clipped width).
 *  - The interlace passes of a frame lower than 5 rows are empty where they have no row (the
 *    reference's pass sizes put rows outside such a frame).
 *  - Every extension, known or unknown label, is walked as a sub-block chain; the graphic control
 *    values come from its first sub-block when that has >= 4 bytes.
 *  - A file that ends inside a header, table, extension or data sub-block is TRUNCATED (the
 *    reference ignores short reads). The data chain is read only as far as the decode goes: a
 *    file cut after the stop code, or after the sub-block that completes the frame, is OK.
 * A failed image yields no pixels. */
enum icx_gif_result {
    ICX_GIF_OK = 0,
    ICX_GIF_NOT_GIF = 1,     /* the first 6 bytes are not "GIF87a" / "GIF89a"                        */
    ICX_GIF_BAD_HEADER = 2,  /* fewer than 13 bytes; zero width or height                            */
    ICX_GIF_MALFORMED = 3,   /* a separator byte not ',' '!' ';'; fx >= width or fy >= height; no
                                palette at all                                                       */
    ICX_GIF_BAD_DATA = 4,    /* minimum code size outside 2..8; an invalid code                      */
    ICX_GIF_TRUNCATED = 5,   /* the file ends first                                                  */
    ICX_GIF_TOO_LARGE = 6,   /* larger than the batch workspace; the write: longer than out_stride   */
    ICX_GIF_INVALID_ARGUMENT = 7, /* the write only: see "GIF write" below                             */
    ICX_GIF_INTERNAL_ERR = -1 /* HIP failure (see icx_last_error)                                    */
};
/* The container walk up to the first image descriptor (host only, no GPU touched): the canvas
 * size, or the code the walk gives. The checks run in file order; a file shorter than 6 bytes is
 * BAD_HEADER. The code stream is checked by the decode. */
int icx_gif_probe(const uint8_t* data, size_t size, int* width, int* height);
/* One image, host in / host out: *out receives a malloc()'d width*height*3 byte buffer (free with
 * icx_free), null unless ICX_GIF_OK. A code the probe gives returns without touching the GPU; a
 * canvas of more than 2^30 pixels is ICX_GIF_TOO_LARGE. */
int icx_gif_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* width, int* height);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output bytes at
 * d_out + i*out_stride (out_stride >= 3*max_width*max_height), per-image status in d_status[i]
 * and {width, height, 3} in d_dims[3i..] (zero for a failed image, whose slot is unspecified).
 * A canvas wider than max_width or higher than max_height is ICX_GIF_TOO_LARGE. Asynchronous on
 * hip_stream (NULL = the context's stream), no host read-back. Returns ICX_GIF_OK or
 * ICX_GIF_INTERNAL_ERR. max_images <= 65535, max_width * max_height <= 2^30. */
typedef struct icx_gif_batch icx_gif_batch;
icx_gif_batch* icx_gif_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_gif_batch_destroy(icx_gif_batch* b);
int icx_gif_batch_decode(icx_gif_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                         const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_gif_batch_decode ("parse", "lzw", "render";
 * synchronises). Returns the number of stages. */
int icx_gif_batch_stage_times(const icx_gif_batch* b, const char** names, float* ms, int cap);

/* ---- TIFF read (Image::readTiff, codecs.cpp:1439-1484: libtiff's TIFFReadRGBAImage) ----------------
 * Output: Type::UBYTE, rows top-down, the first IFD only, d channels:
 *   Photometric 0 (MinIsWhite: a stored v gives 255 - v) and 1           d = 1
 *   Photometric 2 (RGB) with SamplesPerPixel 3                          d = 3
 *   Photometric 2 with SamplesPerPixel 4                                d = 4: the fourth sample as
 *       stored, whatever ExtraSamples says, no premultiply (a deviation from TIFFReadRGBAImage)
 *   Photometric 3 (palette)                                             d = 3: ColorMap SHORT >> 8, as
 *       libtiff and PIL do (the reference would report d = 1)
 * Accepted: classic TIFF ("II*\0" or "MM\0*"); BitsPerSample all 8, one per sample;
 * SamplesPerPixel 1, 3 or 4; PlanarConfiguration 1, or 2 when SamplesPerPixel is 1; FillOrder 1;
 * Orientation 1 or absent; SampleFormat 1 or absent; Compression 1, 5 (LZW), 8 and 32946 (zlib),
 * 32773 (PackBits); Predictor 1 or 2, where 2 is honoured only with compression 5 / 8 / 32946 (as
 * libtiff, the tag is ignored for uncompressed and PackBits data); strips (RowsPerStrip absent or
 * larger than the height: one strip) or tiles of any positive TileWidth / TileLength, clipped at
 * the right and bottom edges. BitsPerSample, ColorMap and SampleFormat are SHORT; every other tag
 * read here may be SHORT or LONG. Unknown tags are ignored, entries need not be sorted, of two
 * entries with one tag the later counts.
 * Chunks: a strip or tile must decompress to rows_in_chunk x row_bytes (a strip's last chunk has
 * fewer rows, a tile is always full size). Fewer bytes, or an invalid code, is BAD_DATA. LZW and
 * PackBits stop at that count and ignore what follows (a stream needs no EOI; a PackBits packet
 * or an LZW string running past the count is cut there). A zlib stream that inflates to MORE than
 * that count is refused as BAD_DATA (what the inflate shared with the PNG and EXR reads does; its
 * Adler-32 is checked); bytes after the zlib trailer are ignored. Uncompressed chunks may be longer
 * than needed. A PackBits header byte of -128 is a no-op; a packet that runs past the chunk's
 * input is BAD_DATA. A chunk whose bytes reach past the file is TRUNCATED. An image fails as a
 * whole, with the code of its lowest-numbered failing chunk; a failed image yields no pixels.
 * LZW (compression 5): MSB first, Clear = 256, EOI = 257, first entry 258, "early change":
 * counting codes after a Clear from 1, codes 1..254 are 9 bits, ..766 are 10, ..1790 are 11, then
 * 12. BAD_DATA: a first code that is not Clear; a first code after a Clear that is not a literal;
 * a code above the next free entry; a table that would grow past entry 4094 without a Clear (at
 * most 3838 codes may follow a Clear before the next one); EOI or the end of
 * the chunk before the last byte. Old-style LSB-first LZW (first byte 0, low bit of the second
 * set) is UNSUPPORTED.
 * The checks run in this order: the header; the IFD's entries in file order (type and count of a
 * known tag -> MALFORMED, its array outside the file -> TRUNCATED); then BAD_HEADER, UNSUPPORTED,
 * MALFORMED and TOO_LARGE as listed below; then the chunks. */
enum icx_tiff_result {
    ICX_TIFF_OK = 0,
    ICX_TIFF_NOT_TIFF = 1,    /* bad magic, or fewer than 8 bytes                                     */
    ICX_TIFF_BAD_HEADER = 2,  /* IFD offset or entry table outside the file; width or height zero or
                                 missing; no chunk offsets                                            */
    ICX_TIFF_UNSUPPORTED = 3, /* BigTIFF (magic 43); BitsPerSample not 8 (also absent: its default is
                                 1) or not one per sample; other compression, photometric, planar,
                                 orientation, fill order, sample format or predictor; SamplesPerPixel
                                 2 or above 4; old-style LZW                                          */
    ICX_TIFF_MALFORMED = 4,   /* a tag of the wrong type or count; offset and byte-count arrays of
                                 different length or not the chunk count; missing byte counts, tile
                                 size or a zero RowsPerStrip; a palette without a ColorMap of 768
                                 SHORTs; strip (273, 279) and tile (322..325) tags both present       */
    ICX_TIFF_BAD_DATA = 5,    /* as defined under Chunks and LZW                                      */
    ICX_TIFF_TRUNCATED = 6,   /* a tag array, the ColorMap or a chunk reaches past the file           */
    ICX_TIFF_TOO_LARGE = 7,   /* larger than the batch workspace; more than 4096 chunks; more than
                                 2^30 pixels (also when padded to whole chunks); a chunk of 2^31
                                 bytes or more                                                        */
    ICX_TIFF_INVALID_ARGUMENT = 8, /* the write only: see "TIFF write" below                          */
    ICX_TIFF_INTERNAL_ERR = -1 /* HIP failure (see icx_last_error)                                    */
};
/* The IFD walk (host only, no GPU touched): width, height and channels, or the code the walk gives
 * (every code above except BAD_DATA and a chunk's TRUNCATED / UNSUPPORTED, which the decode finds). */
int icx_tiff_probe(const uint8_t* data, size_t size, int* width, int* height, int* channels);
/* One image, host in / host out: *out receives a malloc()'d width*height*channels byte buffer
 * (free with icx_free), null unless ICX_TIFF_OK. A code the probe gives returns without touching
 * the GPU. */
int icx_tiff_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* width, int* height,
                    int* channels);
/* Device-resident batch: image i = d_data[d_offsets[i] .. + d_sizes[i]), output bytes at
 * d_out + i*out_stride (out_stride >= 4*max_width*max_height), per-image status in d_status[i]
 * and {width, height, channels} in d_dims[3i..] (zero for a failed image, whose slot is
 * unspecified). Asynchronous on hip_stream (NULL = the context's stream), no host read-back.
 * Returns ICX_TIFF_OK or ICX_TIFF_INTERNAL_ERR. max_images <= 65535, max_width * max_height <= 2^30.
 * Scratch: decompressed chunks wait in a slot of S = round16(4*max_width*max_height) +
 * 16*min(4096, max_width*max_height) bytes per image, each chunk in a room of its full size
 * (TileWidth*TileLength*SamplesPerPixel, or RowsPerStrip*width*SamplesPerPixel with RowsPerStrip
 * clamped to the height) rounded up to 16 bytes. Padded tiles can exceed width*height*channels: an
 * image wider than max_width, higher than max_height, or whose rooms together exceed S is
 * ICX_TIFF_TOO_LARGE (whatever its compression). */
typedef struct icx_tiff_batch icx_tiff_batch;
icx_tiff_batch* icx_tiff_batch_create(icx_ctx* ctx, int max_images, int max_width, int max_height);
void icx_tiff_batch_destroy(icx_tiff_batch* b);
int icx_tiff_batch_decode(icx_tiff_batch* b, int n, const uint8_t* d_data, const uint64_t* d_offsets,
                          const uint64_t* d_sizes, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                          int32_t* d_dims, void* hip_stream);
/* Milliseconds per stage of the last icx_tiff_batch_decode ("parse", "unpack", "render";
 * synchronises). Returns the number of stages. */
int icx_tiff_batch_stage_times(const icx_tiff_batch* b, const char** names, float* ms, int cap);

/* ---- TIFF write (Image::writeTiff, codecs.cpp:1485-1513: libtiff, one ADOBE_DEFLATE strip) ---------
 * pixels: width*height*d bytes, rows top-down, d = 1 (grey), 3 (R,G,B) or 4 (R,G,B,A): the shapes the
 * read returns. A file written here reads back, through icx_tiff_decode, to the same d and bytes.
 * compression: ICX_TIFF_COMPRESSION_NONE (1), _LZW (5), _DEFLATE (8, the reference's) or _PACKBITS
 * (32773). predictor: 1, or 2 with LZW or Deflate only (the read, like libtiff, ignores the tag
 * elsewhere). rows_per_strip: 0 is the image height (one strip, the reference's layout); a positive
 * value is clamped to the height. ICX_TIFF_INVALID_ARGUMENT (and a bound of 0): any other
 * compression, predictor or combination; rows_per_strip < 0; more than 4096 strips; d outside
 * {1, 3, 4}; width or height < 1; more than 2^30 pixels; a strip of 2^31 bytes or more; a null
 * pointer; a worst-case file of 2^32 bytes or more (the offsets are 32-bit).
 * File layout, little-endian ("II*\0"): the strips' data from offset 8, in order, each strip at an
 * even offset (one zero byte after a strip of odd length); then the out-of-line arrays in tag
 * order, each at an even offset: BitsPerSample when d >= 3, StripOffsets and StripByteCounts when
 * there is more than one strip; then the IFD at the next even offset: the entry count, the entries
 * sorted by tag, next-IFD 0. Nothing follows the IFD. Entries: 256 ImageWidth LONG; 257
 * ImageLength LONG; 258 BitsPerSample SHORT x d, all 8; 259 Compression SHORT; 262 Photometric
 * SHORT, 1 for d = 1 and 2 otherwise (the reference sets RGB for every d); 273 StripOffsets LONG x
 * n; 277 SamplesPerPixel SHORT; 278 RowsPerStrip LONG, the clamped value; 279 StripByteCounts LONG
 * x n; 284 PlanarConfiguration SHORT 1; 317 Predictor SHORT 2, only when predictor 2 was asked
 * for; 338 ExtraSamples SHORT 2 (unassociated alpha), only when d = 4.
 * Strip payloads: the raw bytes of strip k are its rows x width*d; with predictor 2 every sample
 * after the first pixel of a row is stored minus the sample d bytes before it, mod 256.
 *   None      the raw bytes.
 *   PackBits  rows are coded row by row, no packet crosses a row. Each maximal run of equal bytes
 *             is cut into pieces of 128 from its start; a piece of 3 or more bytes is a repeat
 *             packet (257 - n, the byte); everything else joins the neighbouring literal stretch;
 *             literal stretches are cut into packets of 128 from their start (n - 1, the bytes).
 *   LZW       libtiff's stream: MSB first, early change (widths as under the read), a leading
 *             Clear, greedy longest match, a Clear after the 3836th code since the last Clear, EOI,
 *             then zero bits to the byte. One stream per strip.
 *   Deflate   an RFC 1950 stream of our own (78 01, dynamic blocks, big-endian Adler-32) that
 *             inflates to exactly the strip's (differenced) bytes: as with PNG and EXR only the
 *             tokenisation is ours. Matches never cross a multiple of 4096 bytes of the strip; a
 *             block covers at most 65536 bytes.
 * icx_tiff_encode_bound: an upper bound of the file's size (0: refused arguments): the layout
 * above with each strip at its payload's bound -- none: exact; PackBits: n + ceil(n / 128) per row
 * of n bytes; LZW: 12 bits per byte, per Clear and for the EOI; Deflate: 9 bits per byte (a
 * Huffman-optimal code costs no more than a flat 9-bit code over 286 symbols and a flat 5-bit
 * distance code, under which no token the parse keeps costs more than 9 bits a byte) times
 * 1 + 1/1024 for the length limiter (its documented worst ratio is 1.000036), 384 bytes and an
 * end-of-block code per block, and 6 bytes of zlib framing. The proof is in icx_tiffw_core.h. */
enum icx_tiff_compression {
    ICX_TIFF_COMPRESSION_NONE = 1,
    ICX_TIFF_COMPRESSION_LZW = 5,
    ICX_TIFF_COMPRESSION_DEFLATE = 8,
    ICX_TIFF_COMPRESSION_PACKBITS = 32773
};
size_t icx_tiff_encode_bound(int width, int height, int d, int compression, int predictor, int rows_per_strip);
/* One image, host in / host out: *out receives the file (malloc()'d, free with icx_free). */
int icx_tiff_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int compression,
                            int predictor, int rows_per_strip, uint8_t** out, size_t* size);
/* The same bytes written to path; ICX_TIFF_INTERNAL_ERR when the file cannot be written. */
int icx_tiff_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d,
                          int compression, int predictor, int rows_per_strip);
/* Device-resident batch: image i's pixels at d_src[i] (device, any alignment), its file at
 * d_out + i*out_stride (any alignment), its size in d_sizes[i] and its code in d_status[i]: OK;
 * INVALID_ARGUMENT (a null d_src[i] or a refused size; size 0); ICX_TIFF_TOO_LARGE when the file is
 * longer than out_stride (nothing of it is written; d_sizes[i] says what it needs). The call
 * returns ICX_TIFF_INVALID_ARGUMENT for n < 0, n > 65535, a refused d / compression / predictor /
 * rows_per_strip or a null array with n > 0, otherwise ICX_TIFF_OK or ICX_TIFF_INTERNAL_ERR. All
 * strips of all images go through each kernel in one launch; the call synchronises hip_stream
 * (NULL = the context's stream) and reads nothing back. */
int icx_tiff_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                 const int32_t* heights, int d, int compression, int predictor, int rows_per_strip,
                                 uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status,
                                 void* hip_stream);

/* ---- GIF write (Image::writeGif, codecs.cpp:544-594) ------------------------------------------------
 * The reference pairs a grey-ramp palette with channel-planar bytes; the file written here is a
 * contract of its own: one GIF89a frame, a global colour table, no extensions, not interlaced. A
 * file written here reads back, through icx_gif_decode, to the table's colours at the pixels'
 * indices: the pixels themselves when they have 256 colours or fewer.
 * pixels: width*height*d bytes, rows top-down, d = 1 (grey: v is the colour v,v,v), 3 (R,G,B) or 4
 * (R,G,B,A: alpha is ignored, as the read returns three channels). width, height: 1..65535.
 * ICX_GIF_INVALID_ARGUMENT (and a bound of 0): a width, height, d, dither, palette_mode or
 * segment_pixels outside what is stated here; a null pointer; more than 2^30 pixels; more than
 * 65535 images.
 * Palette, one rule for every d:
 *   exact  the image has n <= 256 distinct colours: the table holds them in ascending order of
 *          R<<16 | G<<8 | B, a pixel's index is its colour's rank (so the table does not depend on
 *          the order of the pixels). Table bits tb = max(1, ceil(log2 n)), 2^tb entries, those from
 *          n on 0,0,0; minimum code size m = max(2, tb).
 *   cube   more than 256 distinct colours, or palette_mode = ICX_GIF_PALETTE_CUBE: 6 x 7 x 6 levels
 *          of R, G, B, 252 entries, entries 252..255 0,0,0, tb = 8, m = 8. Level k of L is the value
 *          (255*k + (L-1)/2) / (L-1) in integer arithmetic (0,51,..,255 and 0,43,85,128,170,213,255).
 *          A channel value c has level k = (32*c*(L-1) + 255*T) / 8160 in integer arithmetic, with
 *          T = 16 (round half up) without dithering and T = 2*B4[y&3][x&3] + 1 with ordered
 *          dithering, B4 = {{0,8,2,10},{12,4,14,6},{3,11,1,9},{15,7,13,5}}. Index (kr*7 + kg)*6 + kb.
 * Options: segment_pixels: 0 is the default (65536), -1 one segment for the whole image, any other
 * value must be >= 64 (a value >= width*height is one segment). dither: 0 or 1, used only where the
 * cube is. palette_mode: ICX_GIF_PALETTE_AUTO (the rule above) or ICX_GIF_PALETTE_CUBE.
 * Code stream: LSB first; Clear = 2^m, stop = Clear + 1, first free entry Clear + 2; codes are m + 1
 * bits wide after a Clear and one bit wider once the decoder's next free entry equals 2^width, up
 * to 12. The stream is a leading Clear; then for each segment of segment_pixels consecutive indices
 * (row-major, the last one shorter) the greedy longest-match codes of that segment alone, with a
 * Clear immediately after the code whose emission adds entry 4095 (the dictionary restarts); after
 * a segment's last pending code a Clear, after the last segment's the stop code; then zero bits to
 * the byte. A Clear that ends a segment has the width the decoder holds there, so a segment's bit
 * string depends on its own indices and m only: segments are coded independently and their bit
 * strings concatenated. Cutting costs compression: a dictionary restarts at every segment.
 * Container: "GIF89a"; width, height (little-endian), flags 0x80 | (tb-1)<<4 | (tb-1), background
 * 0, aspect 0; the table; ',' 0 0 0 0 width height flags 0; the byte m; the payload in sub-blocks of
 * 255 bytes, the last one shorter (no empty sub-block when the payload is a multiple of 255); a
 * zero terminator; ';'. Nothing follows.
 * icx_gif_encode_bound: an upper bound of the file's size (0: refused arguments), independent of
 * the content and of d: at most N + nseg + 1 + floor(N/3838) codes (one per pixel, a Clear or stop
 * per segment, the leading Clear, a table-full Clear per 3838 codes at least) of 12 bits, the
 * sub-block length bytes, 13 + 768 + 10 + 1 bytes of header, table, descriptor and code size, the
 * terminator and the trailer. The proof is in icx_gifw_core.h. */
enum icx_gif_palette_mode { ICX_GIF_PALETTE_AUTO = 0, ICX_GIF_PALETTE_CUBE = 1 };
size_t icx_gif_encode_bound(int width, int height, int segment_pixels);
/* One image, host in / host out: *out receives the file (malloc()'d, free with icx_free). */
int icx_gif_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int segment_pixels,
                           int dither, int palette_mode, uint8_t** out, size_t* size);
/* The same bytes written to path; ICX_GIF_INTERNAL_ERR when the file cannot be written. */
int icx_gif_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d,
                         int segment_pixels, int dither, int palette_mode);
/* Device-resident batch: image i's pixels at d_src[i] (device, any alignment), its file at
 * d_out + i*out_stride (any alignment), its size in d_sizes[i] and its code in d_status[i]: OK;
 * INVALID_ARGUMENT (a null d_src[i] or a refused size; size 0); ICX_GIF_TOO_LARGE when the file is
 * longer than out_stride (nothing of it is written; d_sizes[i] says what it needs). The call
 * returns ICX_GIF_INVALID_ARGUMENT for n < 0, n > 65535, a refused d / segment_pixels / dither /
 * palette_mode or a null array with n > 0, otherwise ICX_GIF_OK or ICX_GIF_INTERNAL_ERR. All images
 * go through each kernel in one launch; the palette mode, m and every size stay on the device; the
 * call synchronises hip_stream (NULL = the context's stream) and reads nothing back. */
int icx_gif_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int segment_pixels, int dither, int palette_mode,
                                uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status,
                                void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ICX_H */
