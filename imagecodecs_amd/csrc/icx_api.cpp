// icx_api.cpp -- host side of libicx.so: the C ABI declared in include/icx.h.
//
// Contexts own a HIP stream and the NanoJPEG-style single-image state; batches own the
// device workspace of one image group. No CPU decode path exists: every decode runs the
// HIP kernels in icx_decode.hip, and a missing/unusable GPU is reported as an error.
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../../include/icx.h"
#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_step.h"
#include "icx_tga_core.h"
#include "icx_bmp_core.h"
#include "icx_pnm_core.h"
#include "icx_dds_core.h"
#include "icx_hdrw_core.h"
#include "icx_gif_core.h"
#include "icx_tiffw_core.h"
#include "icx_gifw_core.h"

using namespace icx;

struct icx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // njDecode-style state (jpeg_dec.h:313-330 equivalent, per context)
    std::vector<uint8_t> nj_image;
    int nj_w = 0, nj_h = 0, nj_color = 0, nj_size = 0;
    icx_batch* single = nullptr;  // cached workspace for one-image calls
    ExrWs* exr = nullptr;  // grow-only EXR read buffers (icx_exr.hip)
    ExrwWs* exrw = nullptr;  // grow-only EXR write buffers (icx_exrw.hip)
    TgawWs* tgaw = nullptr;  // grow-only Targa write buffers (icx_tga.hip)
    BmpwWs* bmpw = nullptr;  // grow-only BMP write buffers (icx_bmp.hip)
    HdrwWs* hdrw = nullptr;  // grow-only Radiance write buffers (icx_hdrw.hip)
    PnmwWs* pnmw = nullptr;  // grow-only Netpbm write buffers (icx_pnm.hip)
    DdswWs* ddsw = nullptr;  // grow-only DDS write buffers (icx_dds.hip)
    TiffwWs* tiffw = nullptr;  // grow-only TIFF write buffers (icx_tiffw.hip)
    GifwWs* gifw = nullptr;  // grow-only GIF write buffers (icx_gifw.hip)
};

struct EventHook;

// Up to kMaxPipes decode pipelines per batch, each a workspace + a stream: consecutive groups of
// a call alternate between them, so one group's entropy kernels (latency/LDS-bound) run beside
// another group's IDCT/convert (memory-bound) instead of after them.
#ifndef ICX_MAX_PIPES  // (timing experiments: more pipelines)
#define ICX_MAX_PIPES 2
#endif
constexpr int kMaxPipes = ICX_MAX_PIPES;
struct icx_batch {
    icx_ctx* ctx = nullptr;
    int max_images = 0;
    int pipes = 1;
    GroupWs ws[kMaxPipes];
    Blocks mem[kMaxPipes];            // the device and pinned memory ws[p] points into
    hipStream_t pst[kMaxPipes] = {};  // pst[0] unused: pipe 0 runs on the caller's stream
    hipEvent_t fork = nullptr, join[kMaxPipes] = {};
    std::vector<hipEvent_t> front_done;  // per group of a call: its front half has run
    int min_groups = 1;                  // a call is cut into at least this many groups
    bool stagger = false;                // group g's front waits for group g-1's front (ICX_STAGGER=1; measured slower)
    Buf<uint8_t> d_hin;  // staging for icx_jpeg_batch_decode_host
    hipEvent_t done = nullptr;      // recorded after the last decode call's work (path_stats waits on it)
    bool decoded = false;
    std::unique_ptr<EventHook> hook;
};

static std::string g_create_err;

static thread_local char g_msg[512];

#define ICX_HIP(ctx, call, ret)                                                             \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (void)hipGetLastError(); /* reported here: not left for the caller's next check */ \
            std::snprintf(g_msg, sizeof g_msg, "%s failed: %s", #call, hipGetErrorString(e_)); \
            if (ctx) (ctx)->err = g_msg;                                                    \
            return ret;                                                                     \
        }                                                                                   \
    } while (0)
// The same for an allocation through icx_mem.h (`ok` false: HIP's error is still pending).
#define ICX_ALLOC(ctx, ok, ret)                                                                              \
    do {                                                                                                     \
        if (!(ok)) {                                                                                         \
            std::snprintf(g_msg, sizeof g_msg, "%s failed: %s", #ok, hipGetErrorString(hipGetLastError())); \
            if (ctx) (ctx)->err = g_msg;                                                                     \
            return ret;                                                                                      \
        }                                                                                                    \
    } while (0)

// Brackets every pipeline stage with HIP events on the launch stream, and with a roctx range on
// the host (the launch side: `rocprofv3 --marker-trace` shows which stage enqueued which kernels).
// One roctx range per API call, around every stage's range.
struct RoctxRange {
    explicit RoctxRange(const char* m) { (void)roctxRangePushA(m); }
    ~RoctxRange() { (void)roctxRangePop(); }
};
static const char* const kRangeNames[kStCount] = {"icx:parse", "icx:unstuff", "icx:entropy", "icx:write",
                                                  "icx:idct", "icx:upsample", "icx:convert"};
struct EventHook : StageHook {
    struct Rec { Stage s; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
    void reset() { recs.clear(); used = 0; }
    void begin(Stage s, hipStream_t st) override {
        (void)roctxRangePushA(kRangeNames[s]);
        hipEvent_t a = get(), b = get();
        if (!a || !b) return;
        (void)hipEventRecord(a, st);
        recs.push_back({s, a, b});
    }
    void end(Stage s, hipStream_t st) override {
        (void)roctxRangePop();
        for (auto it = recs.rbegin(); it != recs.rend(); ++it)
            if (it->s == s) { (void)hipEventRecord(it->b, st); return; }
    }
    // ms per stage over the records (waits for each; a failed wait or read is dropped, and its
    // error not left for the caller's next check)
    void sum(float acc[kStCount]) const {
        std::fill(acc, acc + kStCount, 0.f);
        for (auto& r : recs) {
            float t = 0;
            if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) acc[r.s] += t;
            else (void)hipGetLastError();
        }
    }
    ~EventHook() override {
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// ------------------------------------------- the host layer the read batches share
// Every read format but JPEG and EXR has the same host side: a batch {ctx, ws, mem, hook}, its
// create / destroy / decode / stage_times, and a one-shot decode through a batch of one. A ReadFmt
// says what differs: the workspace, the codes, the entry names in messages and roctx ranges, the
// stages, the limits create refuses, the workspace allocation, the launcher and what decode asks
// of d_out and out_stride. A new format writes one such struct and entries of a few lines.
namespace {  // (this file's own types: none of them is exported)

template <class F>
struct ReadBatch {
    icx_ctx* ctx = nullptr;
    typename F::Ws ws;
    Blocks mem;  // the device memory ws points into
    std::unique_ptr<EventHook> hook;
};

struct ReadFmtDefaults {
    static constexpr int kStridePx = 4;  // out_stride is at least this x max_w x max_h (0: no floor)
    static int out_refused(icx_ctx*, const void*, uint64_t) { return 0; }  // d_out / out_stride alignment
};

struct HdrFmt : ReadFmtDefaults {
    using Ws = HdrWs;
    using Px = float;
    using Batch = icx_hdr_batch;
    static constexpr int kOk = ICX_HDR_OK, kInternal = ICX_HDR_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_hdr_batch_create", *kDecode = "icx_hdr_batch_decode", *kOne = "icx_hdr_decode";
    static constexpr Stage kOrder[] = {kStParse, kStUnstuff, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "locate", "unpack", "convert"};
    static bool over_limit(int, int, int) { return false; }
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h) { return hdr_ws_alloc(ws, mem, n, w, h); }
    static constexpr auto launch = &launch_hdr_decode;
};

struct PngFmt : ReadFmtDefaults {
    using Ws = PngdWs;
    using Px = uint8_t;
    using Batch = icx_png_batch;
    static constexpr int kOk = ICX_PNGR_OK, kInternal = ICX_PNGR_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_png_batch_create", *kDecode = "icx_png_batch_decode", *kOne = "icx_png_decode";
    static constexpr Stage kOrder[] = {kStParse, kStUnstuff, kStEntropy, kStIdct, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "gather", "inflate", "unfilter", "expand"};
    // (images are one grid dimension; no image the walk accepts is larger than the pixel limit)
    static bool over_limit(int n, int w, int h) { return n > 65535 || w > 0x1000000 || h > 0x1000000; }
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h) { return pngd_ws_alloc(ws, mem, n, w, h); }
    static constexpr auto launch = &launch_pngd_decode;
    static int out_refused(icx_ctx* ctx, const void* d_out, uint64_t out_stride) {
        if (!(reinterpret_cast<uintptr_t>(d_out) & 3) && !(out_stride & 3)) return 0;
        ctx->err = "icx_png_batch_decode: d_out and out_stride must be multiples of 4";
        return ICX_PNGR_INTERNAL_ERR;
    }
};

struct TgaFmt : ReadFmtDefaults {
    using Ws = TgaWs;
    using Px = uint8_t;
    using Batch = icx_tga_batch;
    static constexpr int kOk = ICX_TGA_OK, kInternal = ICX_TGA_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_tga_batch_create", *kDecode = "icx_tga_batch_decode", *kOne = "icx_tga_decode";
    static constexpr Stage kOrder[] = {kStParse, kStUnstuff, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "locate", "expand", "raw"};
    // (images are one grid dimension; pixel indices are 32-bit in the tile tables)
    static bool over_limit(int n, int w, int h, bool) {
        return n > 65535 || w > 65535 || h > 65535 || (int64_t)w * h > ((int64_t)1 << 30);
    }
    // rle false: a workspace for raw files only (no tile tables, no RLE kernels launched).
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h, bool rle) { return tga_ws_alloc(ws, mem, n, w, h, rle); }
    static constexpr auto launch = &launch_tga_decode;
};

struct BmpFmt : ReadFmtDefaults {
    using Ws = BmpWs;
    using Px = uint8_t;
    using Batch = icx_bmp_batch;
    static constexpr int kOk = ICX_BMP_OK, kInternal = ICX_BMP_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_bmp_batch_create", *kDecode = "icx_bmp_batch_decode", *kOne = "icx_bmp_decode";
    static constexpr Stage kOrder[] = {kStParse, kStUnstuff, kStWrite, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "locate", "fill", "expand", "raw"};
    // (images are one grid dimension, a stream's tiles another)
    static bool over_limit(int n, int w, int h, int64_t stream_cap) {
        return n > 65535 || (int64_t)w * h > ((int64_t)1 << 30) || stream_cap < 0 || stream_cap > ((int64_t)1 << 42);
    }
    // stream_cap: the run-length stream bytes per image the tile tables cover; 0: a workspace for
    // raw files only (no tile tables, no RLE kernels launched).
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h, int64_t stream_cap) {
        return bmp_ws_alloc(ws, mem, n, w, h, stream_cap);
    }
    static constexpr auto launch = &launch_bmp_decode;
};

struct PnmFmt : ReadFmtDefaults {
    using Ws = PnmWs;
    using Px = uint8_t;
    using Batch = icx_pnm_batch;
    static constexpr int kOk = ICX_PNM_OK, kInternal = ICX_PNM_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_pnm_batch_create", *kDecode = "icx_pnm_batch_decode", *kOne = "icx_pnm_decode";
    static constexpr Stage kOrder[] = {kStParse, kStUnstuff, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "locate", "text", "stream"};
    // (images are one grid dimension)
    static bool over_limit(int n, int w, int h, int64_t) { return n > 65535 || (int64_t)w * h > ((int64_t)1 << 30); }
    // tiles_cap: tiles of raster text per image (0: a workspace for binary files only).
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h, int64_t tiles_cap) {
        return pnm_ws_alloc(ws, mem, n, w, h, tiles_cap);
    }
    static constexpr auto launch = &launch_pnm_decode;
    static constexpr int kStridePx = 0;  // (a slot holds what the caller sized it for: TOO_LARGE per image)
    static int out_refused(icx_ctx*, const void* d_out, uint64_t out_stride) {  // (sets no message)
        return (reinterpret_cast<uintptr_t>(d_out) & 15) || (out_stride & 15) ? ICX_PNM_INVALID_ARGUMENT : 0;
    }
};

struct DdsFmt : ReadFmtDefaults {
    using Ws = DdsWs;
    using Px = uint8_t;
    using Batch = icx_dds_batch;
    static constexpr int kOk = ICX_DDS_OK, kInternal = ICX_DDS_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_dds_batch_create", *kDecode = "icx_dds_batch_decode", *kOne = "icx_dds_decode";
    static constexpr Stage kOrder[] = {kStParse, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "blocks", "raw"};
    // (images are one grid dimension)
    static bool over_limit(int n, int w, int h) { return n > 65535 || (int64_t)w * h > ((int64_t)1 << 30); }
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h) { return dds_ws_alloc(ws, mem, n, w, h); }
    static constexpr auto launch = &launch_dds_decode;
    static constexpr int kStridePx = 0;  // (a slot holds what the caller sized it for: TOO_LARGE per image)
    static int out_refused(icx_ctx*, const void* d_out, uint64_t out_stride) {  // (sets no message)
        return (reinterpret_cast<uintptr_t>(d_out) & 15) || (out_stride & 15) ? ICX_DDS_INVALID_ARGUMENT : 0;
    }
};

struct GifFmt : ReadFmtDefaults {
    using Ws = GifWs;
    using Px = uint8_t;
    using Batch = icx_gif_batch;
    static constexpr int kOk = ICX_GIF_OK, kInternal = ICX_GIF_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_gif_batch_create", *kDecode = "icx_gif_batch_decode", *kOne = "icx_gif_decode";
    static constexpr Stage kOrder[] = {kStParse, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "lzw", "render"};
    // (images are one grid dimension; pixel indices are 32-bit in the index plane)
    static bool over_limit(int n, int w, int h) {
        return n > 65535 || w > 65535 || h > 65535 || (int64_t)w * h > ((int64_t)1 << 30);
    }
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx*, int n, int w, int h) { return gif_ws_alloc(ws, mem, n, w, h); }
    static constexpr auto launch = &launch_gif_decode;
    static constexpr int kStridePx = 3;
};

struct TiffFmt : ReadFmtDefaults {
    using Ws = TiffWs;
    using Px = uint8_t;
    using Batch = icx_tiff_batch;
    static constexpr int kOk = ICX_TIFF_OK, kInternal = ICX_TIFF_INTERNAL_ERR;
    static constexpr const char *kCreate = "icx_tiff_batch_create", *kDecode = "icx_tiff_batch_decode", *kOne = "icx_tiff_decode";
    static constexpr Stage kOrder[] = {kStParse, kStEntropy, kStConvert};
    static constexpr const char* kLabel[] = {"parse", "unpack", "render"};
    // (images are one grid dimension; byte positions inside a chunk are 32-bit)
    static bool over_limit(int n, int w, int h) { return n > 65535 || (int64_t)w * h > ((int64_t)1 << 30); }
    static bool alloc(Ws& ws, Blocks& mem, icx_ctx* ctx, int n, int w, int h) {
        return tiff_ws_alloc(ws, mem, ctx->device, n, w, h);
    }
    static constexpr auto launch = &launch_tiff_decode;
};

// The device side of a one-shot decode through a batch of one: the file, its {offset, size}, the
// pixels and the result record {status, dims...}. A one-shot declares its batch before this, so
// these buffers are freed first, then the batch.
struct OneShot {
    Buf<uint8_t> in, out;
    Buf<uint64_t> meta;
    Buf<int32_t> res;
    int32_t rec[6] = {0, 0, 0, 0, 0, 0};
};

}  // namespace


struct icx_hdr_batch : ReadBatch<HdrFmt> {
    hipEvent_t done = nullptr;  // recorded after the last decode call's work (locate_stats waits on it)
    int last_n = 0;             // images of that call
    ~icx_hdr_batch() {
        if (done) (void)hipEventDestroy(done);
    }
};
struct icx_png_batch : ReadBatch<PngFmt> {};
struct icx_tga_batch : ReadBatch<TgaFmt> {};
struct icx_bmp_batch : ReadBatch<BmpFmt> {};
struct icx_pnm_batch : ReadBatch<PnmFmt> {};
struct icx_dds_batch : ReadBatch<DdsFmt> {};
struct icx_gif_batch : ReadBatch<GifFmt> {};
struct icx_tiff_batch : ReadBatch<TiffFmt> {};

// `extra`: what the format's workspace takes beyond the sizes (TgaFmt, BmpFmt, PnmFmt).
template <class F, class... Extra>
static typename F::Batch* read_batch_new(icx_ctx* ctx, int max_images, int max_w, int max_h, Extra... extra) {
    if (!ctx || max_images <= 0 || max_w <= 0 || max_h <= 0 || F::over_limit(max_images, max_w, max_h, extra...)) {
        if (ctx) ctx->err = std::string(F::kCreate) + ": bad arguments";
        return nullptr;
    }
    ICX_HIP(ctx, hipSetDevice(ctx->device), nullptr);
    auto* b = new typename F::Batch();
    b->ctx = ctx;
    b->hook = std::make_unique<EventHook>();
    if (!F::alloc(b->ws, b->mem, ctx, max_images, max_w, max_h, extra...)) {
        ctx->err = std::string(F::kCreate) + ": out of device memory: " + hipGetErrorString(hipGetLastError());
        delete b;
        return nullptr;
    }
    return b;
}

template <class B>
static void read_batch_destroy(B* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    delete b;
}

// The checks in this order: n, nothing to do, null pointers, the stride floor, the format's alignment.
template <class F, class Out>
static int read_batch_decode(typename F::Batch* b, int n, const uint8_t* d_data, const uint64_t* d_off,
                             const uint64_t* d_size, Out* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims,
                             void* stream) {
    if (!b) return F::kInternal;
    icx_ctx* ctx = b->ctx;
    if (n < 0 || n > b->ws.max_images) { ctx->err = std::string(F::kDecode) + ": n exceeds batch capacity"; return F::kInternal; }
    if (n == 0) return F::kOk;
    if (!d_data || !d_off || !d_size || !d_out || !d_status || !d_dims) { ctx->err = "null pointer"; return F::kInternal; }
    if (out_stride < (uint64_t)F::kStridePx * b->ws.max_w * b->ws.max_h) { ctx->err = std::string(F::kDecode) + ": out_stride too small"; return F::kInternal; }
    if (const int rc = F::out_refused(ctx, d_out, out_stride)) return rc;
    ICX_HIP(ctx, hipSetDevice(ctx->device), F::kInternal);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const RoctxRange range(F::kDecode);
    b->hook->reset();
    F::launch(b->ws, n, d_data, d_off, d_size, static_cast<typename F::Px*>(d_out), out_stride, d_status, d_dims, st, b->hook.get());
    ICX_HIP(ctx, hipGetLastError(), F::kInternal);
    return F::kOk;
}

template <int K>
static int read_stage_times(const EventHook& hook, const Stage (&order)[K], const char* const (&label)[K], const char** names,
                            float* ms, int cap) {
    float acc[kStCount];
    hook.sum(acc);
    for (int k = 0; k < K && k < cap; ++k) {
        if (names) names[k] = label[k];
        if (ms) ms[k] = acc[order[k]];
    }
    return K;
}

// A probe's outputs: what it found when it returned `ok`, else zero.
static int probe_out(int rc, int ok, int* w, int ww, int* h, int hh, int* d = nullptr, int dd = 0) {
    if (w) *w = rc == ok ? ww : 0;
    if (h) *h = rc == ok ? hh : 0;
    if (d) *d = rc == ok ? dd : 0;
    return rc;
}

static void zero_out(std::initializer_list<int*> outs) {
    for (int* p : outs)
        if (p) *p = 0;
}

// Uploads the file, runs launch(io, st) and downloads rec_ints ints of the record. False: a HIP call failed.
template <class Launch>
static bool one_shot_run(icx_ctx* ctx, OneShot& io, const uint8_t* data, size_t size, size_t in_cap, uint64_t out_bytes,
                         int rec_ints, Launch launch) {
    const uint64_t meta[2] = {0, (uint64_t)size};
    hipStream_t st = ctx->stream;
    return io.in.reserve(in_cap) && io.out.reserve(out_bytes) && io.meta.reserve(16) && io.res.reserve(4 * rec_ints) &&
           hipMemcpyAsync(io.in.p, data, size, hipMemcpyHostToDevice, st) == hipSuccess &&
           hipMemcpyAsync(io.meta.p, meta, 16, hipMemcpyHostToDevice, st) == hipSuccess && launch(io, st) &&
           hipMemcpyAsync(io.rec, io.res.p, 4 * rec_ints, hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess;
}

// The launcher itself with a null hook, for a batch of one whose slot is `stride`.
template <class F>
static auto launch_direct(const typename F::Ws& ws, uint64_t stride) {
    return [&ws, stride](OneShot& io, hipStream_t st) {
        F::launch(ws, 1, io.in.p, io.meta.p, io.meta.p + 1, io.out.p, stride, io.res.p, io.res.p + 1, st, nullptr);
        return hipGetLastError() == hipSuccess;
    };
}

// Hands the caller `nbytes` of pixels and the record's dims; returns the record's status.
template <class F, class T>
static int one_shot_take(icx_ctx* ctx, const OneShot& io, uint64_t nbytes, T** out, std::initializer_list<int*> dims) {
    void* hostp = std::malloc(nbytes);
    if (!hostp || hipMemcpy(hostp, io.out.p, nbytes, hipMemcpyDeviceToHost) != hipSuccess) {
        std::free(hostp);
        ctx->err = std::string(F::kOne) + ": host allocation or copy failed";
        return F::kInternal;
    }
    *out = static_cast<T*>(hostp);
    const int32_t* r = io.rec + 1;
    for (int* p : dims) {
        if (p) *p = *r;
        ++r;
    }
    return io.rec[0];
}

// The one-shot of the byte formats after the probe: pixels only for an image that decoded.
template <class F, class Launch>
static int read_one(icx_ctx* ctx, const uint8_t* data, size_t size, uint64_t nbytes, uint8_t** out,
                    std::initializer_list<int*> dims, Launch launch) {
    OneShot io;
    if (!one_shot_run(ctx, io, data, size, size, nbytes, 4, launch)) {
        if (ctx->err.empty()) ctx->err = std::string(F::kOne) + ": HIP failure";
        return F::kInternal;
    }
    return io.rec[0] == F::kOk ? one_shot_take<F>(ctx, io, nbytes, out, dims) : io.rec[0];
}

// ------------------------------------------- the host layer the writers share (tga, bmp, pnm, hdr)
// The guarded part of encode_device_batch: encode(ws, err) returns 0, or fails with what `err` says;
// nothing may cross the C ABI, so a host allocation failure is an internal error too.
template <class Ws, class Encode>
static int encode_batch_guarded(icx_ctx* ctx, const char* entry, Ws*& ws, Ws* (*create)(), int ok, int internal,
                                Encode encode) {
    ICX_HIP(ctx, hipSetDevice(ctx->device), internal);
    const RoctxRange range(entry);
    std::string err;
    int rc;
    try {
        if (!ws) ws = create();
        rc = encode(*ws, err);
    } catch (const std::exception& e) {
        err = std::string(entry) + ": " + e.what();
        rc = -1;
    }
    if (rc != 0) {
        ctx->err = err.empty() ? std::string(entry) + ": HIP failure" : err;
        return internal;
    }
    return ok;
}

// save_to_memory once the arguments are checked: uploads `nbytes` of pixels, has
// encode(&src, d_file, d_size, d_status, st) write one file of at most `bound` bytes through the
// batch entry, reads {size, status} and hands the caller a copy of the file.
template <class T, class Encode>
static int save_one(icx_ctx* ctx, const char* entry, const void* pixels, uint64_t nbytes, uint64_t bound, uint8_t** out,
                    size_t* size, int ok, int internal, Encode encode) {
    ICX_HIP(ctx, hipSetDevice(ctx->device), internal);
    Buf<T> d_px;
    Buf<uint8_t> d_file;
    Buf<uint64_t> d_res;  // the file's size, then its status
    uint64_t res[2] = {0, 0};
    hipStream_t st = ctx->stream;
    if (!(d_px.reserve(nbytes) && d_file.reserve(bound) && d_res.reserve(16) &&
          hipMemcpyAsync(d_px.p, pixels, nbytes, hipMemcpyHostToDevice, st) == hipSuccess)) {
        ctx->err = std::string(entry) + ": " + hipGetErrorString(hipGetLastError());
        return internal;
    }
    const T* src = d_px.p;
    const int rc = encode(&src, d_file.p, d_res.p, reinterpret_cast<int32_t*>(d_res.p + 1), st);
    if (rc != ok) return rc;
    ICX_HIP(ctx, hipMemcpy(res, d_res.p, 16, hipMemcpyDeviceToHost), internal);
    const int code = (int32_t)(res[1] & 0xFFFFFFFFu);
    if (code != ok) return code;
    uint8_t* hostp = (uint8_t*)std::malloc(res[0]);
    if (!hostp || hipMemcpy(hostp, d_file.p, res[0], hipMemcpyDeviceToHost) != hipSuccess) {
        std::free(hostp);
        (void)hipGetLastError();
        ctx->err = std::string(entry) + ": host allocation or copy failed";
        return internal;
    }
    *out = hostp;
    *size = (size_t)res[0];
    return ok;
}

// save_to_file's tail: writes the file save_to_memory made, and frees it.
static int write_file(icx_ctx* ctx, const char* entry, const char* path, uint8_t* mem, size_t size, int ok, int internal) {
    std::FILE* f = std::fopen(path, "wb");
    const bool wrote = f && std::fwrite(mem, 1, size, f) == size;
    const bool closed = f && std::fclose(f) == 0;
    std::free(mem);
    if (!wrote || !closed) {
        ctx->err = std::string(entry) + ": cannot write " + path;
        return internal;
    }
    return ok;
}

extern "C" {

const char* icx_version(void) { return "icx 0.1.0 gfx950"; }

const char* icx_last_error(const icx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

icx_ctx* icx_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_create_err = "no HIP device available (libicx has no CPU decode path)";
        return nullptr;
    }
    if (device < 0 || device >= n) {
        g_create_err = "device ordinal out of range";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_create_err = "hipSetDevice failed";
        return nullptr;
    }
    auto* c = new icx_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        g_create_err = "hipStreamCreate failed";
        delete c;
        return nullptr;
    }
    return c;
}

void icx_batch_destroy(icx_batch* b);

void icx_destroy(icx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->single) icx_batch_destroy(c->single);
    if (c->exr) exr_ws_destroy(c->exr);
    if (c->exrw) exrw_ws_destroy(c->exrw);
    if (c->tgaw) tgaw_ws_destroy(c->tgaw);
    if (c->bmpw) bmpw_ws_destroy(c->bmpw);
    if (c->hdrw) hdrw_ws_destroy(c->hdrw);
    if (c->pnmw) pnmw_ws_destroy(c->pnmw);
    if (c->ddsw) ddsw_ws_destroy(c->ddsw);
    if (c->tiffw) tiffw_ws_destroy(c->tiffw);
    if (c->gifw) gifw_ws_destroy(c->gifw);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void icx_free(void* p) { std::free(p); }
int icx_ctx_device(const icx_ctx* c) { return c ? c->device : -1; }
void* icx_ctx_stream(const icx_ctx* c) { return c ? (void*)c->stream : nullptr; }

int icx_jpeg_probe(const uint8_t* jpeg, size_t size, int* w, int* h, int* ncomp) {
    if (w) *w = 0;
    if (h) *h = 0;
    if (ncomp) *ncomp = 0;
    if (!jpeg) return ICX_NO_JPEG;
    auto d = std::make_unique<Desc>();
    int st = parse_headers(jpeg, (int64_t)std::min<size_t>(size, 0x7FFFFFFF), *d);
    if (st != kPending) return st;
    if (w) *w = d->W;
    if (h) *h = d->H;
    if (ncomp) *ncomp = d->nc == 1 ? 1 : 3;
    return ICX_OK;
}

// ----------------------------------------------------------------------------- batches
// Bytes of one workspace slot (one image in flight) for max_w x max_h images; fills the caps.
static int64_t ws_per_slot(GroupWs& ws, int max_w, int max_h) {
    ws.max_w = max_w;
    ws.max_h = max_h;
    ws.coef_cap = ws_coef_cap(max_w, max_h);
    ws.plane_cap = ws_plane_cap(max_w, max_h);
    ws.tmp_cap = ws_tmp_cap(max_w, max_h);
    // unstuffed entropy bytes per slot: 2 B/px (ICX_UPOOL_BPP; q90 4:2:0 is ~0.4, a 4:4:4 q100 photo
    // 1.3-2.5). A group whose scans pass the pool defers the rest to further entropy rounds
    // (launch_spec_entropy), so this sizes the common case, not a limit.
    const int bpp = std::getenv("ICX_UPOOL_BPP") ? std::max(1, std::min(16, std::atoi(std::getenv("ICX_UPOOL_BPP")))) : 2;
    ws.ucap = ((int64_t)max_w * max_h * bpp + 4095) / 4096 * 4096;
    ws.rst_cap = ((int64_t)max_w / 8 + 1) * ((int64_t)max_h / 8 + 1);  // >= MCUs per image
    // decode lanes of kSubBytesSmall .. kSubBytes bytes (k_spec_plan picks per image)
    const int64_t tiles_per_slot = ws.ucap / kTileBytes + 2;
    const int64_t lanes_per_slot = ((ws.ucap + kSubBytesSmall - 1) / kSubBytesSmall + kLanes - 1) / kLanes * kLanes + kLanes;
    // coefficient pool: kPoolPerSlot x coef_cap blocks per slot (int16 block + int32 DC escape + map entry)
    // (the generic upsample's ping-pong planes, 6 x tmp_cap, live in the coefficient pool: ws_alloc)
    // per tile: tiles, tile_obase. (tile_rbase, another int32_t per tile, has never been counted:
    // left so, because the automatic group size follows from this value.)
    constexpr int64_t per_tile = sizeof(TileRec) + sizeof(int32_t);
    static_assert(per_tile == 28, "ws_per_slot must not drift");
    // per lane: X, Y, sub, ent, nrec, guess_cnt, rec, gw, crec, clist
    constexpr int64_t per_lane = 2 * sizeof(uint64_t) + sizeof(SubRec) + sizeof(LaneEntry) + sizeof(int32_t) +
                                 4 * sizeof(int32_t) + sizeof(RecState) * kRec + sizeof(GwOut) + sizeof(GcRec) + sizeof(int2);
    static_assert(per_lane == 8 + 8 + 20 + 24 + 4 + 16 + 24 * kRec + 40 + 32 + 8, "ws_per_slot must not drift");
    return ws.coef_cap * kPoolPerSlotX4 / 4 * (64 * 2 + 4 + 8) + ws.plane_cap + (int64_t)sizeof(Desc) + ws.ucap +
           (int64_t)sizeof(StepSet) + tiles_per_slot * per_tile + ws.rst_cap * 8 + lanes_per_slot * per_lane +
           kMaxRepair * 4;
}

static void ws_free(GroupWs& ws, Blocks& mem) {
    mem.release();
    if (ws.ev_defer) (void)hipEventDestroy(ws.ev_defer);
    ws = GroupWs{};
}

// A failure part-way leaves what was allocated to `mem` (icx_batch_destroy frees it).
static bool ws_alloc(icx_ctx* ctx, GroupWs& ws, Blocks& mem, int group, int max_w, int max_h) {
    (void)ws_per_slot(ws, max_w, max_h);
    const int64_t tiles_per_slot = ws.ucap / kTileBytes + 2;
    const int64_t lanes_per_slot = ((ws.ucap + kSubBytesSmall - 1) / kSubBytesSmall + kLanes - 1) / kLanes * kLanes + kLanes;
    ws.slots = group;
    // the U pool and the flat tile / lane records it bounds: two slots' worth beyond the group, so
    // even a one-image group takes a 3 B/px scan (k_spec_plan sends images past the pool to
    // the sequential kernel)
    ws.upool = (int64_t)(group + 2) * ws.ucap;
    ICX_ALLOC(ctx, mem.alloc(ws.desc, sizeof(Desc) * group), false);
    // the coefficient pool (k_spec_plan places each image in it; the guess-write lanes' overflow
    // chunks and count blocks take its tail), + kGwChunk scratch blocks past pool_cap. The static
    // regions take 1.1 x each image's blocks; the tail, 2.5 (G + 2) - 1.1 G > 1.4 G image-blocks,
    // holds every block of every image in overflow chunks (a photo whose flat sky is a few lanes'
    // worth of bytes stores nearly all its blocks there) plus the count lanes' copies and the
    // chunks' rounding, so a conforming group never runs out of it.
    ws.pool_cap = (int64_t)(group + 2) * ws.coef_cap * kPoolPerSlotX4 / 4;
    ICX_ALLOC(ctx, mem.alloc(ws.ac, (size_t)(ws.pool_cap + kGwChunk) * 64 * 2), false);
    ICX_ALLOC(ctx, mem.alloc(ws.dc, (size_t)(ws.pool_cap + kGwChunk) * 4), false);
    ICX_ALLOC(ctx, mem.alloc(ws.map, (size_t)ws.pool_cap * sizeof(uint2)), false);
    ICX_ALLOC(ctx, mem.alloc(ws.chunk_next, (size_t)(ws.pool_cap / kGwChunk + 2) * 4), false);
    ICX_ALLOC(ctx, mem.alloc(ws.pool_next, sizeof(unsigned long long)), false);
    ICX_ALLOC(ctx, mem.alloc(ws.planes, (size_t)ws.plane_cap * group), false);
    // The generic upsample's ping-pong planes (exotic samplings only: k_upsample, k_convert) share
    // the coefficient pool's memory: launch_decode_back runs them after every kernel that reads the
    // group's coefficients (the pool holds >= 15 x the slot's MCU-padded pixels in bytes, the planes
    // 6 x (w + 8)(h + 8) <= 7.6 x), and the next group on this workspace writes the pool only after
    // that, in stream order. (A separate buffer only if the pool were ever too small.)
    if ((int64_t)(ws.pool_cap + kGwChunk) * 64 * 2 >= ws.tmp_cap * 6 * group) {
        ws.tmp = reinterpret_cast<uint8_t*>(ws.ac);
    } else {
        ICX_ALLOC(ctx, mem.alloc(ws.tmp, (size_t)ws.tmp_cap * 6 * group), false);
    }
    ws.tiles_cap = tiles_per_slot * (group + 2);
    ws.lanes_cap = lanes_per_slot * (group + 2);
    ICX_ALLOC(ctx, mem.alloc(ws.spec, sizeof(SpecImg) * group), false);
    ICX_ALLOC(ctx, mem.alloc(ws.tilepre, sizeof(int32_t) * (group + 1)), false);
    ICX_ALLOC(ctx, mem.alloc(ws.wgpre, sizeof(int32_t) * (group + 1)), false);
    ICX_ALLOC(ctx, mem.alloc(ws.wg2pre, sizeof(int32_t) * (group + 1)), false);
    ICX_ALLOC(ctx, mem.alloc(ws.totals, sizeof(int32_t) * 4), false);
    ICX_ALLOC(ctx, mem.alloc(ws.tiles, sizeof(TileRec) * ws.tiles_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.tile_obase, sizeof(int32_t) * ws.tiles_cap), false);
    // + slack: the entropy readers load whole 16-byte chunks (icx_spec_core.h Reader)
    ICX_ALLOC(ctx, mem.alloc(ws.U, (size_t)ws.upool + 256), false);
    ICX_ALLOC(ctx, mem.alloc(ws.X, sizeof(uint64_t) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.sub, sizeof(SubRec) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.rst, sizeof(int64_t) * ws.rst_cap * group), false);
    ICX_ALLOC(ctx, mem.alloc(ws.tile_rbase, sizeof(int32_t) * ws.tiles_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.ent, sizeof(LaneEntry) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.stats, sizeof(int32_t) * kPathStats), false);
    ICX_ALLOC(ctx, mem.alloc(ws.Y, sizeof(uint64_t) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.rec, sizeof(RecState) * kRec * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.nrec, sizeof(int32_t) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.guess_cnt, sizeof(int32_t) * 4 * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.repair, sizeof(int32_t) * kMaxRepair * group), false);
    ICX_ALLOC(ctx, mem.alloc(ws.steps, sizeof(StepSet) * group), false);
    ICX_ALLOC(ctx, mem.alloc(ws.gw, sizeof(GwOut) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.crec, sizeof(GcRec) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.clist, sizeof(int2) * ws.lanes_cap), false);
    ICX_ALLOC(ctx, mem.alloc(ws.h_defer, 3 * sizeof(int32_t), true), false);
    ws.h_defer[0] = ws.h_defer[1] = ws.h_defer[2] = 0;
    ICX_ALLOC(ctx, mem.alloc(ws.h_layout, sizeof(int32_t), true), false);
    *ws.h_layout = 1;
    ICX_HIP(ctx, hipEventCreateWithFlags(&ws.ev_defer, hipEventDisableTiming), false);
    return true;
}

icx_batch* icx_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h, int group) {
    if (!ctx || max_images <= 0 || max_w <= 0 || max_h <= 0 || max_w > 65535 || max_h > 65535) {
        if (ctx) ctx->err = "icx_batch_create: bad arguments";
        return nullptr;
    }
    ICX_HIP(ctx, hipSetDevice(ctx->device), nullptr);
    // Every early return below (an allocation or stream/event creation failing part-way) frees
    // what was already created: the deleter is icx_batch_destroy, which skips null members.
    std::unique_ptr<icx_batch, void (*)(icx_batch*)> b(new icx_batch(), icx_batch_destroy);
    b->ctx = ctx;
    b->max_images = max_images;
    // pipelines: ICX_PIPES (1..2, default 2) when the batch holds at least two images
    int pipes = kMaxPipes;
    if (const char* e = std::getenv("ICX_PIPES")) pipes = std::max(1, std::min(kMaxPipes, std::atoi(e)));
    if (max_images < 2) pipes = 1;
    GroupWs probe;
    const int64_t per_slot = ws_per_slot(probe, max_w, max_h);
    if (group <= 0) {  // auto: up to 80% of the free HBM (288 GB per MI355X), at least one image
        // (C3's 512 images per GPU fit one group per pipeline at ~395 MB per 4096^2 slot: 2 groups
        // of 256 instead of 4 of 128, C3 +3%, C3 with restart markers +12%: its interval lanes take
        // as long for 256 images as for 128)
        size_t free_b = 0, total_b = 0;
        ICX_HIP(ctx, hipMemGetInfo(&free_b, &total_b), nullptr);
        const int64_t budget = (int64_t)(0.8 * (double)free_b);
        group = (int)std::max<int64_t>(1, std::min<int64_t>(max_images, budget / per_slot));
    }
    group = std::min(group, max_images);
    if (group < 2) pipes = 1;
    b->pipes = pipes;
    if (const char* e = std::getenv("ICX_GROUPS")) b->min_groups = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("ICX_STAGGER")) b->stagger = std::atoi(e) != 0;
    for (int p = 0; p < pipes; ++p) {
        // `group` images in flight over all pipes: each workspace holds its share
        const int slots = (group + pipes - 1) / pipes;
        if (!ws_alloc(ctx, b->ws[p], b->mem[p], slots, max_w, max_h)) return nullptr;
        if (p > 0) ICX_HIP(ctx, hipStreamCreateWithFlags(&b->pst[p], hipStreamNonBlocking), nullptr);
        ICX_HIP(ctx, hipEventCreateWithFlags(&b->join[p], hipEventDisableTiming), nullptr);
    }
    ICX_HIP(ctx, hipEventCreateWithFlags(&b->fork, hipEventDisableTiming), nullptr);
    ICX_HIP(ctx, hipEventCreateWithFlags(&b->done, hipEventDisableTiming), nullptr);
    b->hook = std::make_unique<EventHook>();
    return b.release();
}

void icx_batch_destroy(icx_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    for (int p = 0; p < kMaxPipes; ++p) {
        ws_free(b->ws[p], b->mem[p]);
        if (b->pst[p]) (void)hipStreamDestroy(b->pst[p]);
        if (b->join[p]) (void)hipEventDestroy(b->join[p]);
    }
    if (b->fork) (void)hipEventDestroy(b->fork);
    if (b->done) (void)hipEventDestroy(b->done);
    for (auto e : b->front_done) (void)hipEventDestroy(e);
    delete b;
}

// How a call of n images is cut (equal-sized groups, see icx_jpeg_batch_decode): *per images a
// group (the last may hold fewer), returning the groups actually launched, ceil(n / per). Enough
// groups for the slots and at least ICX_GROUPS; and a multiple of the pipelines where rounding the
// count up still gives one (3 groups on 2 pipes run the third alone; 4 smaller ones keep both
// busy) -- only then, since a rounded-up count whose `per` launches fewer groups (n = 5 on slots
// of 2: 4 -> per 2 -> 3 groups) buys nothing.
static int batch_split(const icx_batch* b, int n, int* per_out) {
    const int slots = b->ws[0].slots;
    const int want = std::min(n, std::max((n + slots - 1) / slots, b->min_groups));
    int per = (n + want - 1) / want;
    int ng = (n + per - 1) / per;
    if (b->pipes > 1 && ng > 1 && ng % b->pipes) {
        const int up = (ng + b->pipes - 1) / b->pipes * b->pipes;
        if (up <= n) {
            const int per2 = (n + up - 1) / up;
            const int ng2 = (n + per2 - 1) / per2;
            if (ng2 % b->pipes == 0) {
                per = per2;
                ng = ng2;
            }
        }
    }
    *per_out = per;
    return ng;
}

int icx_batch_groups(const icx_batch* b, int n) {
    int per = 0;
    return b && n > 0 ? batch_split(b, n, &per) : 0;
}

int icx_jpeg_batch_decode(icx_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                          uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    if (!b) return ICX_INTERNAL_ERR;
    icx_ctx* ctx = b->ctx;
    if (n < 0 || n > b->max_images) { ctx->err = "icx_jpeg_batch_decode: n exceeds batch capacity"; return ICX_INTERNAL_ERR; }
    if (n == 0) return ICX_OK;
    if (!d_data || !d_off || !d_size || !d_out || !d_status || !d_dims) { ctx->err = "null pointer"; return ICX_INTERNAL_ERR; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const RoctxRange range("icx_jpeg_batch_decode");
    b->hook->reset();
    for (int p = 0; p < b->pipes; ++p)
        ICX_HIP(ctx, hipMemsetAsync(b->ws[p].stats, 0, sizeof(int32_t) * kPathStats, st), ICX_INTERNAL_ERR);
    // equal-sized groups (512 images on 361 slots -> 256 + 256, not 361 + 151): every kernel's
    // grid is sized by the work of its group, so a small tail group leaves the GPU half idle
    int per = 0;
    const int ng = batch_split(b, n, &per);
    const int used = std::min(b->pipes, ng);
    if (used > 1) {  // the other pipes start after the caller's prior work on `st`
        ICX_HIP(ctx, hipEventRecord(b->fork, st), ICX_INTERNAL_ERR);
        for (int p = 1; p < used; ++p) ICX_HIP(ctx, hipStreamWaitEvent(b->pst[p], b->fork, 0), ICX_INTERNAL_ERR);
    }
    // Software pipeline over the groups, alternating pipes: group g's front half (parse, unstuff,
    // entropy decode: latency-bound) starts when group g-1's front half is done, on the other
    // pipe's stream, so it runs beside group g-1's back half (IDCT, convert: HBM-bound) instead
    // of in lockstep with it.
    const bool stagger = b->stagger && used > 1;
    // Host waits (the deferred-image count and the layout flag read from pinned memory after
    // each group's plan) only when the call runs eagerly: under stream capture (hipGraph) a
    // host wait would invalidate the capture, so every entropy round and every layout's back
    // half is enqueued unconditionally (kFrontAll; empty rounds find no work). ICX_HOST_WAIT=0
    // forces that form without capture.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    ICX_HIP(ctx, hipStreamIsCapturing(st, &cap), ICX_INTERNAL_ERR);
    const char* hw = std::getenv("ICX_HOST_WAIT");  // (read per call: tests vary it)
    const bool no_wait_env = hw && std::atoi(hw) == 0;
    const bool host_wait = !stagger && cap == hipStreamCaptureStatusNone && !no_wait_env;
    while (stagger && (int)b->front_done.size() < ng) {
        hipEvent_t e;
        ICX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), ICX_INTERNAL_ERR);
        b->front_done.push_back(e);
    }
    // Entropy round 0 of the first group on each pipe goes out first; then, per group, the later
    // rounds only while its previous round deferred an image (the host reads that count once the
    // round's k_spec_plan has run: the call returns after the last group's planning, not after the
    // decode), its back half, and round 0 of the group that follows on the same pipe.
    auto front0 = [&](int g) {
        const int g0 = g * per, p = g % used;
        launch_decode_front(b->ws[p], std::min(per, n - g0), d_data, d_off + g0, d_size + g0, out_stride,
                            p == 0 ? st : b->pst[p], b->hook.get(), host_wait ? kFrontFirst : kFrontAll);
    };
    for (int g = 0; g < std::min(used, ng); ++g) {
        if (stagger && g > 0) ICX_HIP(ctx, hipStreamWaitEvent(b->pst[g % used], b->front_done[g - 1], 0), ICX_INTERNAL_ERR);
        front0(g);
        if (stagger) ICX_HIP(ctx, hipEventRecord(b->front_done[g], g % used == 0 ? st : b->pst[g % used]), ICX_INTERNAL_ERR);
    }
    for (int g = 0; g < ng; ++g) {
        const int g0 = g * per, gn = std::min(per, n - g0), p = g % used;
        hipStream_t ps = p == 0 ? st : b->pst[p];
        if (host_wait) launch_decode_front(b->ws[p], gn, d_data, d_off + g0, d_size + g0, out_stride, ps, b->hook.get(),
                                           kFrontRest);
        launch_decode_back(b->ws[p], gn, d_out + (uint64_t)g0 * out_stride, out_stride, d_status + g0, d_dims + 3 * g0,
                           ps, b->hook.get(), host_wait);
        const int gnext = g + used;
        if (gnext < ng) {
            hipStream_t pn = gnext % used == 0 ? st : b->pst[gnext % used];
            if (stagger) ICX_HIP(ctx, hipStreamWaitEvent(pn, b->front_done[gnext - 1], 0), ICX_INTERNAL_ERR);
            front0(gnext);
            if (stagger) ICX_HIP(ctx, hipEventRecord(b->front_done[gnext], pn), ICX_INTERNAL_ERR);
        }
    }
    for (int p = 1; p < used; ++p) {  // the caller's stream waits for every pipe
        ICX_HIP(ctx, hipEventRecord(b->join[p], b->pst[p]), ICX_INTERNAL_ERR);
        ICX_HIP(ctx, hipStreamWaitEvent(st, b->join[p], 0), ICX_INTERNAL_ERR);
    }
    // owned by the batch: path_stats waits on this event, never on the caller's stream (which
    // the caller may destroy after the call)
    ICX_HIP(ctx, hipEventRecord(b->done, st), ICX_INTERNAL_ERR);
    b->decoded = true;
    ICX_HIP(ctx, hipGetLastError(), ICX_INTERNAL_ERR);
    return ICX_OK;
}

// The batch's path counters summed over its pipelines (GroupWs::stats), once the last call's work is done.
static int batch_stats(const icx_batch* b, int32_t (&h)[kPathStats]) {
    for (int k = 0; k < kPathStats; ++k) h[k] = 0;
    // The decode ran on non-blocking streams, which the null stream does not order against:
    // wait for the batch's own event recorded after every pipe joined.
    ICX_HIP(b->ctx, hipSetDevice(b->ctx->device), ICX_INTERNAL_ERR);
    if (b->decoded) ICX_HIP(b->ctx, hipEventSynchronize(b->done), ICX_INTERNAL_ERR);
    for (int p = 0; p < b->pipes; ++p) {
        int32_t q[kPathStats];
        ICX_HIP(b->ctx, hipMemcpy(q, b->ws[p].stats, sizeof q, hipMemcpyDeviceToHost), ICX_INTERNAL_ERR);
        for (int k = 0; k < kPathStats; ++k) h[k] += q[k];
    }
    return ICX_OK;
}

int icx_batch_path_stats(const icx_batch* b, int32_t* parallel, int32_t* fallback, int32_t* sequential) {
    if (!b) return ICX_INTERNAL_ERR;
    int32_t h[kPathStats];
    const int rc = batch_stats(b, h);
    if (rc != ICX_OK) return rc;
    if (parallel) *parallel = h[0];
    if (fallback) *fallback = h[1];
    if (sequential) *sequential = h[2];
    return ICX_OK;
}

int icx_batch_dri_stats(const icx_batch* b, int32_t* gw, int32_t* gw_fallback) {
    if (!b) return ICX_INTERNAL_ERR;
    int32_t h[kPathStats];
    const int rc = batch_stats(b, h);
    if (rc != ICX_OK) return rc;
    if (gw) *gw = h[3];
    if (gw_fallback) *gw_fallback = h[4];
    return ICX_OK;
}

int icx_batch_group(const icx_batch* b) { return b ? b->ws[0].slots : 0; }

int icx_batch_stage_times(const icx_batch* b, const char** names, float* ms, int cap) {
    if (!b) return 0;
    float acc[kStCount];
    b->hook->sum(acc);
    int k = 0;
    for (int s = 0; s < kStCount && k < cap; ++s, ++k) {
        if (names) names[k] = kStageNames[s];
        if (ms) ms[k] = acc[s];
    }
    return kStCount;
}

int icx_jpeg_batch_decode_host(icx_batch* b, int n, const uint8_t* const* jpegs, const size_t* sizes,
                               uint8_t* const* outs, uint64_t out_stride, int32_t* status, int32_t* dims) {
    if (!b) return ICX_INTERNAL_ERR;
    icx_ctx* ctx = b->ctx;
    if (n <= 0) return n == 0 ? ICX_OK : ICX_INTERNAL_ERR;
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    std::vector<uint64_t> off(n), sz(n);
    uint64_t total = 0;
    for (int i = 0; i < n; ++i) { off[i] = total; sz[i] = sizes[i]; total += (sizes[i] + 15) & ~uint64_t(15); }
    const size_t meta = (size_t)n * (8 + 8 + 4 + 12);
    const size_t need = total + meta + (size_t)n * out_stride + 256;
    ICX_ALLOC(ctx, b->d_hin.reserve(need), ICX_OUT_OF_MEM);
    uint8_t* base = b->d_hin.p;
    uint8_t* d_data = base;
    uint64_t* d_off = reinterpret_cast<uint64_t*>(base + ((total + 15) & ~uint64_t(15)));
    uint64_t* d_sz = d_off + n;
    int32_t* d_st = reinterpret_cast<int32_t*>(d_sz + n);
    int32_t* d_dm = d_st + n;
    uint8_t* d_out = reinterpret_cast<uint8_t*>(((uintptr_t)(d_dm + 3 * n) + 255) & ~uintptr_t(255));
    hipStream_t st = ctx->stream;
    for (int i = 0; i < n; ++i)
        if (sz[i]) ICX_HIP(ctx, hipMemcpyAsync(d_data + off[i], jpegs[i], sz[i], hipMemcpyHostToDevice, st), ICX_INTERNAL_ERR);
    ICX_HIP(ctx, hipMemcpyAsync(d_off, off.data(), 8 * n, hipMemcpyHostToDevice, st), ICX_INTERNAL_ERR);
    ICX_HIP(ctx, hipMemcpyAsync(d_sz, sz.data(), 8 * n, hipMemcpyHostToDevice, st), ICX_INTERNAL_ERR);
    int rc = icx_jpeg_batch_decode(b, n, d_data, d_off, d_sz, d_out, out_stride, d_st, d_dm, st);
    if (rc) return rc;
    ICX_HIP(ctx, hipMemcpyAsync(status, d_st, 4 * n, hipMemcpyDeviceToHost, st), ICX_INTERNAL_ERR);
    ICX_HIP(ctx, hipMemcpyAsync(dims, d_dm, 12 * n, hipMemcpyDeviceToHost, st), ICX_INTERNAL_ERR);
    ICX_HIP(ctx, hipStreamSynchronize(st), ICX_INTERNAL_ERR);
    for (int i = 0; i < n; ++i) {
        const size_t bytes = (size_t)dims[3 * i] * dims[3 * i + 1] * dims[3 * i + 2];
        if (status[i] == ICX_OK && bytes)
            ICX_HIP(ctx, hipMemcpyAsync(outs[i], d_out + (uint64_t)i * out_stride, bytes, hipMemcpyDeviceToHost, st),
                    ICX_INTERNAL_ERR);
    }
    ICX_HIP(ctx, hipStreamSynchronize(st), ICX_INTERNAL_ERR);
    return ICX_OK;
}

// ------------------------------------------------------------------- one-image decode
// Image::readJpg's path (codecs.cpp:821-849): probe on the host for the allocation size,
// then the full GPU pipeline on a cached one-slot workspace.
static int decode_one(icx_ctx* ctx, const uint8_t* jpeg, size_t size, std::vector<uint8_t>& out, int& w, int& h,
                      int& color) {
    w = h = color = 0;
    out.clear();
    if (!ctx) return ICX_INTERNAL_ERR;
    int pw = 0, ph = 0, pc = 0;
    const int probe = icx_jpeg_probe(jpeg, size, &pw, &ph, &pc);
    if (probe != ICX_OK) return probe;  // header-level result is final (no entropy data reached)
    if (!ctx->single || ctx->single->ws[0].max_w < pw || ctx->single->ws[0].max_h < ph) {
        if (ctx->single) icx_batch_destroy(ctx->single);
        ctx->single = icx_batch_create(ctx, 1, std::max(pw, 1), std::max(ph, 1), 1);
        if (!ctx->single) return ICX_OUT_OF_MEM;
    }
    const uint8_t* in[1] = {jpeg};
    size_t sizes[1] = {std::min<size_t>(size, 0x7FFFFFFF)};
    out.resize(std::max<size_t>((size_t)pw * ph * 3, 1));
    uint8_t* outs[1] = {out.data()};
    int32_t st = 0, dims[3] = {0, 0, 0};
    int rc = icx_jpeg_batch_decode_host(ctx->single, 1, in, sizes, outs, out.size(), &st, dims);
    if (rc) return rc;
    if (st != ICX_OK) { out.clear(); return st; }
    w = dims[0];
    h = dims[1];
    color = dims[2] == 3;
    out.resize((size_t)w * h * dims[2]);
    return ICX_OK;
}

int icx_jpeg_decode(icx_ctx* ctx, const uint8_t* jpeg, size_t size, uint8_t** out, int* w, int* h, int* ncomp) {
    if (out) *out = nullptr;
    std::vector<uint8_t> buf;
    int W = 0, H = 0, color = 0;
    int rc = decode_one(ctx, jpeg, size, buf, W, H, color);
    if (w) *w = W;
    if (h) *h = H;
    if (ncomp) *ncomp = rc == ICX_OK ? (color ? 3 : 1) : 0;
    if (rc == ICX_OK && out && !buf.empty()) {
        *out = static_cast<uint8_t*>(std::malloc(buf.size()));
        if (!*out) return ICX_OUT_OF_MEM;
        std::memcpy(*out, buf.data(), buf.size());
    }
    return rc;
}

// ------------------------------------------------------- NanoJPEG-compatible state API
void icx_nj_init(icx_ctx* ctx) {
    if (!ctx) return;
    ctx->nj_image.clear();
    ctx->nj_w = ctx->nj_h = ctx->nj_color = ctx->nj_size = 0;
}
void icx_nj_done(icx_ctx* ctx) { icx_nj_init(ctx); }

int icx_nj_decode(icx_ctx* ctx, const void* jpeg, int size) {
    if (!ctx) return ICX_INTERNAL_ERR;
    icx_nj_init(ctx);  // njDecode starts with njDone (jpeg_dec.h:881)
    int W = 0, H = 0, color = 0;
    int rc = decode_one(ctx, static_cast<const uint8_t*>(jpeg), (size_t)(size & 0x7FFFFFFF), ctx->nj_image, W, H, color);
    if (rc == ICX_OK) {
        ctx->nj_w = W;
        ctx->nj_h = H;
        ctx->nj_color = color;
        ctx->nj_size = (int)ctx->nj_image.size();
    }
    return rc;
}
int icx_nj_get_width(const icx_ctx* ctx) { return ctx ? ctx->nj_w : 0; }
int icx_nj_get_height(const icx_ctx* ctx) { return ctx ? ctx->nj_h : 0; }
int icx_nj_is_color(const icx_ctx* ctx) { return ctx ? ctx->nj_color : 0; }
unsigned char* icx_nj_get_image(icx_ctx* ctx) {
    return (ctx && !ctx->nj_image.empty()) ? ctx->nj_image.data() : nullptr;
}
int icx_nj_get_image_size(const icx_ctx* ctx) { return ctx ? ctx->nj_size : 0; }

// ------------------------------------------------------------------ encode (tiny_jpeg)
int icx_tje_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, int quality, int width, int height,
                             int num_components, const unsigned char* src) {
    if (!ctx || !func) return 0;
    if (quality < 1 || quality > 3) { ctx->err = "quality must be 1, 2 or 3"; return 0; }   // jpeg_enc.h:1223
    if (num_components != 3 && num_components != 4) { ctx->err = "num_components must be 3 or 4"; return 0; }  // :954
    if (width > 0xFFFF || height > 0xFFFF || width < 0 || height < 0) { ctx->err = "image too large"; return 0; }  // :958
    if ((int64_t)width * height > 0 && !src) { ctx->err = "null source"; return 0; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), 0);
    std::vector<uint8_t> file;
    if (!tje_encode_gpu(ctx->stream, quality, width, height, num_components, src, file)) {
        ctx->err = "HIP failure in tje_encode_gpu";
        return 0;
    }
    // tje hands the sink buffered chunks of TJEI_BUFFER_SIZE-1 bytes (jpeg_enc.h:474-496)
    for (size_t o = 0; o < file.size(); o += 1023)
        func(context, file.data() + o, (int)std::min<size_t>(1023, file.size() - o));
    return 1;
}

static void file_sink(void* ctx, void* data, int size) { std::fwrite(data, (size_t)size, 1, (FILE*)ctx); }

int icx_tje_encode_to_file_at_quality(icx_ctx* ctx, const char* dest_path, int quality, int width, int height,
                                      int num_components, const unsigned char* src) {
    FILE* fd = std::fopen(dest_path, "wb");  // jpeg_enc.h:1194-1213
    if (!fd) { if (ctx) ctx->err = "could not open file for writing"; return 0; }
    int result = icx_tje_encode_with_func(ctx, file_sink, fd, quality, width, height, num_components, src);
    result |= 0 == std::fclose(fd);  // the reference's own (lossy) success rule, :1210
    return result;
}

int icx_tje_encode_to_file(icx_ctx* ctx, const char* dest_path, int width, int height, int num_components,
                           const unsigned char* src) {
    return icx_tje_encode_to_file_at_quality(ctx, dest_path, 3, width, height, num_components, src);  // :1177-1185
}

// ------------------------------------------------------------------ encode extension (C4)
static const char* enc_args_bad(int quality, int subsampling, int width, int height, int comps) {
    if (quality < 1 || quality > 100) return "quality must be 1..100";
    if (subsampling != 444 && subsampling != 420) return "subsampling must be 444 or 420";
    if (comps != 3 && comps != 4) return "num_components must be 3 or 4";
    if (width > 0xFFFF || height > 0xFFFF || width < 0 || height < 0) return "image too large";
    return nullptr;
}

int icx_jpeg_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, int quality, int subsampling,
                              int width, int height, int num_components, const unsigned char* src) {
    if (!ctx || !func) return 0;
    if (const char* e = enc_args_bad(quality, subsampling, width, height, num_components)) { ctx->err = e; return 0; }
    if ((int64_t)width * height > 0 && !src) { ctx->err = "null source"; return 0; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), 0);
    std::vector<uint8_t> file;
    if (!jpeg_encode_gpu(ctx->stream, quality, subsampling, width, height, num_components, src, file)) {
        ctx->err = "HIP failure in jpeg_encode_gpu";
        return 0;
    }
    for (size_t o = 0; o < file.size(); o += 1023)
        func(context, file.data() + o, (int)std::min<size_t>(1023, file.size() - o));
    return 1;
}

struct icx_encoder {
    icx_ctx* ctx = nullptr;
    EncWs* ws = nullptr;
};

icx_encoder* icx_encoder_create(icx_ctx* ctx) {
    if (!ctx) return nullptr;
    icx_encoder* e = new icx_encoder();
    e->ctx = ctx;
    e->ws = enc_ws_create();
    return e;
}

void icx_encoder_destroy(icx_encoder* enc) {
    if (!enc) return;
    (void)hipSetDevice(enc->ctx->device);
    enc_ws_destroy(enc->ws);
    delete enc;
}

int icx_encoder_stage_times(icx_encoder* enc, const char** names, float* ms, int cap) {
    if (!enc || cap <= 0) return 0;
    return enc_ws_stage_times(enc->ws, names, ms, cap);
}

int icx_jpeg_encode_device(icx_encoder* enc, int quality, int subsampling, int width, int height,
                           int num_components, const uint8_t* d_src, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* out_size, void* hip_stream) {
    if (!enc || !out_size) return ICX_UNSUPPORTED;
    icx_ctx* ctx = enc->ctx;
    if (const char* e = enc_args_bad(quality, subsampling, width, height, num_components)) {
        ctx->err = e;
        return ICX_UNSUPPORTED;
    }
    if (((int64_t)width * height > 0 && !d_src) || (out_cap && !d_out)) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    const int rc = jpeg_encode_device(st, enc->ws, quality, subsampling, width, height, num_components, d_src, d_out,
                                      out_cap, out_size);
    if (rc < 0) { ctx->err = "HIP failure in jpeg_encode_device"; return ICX_INTERNAL_ERR; }
    return rc == 0 ? ICX_OK : ICX_OUT_OF_MEM;
}

int icx_jpeg_encode_device_batch(icx_encoder* enc, int n, int quality, int subsampling, int width, int height,
                                 int num_components, const uint8_t* const* d_srcs, uint8_t* d_out, uint64_t out_stride,
                                 uint64_t* out_sizes, int32_t* status, void* hip_stream) {
    if (!enc || n < 0 || (n > 0 && (!d_srcs || !out_sizes || !status))) return ICX_UNSUPPORTED;
    icx_ctx* ctx = enc->ctx;
    if (const char* e = enc_args_bad(quality, subsampling, width, height, num_components)) {
        ctx->err = e;
        return ICX_UNSUPPORTED;
    }
    for (int i = 0; i < n; ++i)
        if ((int64_t)width * height > 0 && !d_srcs[i]) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    if (n > 0 && out_stride && !d_out) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    std::vector<int32_t> rc(n > 0 ? n : 1);
    if (jpeg_encode_device_batch(st, enc->ws, n, quality, subsampling, width, height, num_components, d_srcs, d_out,
                                 out_stride, out_sizes, rc.data()) < 0) {
        ctx->err = "HIP failure in jpeg_encode_device_batch";
        return ICX_INTERNAL_ERR;
    }
    for (int i = 0; i < n; ++i) status[i] = rc[i] == 0 ? ICX_OK : ICX_OUT_OF_MEM;
    return ICX_OK;
}

// ------------------------------------------------------------------ PNG (png_encoder::saveToFile)
static const char* png_args_bad(int w, int h, int d) {
    if (d != 3 && d != 4) return "d must be 3 or 4";
    if (w <= 0 || h <= 0) return "empty image";
    if ((int64_t)w * h > (int64_t)1 << 31) return "image too large";
    return nullptr;
}

int icx_png_encode_with_func(icx_ctx* ctx, icx_write_func* func, void* context, const unsigned char* pixels, int width,
                             int height, int d) {
    if (!ctx || !func) return 0;
    if (const char* e = png_args_bad(width, height, d)) { ctx->err = e; return 0; }
    if (!pixels) { ctx->err = "null source"; return 0; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), 0);
    std::vector<uint8_t> file;
    if (!png_encode_gpu(ctx->stream, width, height, d, pixels, file)) {
        ctx->err = "HIP failure in png_encode_gpu";
        return 0;
    }
    for (size_t o = 0; o < file.size(); o += 1023)
        func(context, file.data() + o, (int)std::min<size_t>(1023, file.size() - o));
    return 1;
}

int icx_png_save_to_file(icx_ctx* ctx, const char* path, const unsigned char* pixels, int width, int height, int d) {
    if (!ctx || !path) return ICX_UNSUPPORTED;
    FILE* fd = std::fopen(path, "wb");
    if (!fd) { ctx->err = "could not open file for writing"; return ICX_INTERNAL_ERR; }
    const int ok = icx_png_encode_with_func(ctx, file_sink, fd, pixels, width, height, d);
    const bool closed = std::fclose(fd) == 0;
    if (!ok) return png_args_bad(width, height, d) || !pixels ? ICX_UNSUPPORTED : ICX_INTERNAL_ERR;
    return closed ? ICX_OK : ICX_INTERNAL_ERR;
}

// Images the PNG batch entry keeps in flight (each with its own workspace and stream):
// ICX_PNG_INFLIGHT, 1..8.
constexpr int kPngInflightMax = 8;
struct icx_png_encoder {
    icx_ctx* ctx = nullptr;
    PngWs* ws = nullptr;
    PngWs* wsx[kPngInflightMax] = {};      // the batch entry's other workspaces + streams (created on use)
    hipStream_t stx[kPngInflightMax] = {};
    hipEvent_t fork = nullptr;
};

icx_png_encoder* icx_png_encoder_create(icx_ctx* ctx) {
    if (!ctx) return nullptr;
    icx_png_encoder* e = new icx_png_encoder();
    e->ctx = ctx;
    e->ws = png_ws_create();
    return e;
}

void icx_png_encoder_destroy(icx_png_encoder* enc) {
    if (!enc) return;
    (void)hipSetDevice(enc->ctx->device);
    png_ws_destroy(enc->ws);
    for (int j = 0; j < kPngInflightMax; ++j) {
        if (enc->wsx[j]) png_ws_destroy(enc->wsx[j]);
        if (enc->stx[j]) (void)hipStreamDestroy(enc->stx[j]);
    }
    if (enc->fork) (void)hipEventDestroy(enc->fork);
    delete enc;
}

int icx_png_encode_device(icx_png_encoder* enc, int width, int height, int d, const uint8_t* d_src, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* out_size, void* hip_stream) {
    if (!enc || !out_size) return ICX_UNSUPPORTED;
    icx_ctx* ctx = enc->ctx;
    if (const char* e = png_args_bad(width, height, d)) { ctx->err = e; return ICX_UNSUPPORTED; }
    if (!d_src || (out_cap && !d_out)) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    const int rc = png_encode_device(st, enc->ws, width, height, d, d_src, d_out, out_cap, out_size);
    if (rc < 0) { ctx->err = "HIP failure in png_encode_device"; return ICX_INTERNAL_ERR; }
    return rc == 0 ? ICX_OK : ICX_OUT_OF_MEM;
}

int icx_png_encode_device_batch(icx_png_encoder* enc, int n, int width, int height, int d, const uint8_t* const* d_srcs,
                                uint8_t* d_out, uint64_t out_stride, uint64_t* out_sizes, int32_t* status,
                                void* hip_stream) {
    if (!enc || n < 0 || (n > 0 && (!d_srcs || !out_sizes || !status))) return ICX_UNSUPPORTED;
    icx_ctx* ctx = enc->ctx;
    if (const char* e = png_args_bad(width, height, d)) { ctx->err = e; return ICX_UNSUPPORTED; }
    for (int i = 0; i < n; ++i)
        if (!d_srcs[i]) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    if (n > 0 && (!d_out || !out_stride)) { ctx->err = "null buffer"; return ICX_UNSUPPORTED; }
    if (n == 0) return ICX_OK;
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_INTERNAL_ERR);
    const int k = [] {  // (read per call)
        const char* e = std::getenv("ICX_PNG_INFLIGHT");
        return e ? std::max(1, std::min(kPngInflightMax, std::atoi(e))) : kPngInflightMax;
    }();
    if (!enc->fork) ICX_HIP(ctx, hipEventCreateWithFlags(&enc->fork, hipEventDisableTiming), ICX_INTERNAL_ERR);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    // the other streams start after the caller's prior work on `st` (which may produce the inputs)
    ICX_HIP(ctx, hipEventRecord(enc->fork, st), ICX_INTERNAL_ERR);
    hipStream_t sts[kPngInflightMax];
    PngWs* wss[kPngInflightMax];
    sts[0] = st;
    wss[0] = enc->ws;
    for (int j = 1; j < k; ++j) {
        if (!enc->wsx[j]) enc->wsx[j] = png_ws_create();
        if (!enc->stx[j]) ICX_HIP(ctx, hipStreamCreateWithFlags(&enc->stx[j], hipStreamNonBlocking), ICX_INTERNAL_ERR);
        ICX_HIP(ctx, hipStreamWaitEvent(enc->stx[j], enc->fork, 0), ICX_INTERNAL_ERR);
        sts[j] = enc->stx[j];
        wss[j] = enc->wsx[j];
    }
    std::vector<int32_t> rc(n, -1);
    for (int i = 0; i < n; ++i) out_sizes[i] = 0;
    const int call = png_encode_device_batch(k, sts, wss, n, width, height, d, d_srcs, d_out, out_stride, out_sizes,
                                             rc.data());
    // every image gets its own status, also when another one failed: 0 OK, 1 its file did not fit
    // out_stride, -1 a HIP or host allocation failure in its own job
    for (int i = 0; i < n; ++i) {
        status[i] = rc[i] == 0 ? ICX_OK : rc[i] == 1 ? ICX_OUT_OF_MEM : ICX_INTERNAL_ERR;
        if (rc[i] < 0) out_sizes[i] = 0;
    }
    if (call < 0) {  // a stream failed: the whole call
        ctx->err = "HIP failure in png_encode_device_batch";
        return ICX_INTERNAL_ERR;
    }
    for (int i = 0; i < n; ++i)
        if (rc[i] < 0) { ctx->err = "png_encode_device_batch: an image's job failed (see status)"; break; }
    return ICX_OK;
}

int icx_png_encoder_stage_times(icx_png_encoder* enc, const char** names, float* ms, int cap) {
    if (!enc || cap <= 0) return 0;
    const int k = png_ws_stage_times(enc->ws, names, ms, cap);
    for (int j = 1; j < kPngInflightMax; ++j) {  // the batch entry's other workspaces: summed
        if (!enc->wsx[j] || !ms) continue;
        float m2[8] = {};
        const int k2 = png_ws_stage_times(enc->wsx[j], nullptr, m2, std::min(cap, 8));
        for (int i = 0; i < std::min(k, k2); ++i) ms[i] += m2[i];
    }
    return k;
}

// --------------------------------------------------------- Radiance .hdr (Image::readHdr)
int icx_hdr_probe(const uint8_t* data, size_t size, int* w, int* h) {
    int ww = 0, hh = 0;
    const int rc = data ? hdr_probe(data, (int64_t)size, &ww, &hh) : ICX_HDR_NOT_RADIANCE;
    return probe_out(rc, ICX_HDR_OK, w, ww, h, hh);
}

icx_hdr_batch* icx_hdr_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<HdrFmt>(ctx, max_images, max_w, max_h);
}

void icx_hdr_batch_destroy(icx_hdr_batch* b) { read_batch_destroy(b); }

int icx_hdr_batch_decode(icx_hdr_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         float* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    const int rc = read_batch_decode<HdrFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
    if (rc != ICX_HDR_OK) return rc;
    b->last_n = n;
    if (n == 0) return rc;
    // owned by the batch: locate_stats waits on this event, never on the caller's stream (which
    // the caller may destroy after the call)
    if (!b->done) ICX_HIP(b->ctx, hipEventCreateWithFlags(&b->done, hipEventDisableTiming), ICX_HDR_INTERNAL_ERR);
    ICX_HIP(b->ctx, hipEventRecord(b->done, stream ? (hipStream_t)stream : b->ctx->stream), ICX_HDR_INTERNAL_ERR);
    return rc;
}

int icx_hdr_batch_locate_stats(const icx_hdr_batch* b, int32_t* modes, int32_t* ncand, int cap) {
    if (!b) return ICX_HDR_INTERNAL_ERR;
    const int n = b->last_n;
    if (n <= 0) return 0;
    // The decode may have run on a non-blocking stream, which the null stream does not order
    // against: wait for the batch's own event recorded after it.
    ICX_HIP(b->ctx, hipSetDevice(b->ctx->device), ICX_HDR_INTERNAL_ERR);
    ICX_HIP(b->ctx, hipEventSynchronize(b->done), ICX_HDR_INTERNAL_ERR);
    std::vector<HdrDesc> h((size_t)n);
    ICX_HIP(b->ctx, hipMemcpy(h.data(), b->ws.desc, (size_t)n * sizeof(HdrDesc), hipMemcpyDeviceToHost), ICX_HDR_INTERNAL_ERR);
    for (int i = 0; i < n && i < cap; ++i) {
        if (modes) modes[i] = h[i].mode;
        if (ncand) ncand[i] = h[i].ncand;
    }
    return n;
}

int icx_hdr_batch_stage_times(const icx_hdr_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, HdrFmt::kOrder, HdrFmt::kLabel, names, ms, cap) : 0;
}

int icx_hdr_decode(icx_ctx* ctx, const uint8_t* data, size_t size, float** out, int* w, int* h, int* rows) {
    if (out) *out = nullptr;
    zero_out({w, h, rows});
    if (!ctx || !out) return ICX_HDR_INTERNAL_ERR;
    int ww = 0, hh = 0;
    const int prc = icx_hdr_probe(data, size, &ww, &hh);
    if (prc != ICX_HDR_OK) return prc;  // header errors need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_HDR_INTERNAL_ERR);
    std::unique_ptr<icx_hdr_batch, void (*)(icx_hdr_batch*)> b(icx_hdr_batch_create(ctx, 1, ww, hh), icx_hdr_batch_destroy);
    if (!b) return ICX_HDR_INTERNAL_ERR;
    const uint64_t nout = 4ull * ww * hh;  // floats
    OneShot io;
    // (through the public entry: its hook and roctx range; the readers load past the file's end)
    if (!one_shot_run(ctx, io, data, size, size + 16, nout * 4, 4, [&](OneShot& o, hipStream_t st) {
            return icx_hdr_batch_decode(b.get(), 1, o.in.p, o.meta.p, o.meta.p + 1, reinterpret_cast<float*>(o.out.p), nout,
                                        o.res.p, o.res.p + 1, st) == ICX_HDR_OK;
        })) {
        if (ctx->err.empty()) ctx->err = "icx_hdr_decode: HIP failure";
        return ICX_HDR_INTERNAL_ERR;
    }
    // whatever the status: a truncated file returns the rows it had, and how many
    return one_shot_take<HdrFmt>(ctx, io, nout * 4, out, {w, h, rows});
}

// --------------------------------------------------------- PNG read (Image::readPng)
int icx_png_probe(const uint8_t* data, size_t size, int* w, int* h) {
    int ww = 0, hh = 0;
    const int rc = data ? pngd_probe(data, (int64_t)size, &ww, &hh) : ICX_PNGR_NOT_PNG;
    return probe_out(rc, ICX_PNGR_OK, w, ww, h, hh);
}

icx_png_batch* icx_png_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<PngFmt>(ctx, max_images, max_w, max_h);
}

void icx_png_batch_destroy(icx_png_batch* b) { read_batch_destroy(b); }

int icx_png_batch_decode(icx_png_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<PngFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_png_batch_stage_times(const icx_png_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, PngFmt::kOrder, PngFmt::kLabel, names, ms, cap) : 0;
}

int icx_png_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* w, int* h) {
    if (out) *out = nullptr;
    zero_out({w, h});
    if (!ctx || !out) return ICX_PNGR_INTERNAL_ERR;
    int ww = 0, hh = 0;
    const int prc = icx_png_probe(data, size, &ww, &hh);
    if (prc != ICX_PNGR_OK) return prc;  // header and chunk errors need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_PNGR_INTERNAL_ERR);
    std::unique_ptr<icx_png_batch, void (*)(icx_png_batch*)> b(icx_png_batch_create(ctx, 1, ww, hh), icx_png_batch_destroy);
    if (!b) return ICX_PNGR_INTERNAL_ERR;
    const uint64_t nout = 4ull * ww * hh;
    // (through the public entry: its hook and roctx range)
    return read_one<PngFmt>(ctx, data, size, nout, out, {w, h}, [&](OneShot& o, hipStream_t st) {
        return icx_png_batch_decode(b.get(), 1, o.in.p, o.meta.p, o.meta.p + 1, o.out.p, nout, o.res.p, o.res.p + 1, st) ==
               ICX_PNGR_OK;
    });
}

// --------------------------------------------------------- OpenEXR (Image::readExr)
int icx_exr_probe(const uint8_t* data, size_t size, int* w, int* h) {
    if (w) *w = 0;
    if (h) *h = 0;
    if (!data) return ICX_EXR_INVALID_ARGUMENT;
    try {  // (nothing may cross the C ABI: a host allocation failure is an internal error)
        return exr_probe(data, size, w, h);
    } catch (const std::exception&) {
        return ICX_EXR_INTERNAL_ERR;
    }
}

int icx_exr_decode(icx_ctx* ctx, const uint8_t* data, size_t size, float** out, int* w, int* h) {
    if (out) *out = nullptr;
    if (w) *w = 0;
    if (h) *h = 0;
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (!data || !out) return ICX_EXR_INVALID_ARGUMENT;  // LoadEXRFromMemory's NULL checks (:6648-6651)
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_EXR_INTERNAL_ERR);
    const RoctxRange range("icx_exr_decode");
    int ww = 0, hh = 0;
    std::string err;
    int rc;
    try {  // (nothing may cross the C ABI: a host allocation failure is an internal error)
        if (!ctx->exr) ctx->exr = exr_ws_create();
        rc = exr_decode(ctx->stream, *ctx->exr, data, size, nullptr, nullptr, 0, out, &ww, &hh, err);
    } catch (const std::exception& e) {
        err = std::string("icx_exr_decode: ") + e.what();
        rc = ICX_EXR_INTERNAL_ERR;
    }
    if (rc == ICX_EXR_INTERNAL_ERR) ctx->err = err.empty() ? "icx_exr_decode: HIP failure" : err;
    if (rc == ICX_EXR_SUCCESS) {
        if (w) *w = ww;
        if (h) *h = hh;
    }
    return rc;
}

int icx_exr_decode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* data, const uint8_t* const* d_data,
                                const size_t* sizes, float* const* d_out, const size_t* out_floats, int32_t* codes,
                                int32_t* widths, int32_t* heights) {
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (n < 0 || (n > 0 && (!data || !d_data || !sizes || !d_out || !out_floats || !codes || !widths || !heights)))
        return ICX_EXR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i)
        if (!data[i] || !d_data[i] || !d_out[i] || (reinterpret_cast<uintptr_t>(d_data[i]) & 15)) {
            ctx->err = "icx_exr_decode_device_batch: d_data[i] must be non-null and 16-byte aligned";
            return ICX_EXR_INVALID_ARGUMENT;
        }
    if (n == 0) return ICX_EXR_SUCCESS;
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_EXR_INTERNAL_ERR);
    const RoctxRange range("icx_exr_decode_device_batch");
    std::string err;
    int rc;
    try {
        if (!ctx->exr) ctx->exr = exr_ws_create();
        rc = exr_decode_batch(ctx->stream, *ctx->exr, n, data, d_data, sizes, d_out, out_floats, codes, widths, heights, err);
    } catch (const std::exception& e) {
        err = std::string("icx_exr_decode_device_batch: ") + e.what();
        rc = ICX_EXR_INTERNAL_ERR;
    }
    if (rc != 0) {
        ctx->err = err.empty() ? "icx_exr_decode_device_batch: HIP failure" : err;
        return ICX_EXR_INTERNAL_ERR;
    }
    return ICX_EXR_SUCCESS;
}

int icx_exr_decode_device(icx_ctx* ctx, const uint8_t* data, const uint8_t* d_data, size_t size, float* d_out,
                          size_t out_floats, int* w, int* h) {
    if (w) *w = 0;
    if (h) *h = 0;
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (!data || !d_data || !d_out || (reinterpret_cast<uintptr_t>(d_data) & 15)) {
        ctx->err = "icx_exr_decode_device: d_data must be non-null and 16-byte aligned";
        return ICX_EXR_INVALID_ARGUMENT;
    }
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_EXR_INTERNAL_ERR);
    const RoctxRange range("icx_exr_decode_device");
    int ww = 0, hh = 0;
    std::string err;
    int rc;
    try {
        if (!ctx->exr) ctx->exr = exr_ws_create();
        rc = exr_decode(ctx->stream, *ctx->exr, data, size, d_data, d_out, out_floats, nullptr, &ww, &hh, err);
    } catch (const std::exception& e) {
        err = std::string("icx_exr_decode_device: ") + e.what();
        rc = ICX_EXR_INTERNAL_ERR;
    }
    if (rc == ICX_EXR_INTERNAL_ERR) ctx->err = err.empty() ? "icx_exr_decode_device: HIP failure" : err;
    if (rc == ICX_EXR_SUCCESS) {
        if (w) *w = ww;
        if (h) *h = hh;
    }
    return rc;
}

// --------------------------------------------------------- OpenEXR (Image::writeExr)
size_t icx_exr_encode_bound(int width, int height, int components, int save_as_fp16) {
    try {
        return exrw_encode_bound(width, height, components, save_as_fp16);
    } catch (const std::exception&) {
        return 0;
    }
}

int icx_exr_encode_device_batch(icx_ctx* ctx, int n, const float* const* d_src, const int32_t* widths,
                                const int32_t* heights, int components, int save_as_fp16, uint8_t* const* d_out,
                                const size_t* caps, int32_t* codes, size_t* sizes) {
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (n < 0 || (n > 0 && (!d_src || !widths || !heights || !d_out || !caps || !codes || !sizes)))
        return ICX_EXR_INVALID_ARGUMENT;
    if (n == 0) return ICX_EXR_SUCCESS;
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_EXR_INTERNAL_ERR);
    const RoctxRange range("icx_exr_encode_device_batch");
    std::string err;
    int rc;
    try {  // (nothing may cross the C ABI: a host allocation failure is an internal error)
        if (!ctx->exrw) ctx->exrw = exrw_ws_create();
        rc = exrw_encode_batch(ctx->stream, *ctx->exrw, n, d_src, widths, heights, components, save_as_fp16, d_out, caps,
                               codes, sizes, err);
    } catch (const std::exception& e) {
        err = std::string("icx_exr_encode_device_batch: ") + e.what();
        rc = ICX_EXR_INTERNAL_ERR;
    }
    if (rc != 0) {
        ctx->err = err.empty() ? "icx_exr_encode_device_batch: HIP failure" : err;
        return ICX_EXR_INTERNAL_ERR;
    }
    for (int i = 0; i < n; ++i)
        if (codes[i] == ICX_EXR_INTERNAL_ERR) ctx->err = "icx_exr_encode_device_batch: an output buffer is too small";
    return ICX_EXR_SUCCESS;
}

int icx_exr_encode_device(icx_ctx* ctx, const float* d_src, int width, int height, int components, int save_as_fp16,
                          uint8_t* d_out, size_t cap, size_t* size) {
    if (size) *size = 0;
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (!d_src || !d_out || !size) return ICX_EXR_INVALID_ARGUMENT;
    int32_t code = 0, w = width, h = height;
    const int rc = icx_exr_encode_device_batch(ctx, 1, &d_src, &w, &h, components, save_as_fp16, &d_out, &cap, &code, size);
    if (rc != ICX_EXR_SUCCESS) return rc;
    if (code == ICX_EXR_INTERNAL_ERR) ctx->err = "icx_exr_encode_device: output buffer too small";
    return code;
}

int icx_exr_save_to_memory(icx_ctx* ctx, const float* data, int width, int height, int components, int save_as_fp16,
                           uint8_t** out, size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (!data || !out || !size || !exrw_args_ok(width, height, components)) return ICX_EXR_INVALID_ARGUMENT;
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_EXR_INTERNAL_ERR);
    const RoctxRange range("icx_exr_save_to_memory");
    std::string err;
    int rc;
    try {
        if (!ctx->exrw) ctx->exrw = exrw_ws_create();
        rc = exrw_save_to_memory(ctx->stream, *ctx->exrw, data, width, height, components, save_as_fp16, out, size, err);
    } catch (const std::exception& e) {
        err = std::string("icx_exr_save_to_memory: ") + e.what();
        rc = ICX_EXR_INTERNAL_ERR;
    }
    if (rc == ICX_EXR_INTERNAL_ERR) ctx->err = err.empty() ? "icx_exr_save_to_memory: HIP failure" : err;
    return rc;
}

int icx_exr_save_to_file(icx_ctx* ctx, const char* path, const float* data, int width, int height, int components,
                         int save_as_fp16) {
    if (!ctx) return ICX_EXR_INTERNAL_ERR;
    if (!path) return ICX_EXR_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_exr_save_to_memory(ctx, data, width, height, components, save_as_fp16, &mem, &size);
    if (rc != ICX_EXR_SUCCESS) return rc;
    return write_file(ctx, "icx_exr_save_to_file", path, mem, size, ICX_EXR_SUCCESS, ICX_EXR_INTERNAL_ERR);
}

// --------------------------------------------------------- Targa (Image::readTga / writeTga)
int icx_tga_probe(const uint8_t* data, size_t size, int* w, int* h, int* channels) {
    int ww = 0, hh = 0, dd = 0;
    const int rc = data ? tga_probe(data, (int64_t)size, &ww, &hh, &dd) : ICX_TGA_BAD_HEADER;
    return probe_out(rc, ICX_TGA_OK, w, ww, h, hh, channels, dd);
}

icx_tga_batch* icx_tga_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<TgaFmt>(ctx, max_images, max_w, max_h, true);
}

void icx_tga_batch_destroy(icx_tga_batch* b) { read_batch_destroy(b); }

int icx_tga_batch_decode(icx_tga_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<TgaFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_tga_batch_stage_times(const icx_tga_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, TgaFmt::kOrder, TgaFmt::kLabel, names, ms, cap) : 0;
}

int icx_tga_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* w, int* h, int* channels) {
    if (out) *out = nullptr;
    zero_out({w, h, channels});
    if (!ctx || !out) return ICX_TGA_INTERNAL_ERR;
    int ww = 0, hh = 0, dd = 0;
    const int prc = icx_tga_probe(data, size, &ww, &hh, &dd);
    if (prc != ICX_TGA_OK) return prc;  // header errors need no device work
    if ((int64_t)ww * hh > ((int64_t)1 << 30)) return ICX_TGA_TOO_LARGE;  // (no batch workspace is that large)
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_TGA_INTERNAL_ERR);
    // (the probe accepted the header: byte 2 is the image type, 9-11 run-length coded; a raw file
    // needs no tile tables, and the one slot holds just the image's w*h*d bytes)
    std::unique_ptr<icx_tga_batch, void (*)(icx_tga_batch*)> b(read_batch_new<TgaFmt>(ctx, 1, ww, hh, data[2] >= 9),
                                                               icx_tga_batch_destroy);
    if (!b) return ICX_TGA_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * dd;
    return read_one<TgaFmt>(ctx, data, size, nout, out, {w, h, channels}, launch_direct<TgaFmt>(b->ws, nout));
}

size_t icx_tga_encode_bound(int width, int height, int d) { return (size_t)tga_encode_bound(width, height, d); }

int icx_tga_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_TGA_INTERNAL_ERR;
    if (n < 0 || n > 65535 || (d != 1 && d != 3 && d != 4) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_TGA_INVALID_ARGUMENT;
    if (n == 0) return ICX_TGA_OK;
    return encode_batch_guarded(ctx, "icx_tga_encode_device_batch", ctx->tgaw, tgaw_ws_create, ICX_TGA_OK,
                                ICX_TGA_INTERNAL_ERR, [&](TgawWs& ws, std::string& err) {
                                    return tga_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                            heights, d, rle != 0, d_out, out_stride, d_sizes, d_status, err);
                                });
}

int icx_tga_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int rle, uint8_t** out,
                           size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_TGA_INTERNAL_ERR;
    const uint64_t bound = tga_encode_bound(width, height, d);
    if (!pixels || !out || !size || bound == 0) return ICX_TGA_INVALID_ARGUMENT;
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_tga_save_to_memory", pixels, (uint64_t)width * height * d, bound, out, size, ICX_TGA_OK,
                             ICX_TGA_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_tga_encode_device_batch(ctx, 1, src, &w, &h, d, rle, d_file, bound, d_size, d_status, st);
                             });
}

int icx_tga_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d, int rle) {
    if (!ctx) return ICX_TGA_INTERNAL_ERR;
    if (!path) return ICX_TGA_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_tga_save_to_memory(ctx, pixels, width, height, d, rle, &mem, &size);
    if (rc != ICX_TGA_OK) return rc;
    return write_file(ctx, "icx_tga_save_to_file", path, mem, size, ICX_TGA_OK, ICX_TGA_INTERNAL_ERR);
}


// --------------------------------------------------------- BMP (Image::readBmp / writeBmp)
int icx_bmp_probe(const uint8_t* data, size_t size, int* w, int* h, int* channels) {
    int ww = 0, hh = 0, dd = 0;
    const int rc = data ? bmp_probe(data, (int64_t)size, &ww, &hh, &dd, nullptr) : ICX_BMP_NOT_BMP;
    return probe_out(rc, ICX_BMP_OK, w, ww, h, hh, channels, dd);
}

icx_bmp_batch* icx_bmp_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    // (sizes read_batch_new refuses have no bound to speak of)
    const bool sized = max_w > 0 && max_h > 0 && (int64_t)max_w * max_h <= ((int64_t)1 << 30);
    return read_batch_new<BmpFmt>(ctx, max_images, max_w, max_h, sized ? bmp_stream_bound(max_w, max_h) : 0);
}

void icx_bmp_batch_destroy(icx_bmp_batch* b) { read_batch_destroy(b); }

int icx_bmp_batch_decode(icx_bmp_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<BmpFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_bmp_batch_stage_times(const icx_bmp_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, BmpFmt::kOrder, BmpFmt::kLabel, names, ms, cap) : 0;
}

int icx_bmp_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* w, int* h, int* channels) {
    if (out) *out = nullptr;
    zero_out({w, h, channels});
    if (!ctx || !out) return ICX_BMP_INTERNAL_ERR;
    int ww = 0, hh = 0, dd = 0;
    int64_t stream = 0;
    const int prc = data ? bmp_probe(data, (int64_t)size, &ww, &hh, &dd, &stream) : ICX_BMP_NOT_BMP;
    if (prc != ICX_BMP_OK) return prc;  // header errors (more than 2^30 pixels among them) need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_BMP_INTERNAL_ERR);
    // (the tile tables cover this file's own stream, whatever its length; a raw file needs none,
    // and the one slot holds just the image's w*h*d bytes)
    std::unique_ptr<icx_bmp_batch, void (*)(icx_bmp_batch*)> b(read_batch_new<BmpFmt>(ctx, 1, ww, hh, stream),
                                                               icx_bmp_batch_destroy);
    if (!b) return ICX_BMP_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * dd;
    return read_one<BmpFmt>(ctx, data, size, nout, out, {w, h, channels}, launch_direct<BmpFmt>(b->ws, nout));
}

size_t icx_bmp_encode_bound(int width, int height, int d) { return (size_t)bmp_encode_bound(width, height, d); }

int icx_bmp_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_BMP_INTERNAL_ERR;
    if (n < 0 || n > 65535 || (d != 1 && d != 3 && d != 4) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_BMP_INVALID_ARGUMENT;
    if (n == 0) return ICX_BMP_OK;
    return encode_batch_guarded(ctx, "icx_bmp_encode_device_batch", ctx->bmpw, bmpw_ws_create, ICX_BMP_OK,
                                ICX_BMP_INTERNAL_ERR, [&](BmpwWs& ws, std::string& err) {
                                    return bmp_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                            heights, d, d_out, out_stride, d_sizes, d_status, err);
                                });
}

int icx_bmp_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, uint8_t** out,
                           size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_BMP_INTERNAL_ERR;
    const uint64_t bound = bmp_encode_bound(width, height, d);
    if (!pixels || !out || !size || bound == 0) return ICX_BMP_INVALID_ARGUMENT;
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_bmp_save_to_memory", pixels, (uint64_t)width * height * d, bound, out, size, ICX_BMP_OK,
                             ICX_BMP_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_bmp_encode_device_batch(ctx, 1, src, &w, &h, d, d_file, bound, d_size, d_status, st);
                             });
}

int icx_bmp_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d) {
    if (!ctx) return ICX_BMP_INTERNAL_ERR;
    if (!path) return ICX_BMP_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_bmp_save_to_memory(ctx, pixels, width, height, d, &mem, &size);
    if (rc != ICX_BMP_OK) return rc;
    return write_file(ctx, "icx_bmp_save_to_file", path, mem, size, ICX_BMP_OK, ICX_BMP_INTERNAL_ERR);
}


// --------------------------------------------------------- Netpbm (Image::readPbm / writePbm)

static int pnm_probe_at(const uint8_t* data, size_t size, int* w, int* h, int* d, int* type, int* maxval, int64_t* raster_at) {
    int v[5] = {0, 0, 0, 0, 0};
    int64_t at = -1;
    const int rc = data ? pnm_probe(data, (int64_t)size, &v[0], &v[1], &v[2], &v[3], &v[4], &at) : ICX_PNM_NOT_PNM;
    int* const dst[5] = {w, h, d, type, maxval};
    for (int k = 0; k < 5; ++k)
        if (dst[k]) *dst[k] = rc == ICX_PNM_OK ? v[k] : 0;
    if (raster_at) *raster_at = at;
    return rc;
}

int icx_pnm_probe(const uint8_t* data, size_t size, int* w, int* h, int* channels, int* type, int* maxval) {
    return pnm_probe_at(data, size, w, h, channels, type, maxval, nullptr);
}

icx_pnm_batch* icx_pnm_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    if (max_w <= 0 || max_h <= 0) return read_batch_new<PnmFmt>(ctx, max_images, max_w, max_h, (int64_t)0);  // (refused there)
    return read_batch_new<PnmFmt>(ctx, max_images, max_w, max_h, pnm_default_tiles(max_w, max_h));
}

void icx_pnm_batch_destroy(icx_pnm_batch* b) { read_batch_destroy(b); }

int icx_pnm_batch_decode(icx_pnm_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         void* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<PnmFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_pnm_batch_stage_times(const icx_pnm_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, PnmFmt::kOrder, PnmFmt::kLabel, names, ms, cap) : 0;
}

// (the two halves of read_one with a tail of its own: a six-int record, a slot rounded up to 16
// bytes, and messages that say more)
int icx_pnm_decode(icx_ctx* ctx, const uint8_t* data, size_t size, void** out, int* w, int* h, int* channels, int* type,
                   int* maxval) {
    if (out) *out = nullptr;
    zero_out({w, h, channels, type, maxval});
    if (!ctx || !out) return ICX_PNM_INTERNAL_ERR;
    int ww = 0, hh = 0, dd = 0, tt = 0, mv = 0;
    int64_t raster_at = -1;
    const int prc = pnm_probe_at(data, size, &ww, &hh, &dd, &tt, &mv, &raster_at);
    if (prc != ICX_PNM_OK) return prc;  // header errors and a short binary raster need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_PNM_INTERNAL_ERR);
    // (a text file gets a tile for every kPnmTile bytes of its text: nothing is TOO_LARGE here)
    const int64_t tiles = raster_at >= 0 ? ((int64_t)size - raster_at + kPnmTile - 1) / kPnmTile + 1 : 0;
    std::unique_ptr<icx_pnm_batch, void (*)(icx_pnm_batch*)> b(read_batch_new<PnmFmt>(ctx, 1, ww, hh, tiles),
                                                               icx_pnm_batch_destroy);
    if (!b) return ICX_PNM_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * dd * pnm_elem_bytes(tt), stride = (nout + 15) & ~(uint64_t)15;
    OneShot io;
    if (!one_shot_run(ctx, io, data, size, size, stride, 6, launch_direct<PnmFmt>(b->ws, stride))) {
        const hipError_t e = hipGetLastError();
        ctx->err = std::string("icx_pnm_decode: HIP failure: ") + hipGetErrorString(e);
        return ICX_PNM_INTERNAL_ERR;
    }
    if (io.rec[0] == ICX_PNM_INTERNAL_ERR) ctx->err = "icx_pnm_decode: the text kernels left no verdict";
    return io.rec[0] == ICX_PNM_OK ? one_shot_take<PnmFmt>(ctx, io, nout, out, {w, h, channels, type, maxval}) : io.rec[0];
}

size_t icx_pnm_encode_bound(int width, int height, int d, int type, int format) {
    return (size_t)pnm_encode_bound(width, height, d, type, format);
}

int icx_pnm_encode_device_batch(icx_ctx* ctx, int n, const void* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int type, int format, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_PNM_INTERNAL_ERR;
    // (1, 1: whether this d, type and format go together at all)
    if (n < 0 || n > 65535 || !pnm_write_args_ok(1, 1, d, type, format) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_PNM_INVALID_ARGUMENT;
    if (n == 0) return ICX_PNM_OK;
    return encode_batch_guarded(ctx, "icx_pnm_encode_device_batch", ctx->pnmw, pnmw_ws_create, ICX_PNM_OK,
                                ICX_PNM_INTERNAL_ERR, [&](PnmwWs& ws, std::string& err) {
                                    return pnm_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n,
                                                            reinterpret_cast<const uint8_t* const*>(d_src), widths, heights, d,
                                                            type, format, d_out, out_stride, d_sizes, d_status, err);
                                });
}

int icx_pnm_save_to_memory(icx_ctx* ctx, const void* pixels, int width, int height, int d, int type, int format,
                           uint8_t** out, size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_PNM_INTERNAL_ERR;
    const uint64_t bound = pnm_encode_bound(width, height, d, type, format);
    if (!pixels || !out || !size || bound == 0) return ICX_PNM_INVALID_ARGUMENT;
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_pnm_save_to_memory", pixels, (uint64_t)width * height * d * pnm_elem_bytes(type), bound,
                             out, size, ICX_PNM_OK, ICX_PNM_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_pnm_encode_device_batch(ctx, 1, reinterpret_cast<const void* const*>(src), &w, &h, d,
                                                                    type, format, d_file, bound, d_size, d_status, st);
                             });
}

int icx_pnm_save_to_file(icx_ctx* ctx, const char* path, const void* pixels, int width, int height, int d, int type,
                         int format) {
    if (!ctx) return ICX_PNM_INTERNAL_ERR;
    if (!path) return ICX_PNM_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_pnm_save_to_memory(ctx, pixels, width, height, d, type, format, &mem, &size);
    if (rc != ICX_PNM_OK) return rc;
    return write_file(ctx, "icx_pnm_save_to_file", path, mem, size, ICX_PNM_OK, ICX_PNM_INTERNAL_ERR);
}

// --------------------------------------------------------- DDS (Image::readDds / writeDds)
static int dds_probe_all(const uint8_t* data, size_t size, int* w, int* h, int* d, int* type) {
    int v[4] = {0, 0, 0, 0};
    const int rc = data ? dds_probe(data, (int64_t)size, &v[0], &v[1], &v[2], &v[3]) : ICX_DDS_NOT_DDS;
    int* const dst[4] = {w, h, d, type};
    for (int k = 0; k < 4; ++k)
        if (dst[k]) *dst[k] = rc == ICX_DDS_OK ? v[k] : 0;
    return rc;
}

int icx_dds_probe(const uint8_t* data, size_t size, int* w, int* h, int* channels, int* type) {
    return dds_probe_all(data, size, w, h, channels, type);
}

icx_dds_batch* icx_dds_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<DdsFmt>(ctx, max_images, max_w, max_h);
}

void icx_dds_batch_destroy(icx_dds_batch* b) { read_batch_destroy(b); }

int icx_dds_batch_decode(icx_dds_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         void* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<DdsFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_dds_batch_stage_times(const icx_dds_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, DdsFmt::kOrder, DdsFmt::kLabel, names, ms, cap) : 0;
}

// (the two halves of read_one, as icx_pnm_decode: a five-int record and a slot rounded up to 16 bytes)
int icx_dds_decode(icx_ctx* ctx, const uint8_t* data, size_t size, void** out, int* w, int* h, int* channels, int* type) {
    if (out) *out = nullptr;
    zero_out({w, h, channels, type});
    if (!ctx || !out) return ICX_DDS_INTERNAL_ERR;
    int ww = 0, hh = 0, dd = 0, tt = 0;
    const int prc = dds_probe_all(data, size, &ww, &hh, &dd, &tt);
    if (prc != ICX_DDS_OK) return prc;  // header errors and a short top level need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_DDS_INTERNAL_ERR);
    std::unique_ptr<icx_dds_batch, void (*)(icx_dds_batch*)> b(read_batch_new<DdsFmt>(ctx, 1, ww, hh), icx_dds_batch_destroy);
    if (!b) return ICX_DDS_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * dd * dds_elem_bytes(tt), stride = (nout + 15) & ~(uint64_t)15;
    OneShot io;
    if (!one_shot_run(ctx, io, data, size, size, stride, 5, launch_direct<DdsFmt>(b->ws, stride))) {
        const hipError_t e = hipGetLastError();
        ctx->err = std::string("icx_dds_decode: HIP failure: ") + hipGetErrorString(e);
        return ICX_DDS_INTERNAL_ERR;
    }
    return io.rec[0] == ICX_DDS_OK ? one_shot_take<DdsFmt>(ctx, io, nout, out, {w, h, channels, type}) : io.rec[0];
}

size_t icx_dds_encode_bound(int width, int height, int d, int format) { return (size_t)dds_encode_bound(width, height, d, format); }

int icx_dds_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int format, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_DDS_INTERNAL_ERR;
    // (1, 1: whether this d and format are known at all)
    if (n < 0 || n > 65535 || !dds_write_args_ok(1, 1, d, format) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_DDS_INVALID_ARGUMENT;
    if (n == 0) return ICX_DDS_OK;
    return encode_batch_guarded(ctx, "icx_dds_encode_device_batch", ctx->ddsw, ddsw_ws_create, ICX_DDS_OK,
                                ICX_DDS_INTERNAL_ERR, [&](DdswWs& ws, std::string& err) {
                                    return dds_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                            heights, d, format, d_out, out_stride, d_sizes, d_status, err);
                                });
}

int icx_dds_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int format, uint8_t** out,
                           size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_DDS_INTERNAL_ERR;
    const uint64_t bound = dds_encode_bound(width, height, d, format);
    if (!pixels || !out || !size || bound == 0) return ICX_DDS_INVALID_ARGUMENT;
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_dds_save_to_memory", pixels, (uint64_t)width * height * d, bound, out, size, ICX_DDS_OK,
                             ICX_DDS_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_dds_encode_device_batch(ctx, 1, src, &w, &h, d, format, d_file, bound, d_size, d_status, st);
                             });
}

int icx_dds_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d, int format) {
    if (!ctx) return ICX_DDS_INTERNAL_ERR;
    if (!path) return ICX_DDS_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_dds_save_to_memory(ctx, pixels, width, height, d, format, &mem, &size);
    if (rc != ICX_DDS_OK) return rc;
    return write_file(ctx, "icx_dds_save_to_file", path, mem, size, ICX_DDS_OK, ICX_DDS_INTERNAL_ERR);
}

// --------------------------------------------------------- Radiance .hdr write (Image::writeHdr)
size_t icx_hdr_encode_bound(int width, int height, int d, int rle) { return (size_t)hdrw_encode_bound(width, height, d, rle); }

// (the arguments are checked before the context here, unlike the byte writers)
int icx_hdr_encode_device_batch(icx_ctx* ctx, int n, const float* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride,
                                uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (n < 0 || n > 65535 || (d != 3 && d != 4) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_HDR_INVALID_ARGUMENT;
    if (!ctx) return ICX_HDR_INTERNAL_ERR;
    if (n == 0) return ICX_HDR_OK;
    return encode_batch_guarded(ctx, "icx_hdr_encode_device_batch", ctx->hdrw, hdrw_ws_create, ICX_HDR_OK,
                                ICX_HDR_INTERNAL_ERR, [&](HdrwWs& ws, std::string& err) {
                                    return hdr_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                            heights, d, rle != 0, d_out, out_stride, d_sizes, d_status, err);
                                });
}

int icx_hdr_save_to_memory(icx_ctx* ctx, const float* pixels, int width, int height, int d, int rle, uint8_t** out,
                           size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    const uint64_t bound = hdrw_encode_bound(width, height, d, rle);
    if (!pixels || !out || !size || bound == 0) return ICX_HDR_INVALID_ARGUMENT;  // (before any device work)
    if (!ctx) return ICX_HDR_INTERNAL_ERR;
    const int32_t w = width, h = height;
    return save_one<float>(ctx, "icx_hdr_save_to_memory", pixels, (uint64_t)width * height * d * sizeof(float), bound, out, size,
                           ICX_HDR_OK, ICX_HDR_INTERNAL_ERR,
                           [&](const float* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                               return icx_hdr_encode_device_batch(ctx, 1, src, &w, &h, d, rle, d_file, bound, d_size, d_status, st);
                           });
}

int icx_hdr_save_to_file(icx_ctx* ctx, const char* path, const float* pixels, int width, int height, int d, int rle) {
    if (!path) return ICX_HDR_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_hdr_save_to_memory(ctx, pixels, width, height, d, rle, &mem, &size);
    if (rc != ICX_HDR_OK) return rc;
    return write_file(ctx, "icx_hdr_save_to_file", path, mem, size, ICX_HDR_OK, ICX_HDR_INTERNAL_ERR);
}

// --------------------------------------------------------- GIF (Image::readGif)
int icx_gif_probe(const uint8_t* data, size_t size, int* w, int* h) {
    int ww = 0, hh = 0;
    const int rc = data ? gif_probe(data, (int64_t)size, &ww, &hh) : ICX_GIF_BAD_HEADER;
    return probe_out(rc, ICX_GIF_OK, w, ww, h, hh);
}

icx_gif_batch* icx_gif_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<GifFmt>(ctx, max_images, max_w, max_h);
}

void icx_gif_batch_destroy(icx_gif_batch* b) { read_batch_destroy(b); }

int icx_gif_batch_decode(icx_gif_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                         uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<GifFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_gif_batch_stage_times(const icx_gif_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, GifFmt::kOrder, GifFmt::kLabel, names, ms, cap) : 0;
}

int icx_gif_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* w, int* h) {
    if (out) *out = nullptr;
    zero_out({w, h});
    if (!ctx || !out) return ICX_GIF_INTERNAL_ERR;
    int ww = 0, hh = 0;
    const int prc = icx_gif_probe(data, size, &ww, &hh);
    if (prc != ICX_GIF_OK) return prc;  // container errors need no device work
    if ((int64_t)ww * hh > ((int64_t)1 << 30)) return ICX_GIF_TOO_LARGE;  // (no batch workspace is that large)
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_GIF_INTERNAL_ERR);
    std::unique_ptr<icx_gif_batch, void (*)(icx_gif_batch*)> b(icx_gif_batch_create(ctx, 1, ww, hh), icx_gif_batch_destroy);
    if (!b) return ICX_GIF_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * 3;
    return read_one<GifFmt>(ctx, data, size, nout, out, {w, h}, launch_direct<GifFmt>(b->ws, nout));
}

// --------------------------------------------------------- TIFF (Image::readTiff)
int icx_tiff_probe(const uint8_t* data, size_t size, int* w, int* h, int* d) {
    int ww = 0, hh = 0, dd = 0, pw = 0, ph = 0;
    const int rc = data ? tiff_probe(data, (int64_t)size, &ww, &hh, &dd, &pw, &ph) : ICX_TIFF_NOT_TIFF;
    return probe_out(rc, ICX_TIFF_OK, w, ww, h, hh, d, dd);
}

icx_tiff_batch* icx_tiff_batch_create(icx_ctx* ctx, int max_images, int max_w, int max_h) {
    return read_batch_new<TiffFmt>(ctx, max_images, max_w, max_h);
}

void icx_tiff_batch_destroy(icx_tiff_batch* b) { read_batch_destroy(b); }

int icx_tiff_batch_decode(icx_tiff_batch* b, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                          uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, void* stream) {
    return read_batch_decode<TiffFmt>(b, n, d_data, d_off, d_size, d_out, out_stride, d_status, d_dims, stream);
}

int icx_tiff_batch_stage_times(const icx_tiff_batch* b, const char** names, float* ms, int cap) {
    return b ? read_stage_times(*b->hook, TiffFmt::kOrder, TiffFmt::kLabel, names, ms, cap) : 0;
}

int icx_tiff_decode(icx_ctx* ctx, const uint8_t* data, size_t size, uint8_t** out, int* w, int* h, int* d) {
    if (out) *out = nullptr;
    zero_out({w, h, d});
    if (!ctx || !out) return ICX_TIFF_INTERNAL_ERR;
    int ww = 0, hh = 0, dd = 0, pw = 0, ph = 0;
    const int prc = data ? tiff_probe(data, (int64_t)size, &ww, &hh, &dd, &pw, &ph) : ICX_TIFF_NOT_TIFF;
    if (prc != ICX_TIFF_OK) return prc;  // container errors need no device work
    ICX_HIP(ctx, hipSetDevice(ctx->device), ICX_TIFF_INTERNAL_ERR);
    // a workspace for the size padded to whole chunks: every file the walk accepts fits its scratch
    std::unique_ptr<icx_tiff_batch, void (*)(icx_tiff_batch*)> b(icx_tiff_batch_create(ctx, 1, pw, ph), icx_tiff_batch_destroy);
    if (!b) return ICX_TIFF_INTERNAL_ERR;
    const uint64_t nout = (uint64_t)ww * hh * dd;
    return read_one<TiffFmt>(ctx, data, size, nout, out, {w, h, d}, launch_direct<TiffFmt>(b->ws, nout));
}

// ------------------------------------------------------------ TIFF write (Image::writeTiff)
size_t icx_tiff_encode_bound(int width, int height, int d, int compression, int predictor, int rows_per_strip) {
    return (size_t)tiffw_bound(width, height, d, compression, predictor, rows_per_strip);
}

int icx_tiff_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                 const int32_t* heights, int d, int compression, int predictor, int rows_per_strip,
                                 uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_TIFF_INTERNAL_ERR;
    TiffwGeom g;  // (a 1 x 1 image tells whether d, the compression, the predictor and the rows go together)
    if (n < 0 || n > 65535 || !tiffw_geom(1, 1, d, compression, predictor, rows_per_strip, &g) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_TIFF_INVALID_ARGUMENT;
    if (n == 0) return ICX_TIFF_OK;
    return encode_batch_guarded(ctx, "icx_tiff_encode_device_batch", ctx->tiffw, tiffw_ws_create, ICX_TIFF_OK,
                                ICX_TIFF_INTERNAL_ERR, [&](TiffwWs& ws, std::string& err) {
                                    return tiffw_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                              heights, d, compression, predictor, rows_per_strip, d_out,
                                                              out_stride, d_sizes, d_status, err);
                                });
}

int icx_tiff_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int compression,
                            int predictor, int rows_per_strip, uint8_t** out, size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_TIFF_INTERNAL_ERR;
    const uint64_t bound = tiffw_bound(width, height, d, compression, predictor, rows_per_strip);
    if (!pixels || !out || !size || bound == 0) return ICX_TIFF_INVALID_ARGUMENT;
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_tiff_save_to_memory", pixels, (uint64_t)width * height * d, bound, out, size,
                             ICX_TIFF_OK, ICX_TIFF_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_tiff_encode_device_batch(ctx, 1, src, &w, &h, d, compression, predictor,
                                                                     rows_per_strip, d_file, bound, d_size, d_status, st);
                             });
}

int icx_tiff_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d,
                          int compression, int predictor, int rows_per_strip) {
    if (!ctx) return ICX_TIFF_INTERNAL_ERR;
    if (!path) return ICX_TIFF_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_tiff_save_to_memory(ctx, pixels, width, height, d, compression, predictor, rows_per_strip, &mem, &size);
    if (rc != ICX_TIFF_OK) return rc;
    return write_file(ctx, "icx_tiff_save_to_file", path, mem, size, ICX_TIFF_OK, ICX_TIFF_INTERNAL_ERR);
}

// ------------------------------------------------------------ GIF write (Image::writeGif)
size_t icx_gif_encode_bound(int width, int height, int segment_pixels) {
    return (size_t)gifw_bound(width, height, segment_pixels);
}

int icx_gif_encode_device_batch(icx_ctx* ctx, int n, const uint8_t* const* d_src, const int32_t* widths,
                                const int32_t* heights, int d, int segment_pixels, int dither, int palette_mode,
                                uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, void* stream) {
    if (!ctx) return ICX_GIF_INTERNAL_ERR;
    GifwGeom g;  // (a 1 x 1 image tells whether d and the options are legal)
    if (n < 0 || n > 65535 || !gifw_geom(1, 1, d, segment_pixels, dither, palette_mode, &g) ||
        (n > 0 && (!d_src || !widths || !heights || !d_out || !d_sizes || !d_status)))
        return ICX_GIF_INVALID_ARGUMENT;
    if (n == 0) return ICX_GIF_OK;
    return encode_batch_guarded(ctx, "icx_gif_encode_device_batch", ctx->gifw, gifw_ws_create, ICX_GIF_OK,
                                ICX_GIF_INTERNAL_ERR, [&](GifwWs& ws, std::string& err) {
                                    return gifw_encode_batch(stream ? (hipStream_t)stream : ctx->stream, ws, n, d_src, widths,
                                                             heights, d, segment_pixels, dither, palette_mode, d_out,
                                                             out_stride, d_sizes, d_status, err);
                                });
}

int icx_gif_save_to_memory(icx_ctx* ctx, const uint8_t* pixels, int width, int height, int d, int segment_pixels,
                           int dither, int palette_mode, uint8_t** out, size_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!ctx) return ICX_GIF_INTERNAL_ERR;
    GifwGeom g;
    if (!pixels || !out || !size || !gifw_geom(width, height, d, segment_pixels, dither, palette_mode, &g))
        return ICX_GIF_INVALID_ARGUMENT;
    const uint64_t bound = gifw_bound(width, height, segment_pixels);
    const int32_t w = width, h = height;
    return save_one<uint8_t>(ctx, "icx_gif_save_to_memory", pixels, (uint64_t)width * height * d, bound, out, size,
                             ICX_GIF_OK, ICX_GIF_INTERNAL_ERR,
                             [&](const uint8_t* const* src, uint8_t* d_file, uint64_t* d_size, int32_t* d_status, hipStream_t st) {
                                 return icx_gif_encode_device_batch(ctx, 1, src, &w, &h, d, segment_pixels, dither,
                                                                    palette_mode, d_file, bound, d_size, d_status, st);
                             });
}

int icx_gif_save_to_file(icx_ctx* ctx, const char* path, const uint8_t* pixels, int width, int height, int d,
                         int segment_pixels, int dither, int palette_mode) {
    if (!ctx) return ICX_GIF_INTERNAL_ERR;
    if (!path) return ICX_GIF_INVALID_ARGUMENT;
    uint8_t* mem = nullptr;
    size_t size = 0;
    const int rc = icx_gif_save_to_memory(ctx, pixels, width, height, d, segment_pixels, dither, palette_mode, &mem, &size);
    if (rc != ICX_GIF_OK) return rc;
    return write_file(ctx, "icx_gif_save_to_file", path, mem, size, ICX_GIF_OK, ICX_GIF_INTERNAL_ERR);
}

}  // extern "C"
