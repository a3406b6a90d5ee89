// icx_internal.h -- declarations shared by the host API (icx_api.cpp) and the kernel
// launchers (icx_decode.hip). Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "icx_jpeg.h"

namespace icx {

// ---- speculative parallel entropy decode (icx_spec.hip) ----
constexpr int kTileBytes = 4096;   // raw bytes per unstuff tile (256 lanes x 16 B)
constexpr int kSubBytes = 2560;      // longest decode lane (unstuffed bytes per subsequence)
constexpr int kMaxRounds = 8;        // entropy rounds per group at most (launch_spec_entropy; ICX_ROUNDS 1..8)
constexpr int kPoolPerSlotX4 = 10;   // coefficient pool: 2.5 x an image's blocks per workspace slot (icx_api.cpp)
constexpr int kSubBytesSmall = 512;  // shortest: k_spec_plan sizes each image's lanes in between so
                                     // they fill whole 512-lane workgroups (icx_spec.hip)
constexpr int kRec = 16;           // block-start states a guess lane records for resync
constexpr int kGenericWG = 4096;    // workgroups per launch of the other-sampling back-half kernels
constexpr int kGuessLead = 4096;     // bits a guess lane decodes before its range (k_gw_lane, k_spec_guess):
                                     // at most a quarter of the lane (min(kGuessLead, 2 x lane bytes))
constexpr int kMaxRepair = 1024;   // unsynchronised lanes repaired per image before giving up
constexpr int kLanes = 256;        // lanes per decode workgroup (lane records are numbered in these)
constexpr int kWriteLanesBig = 512;  // write-pass workgroup for large images: tables amortised
                                     // over 512 lanes -> 2 workgroups / CU = 4 waves per SIMD
constexpr int kSpecMaxBpm = 16;    // blocks per MCU handled by the parallel path
enum : int32_t { kSpecSyntax = 1, kSpecGiveUp = 2 };

struct SpecImg {
    int32_t mode;          // 0 not on this path, 1 active, 2 fall back to the sequential kernel,
                           // 3 restart intervals (DRI): one write lane per interval, 4 deferred to the
                           // next round (the pools were full), 5 finished in an earlier round
    int32_t err;           // kSpecSyntax | kSpecGiveUp (atomicOr)
    int32_t ntiles, tile_base;
    int32_t nwg, wg_base;  // 256-lane decode groups; the image's first lane record / 256 (subsequence
                           // images only: a flat numbering over the batch group's lane records)
    int32_t nsub, nrepair;   // lanes; unsynchronised lanes queued for repair
    int32_t nint, nrst;      // DRI (modes 3, and 1 with kint): restart intervals; restart markers found in U
    int32_t sub_bytes;       // unstuffed bytes per decode lane (mode 1)
    int32_t gw_S;            // guess-write static pool slots per lane (mode 1)
    int64_t scan_len;      // raw entropy-coded bytes (file end - scan start)
    int64_t ulen;          // unstuffed data bytes before FF D9 / end of file / bad marker
    int64_t errpos;        // unstuffed index whose fetch is a syntax error (INT64_MAX: none)
    int64_t total_blocks;
    int64_t uoff;          // byte offset of the image's unstuffed stream in GroupWs::U (4 KiB aligned)
    int32_t ncount;        // guess-write lanes queued for the count decode (k_gw_check)
    int32_t dri_first;     // DRI: 2 j + (kind == kDriElsewhere) of the first interval j not ending
                           // at its marker (dri_end_kind; atomicMin, INT32_MAX: none)
    int64_t tail_G, tail_n;  // guess-write: the lanes' blocks end at block tail_G, tail_n before the
    int32_t tail_p[3];       // frame's last (k_gw_tail reads on into the padding; DC predictors there)
    int32_t kint;            // guess-write over restart intervals (mode 1, DRI): lanes per interval
                             // (lane j in interval j / kint, icx_spec_core.h lane_span); 0 otherwise
};
struct TileRec { int32_t kept, end_err; int64_t end_at; int32_t nrst, pad_; };
struct SubRec { int32_t cnt, ds0, ds1, ds2; int32_t mism; };
// A block-start state seen by a guess lane: bit offset from the lane start, block-in-MCU,
// DC codes decoded before it, and the per-component DC-diff sums before it.
struct RecState { uint32_t rel; int32_t b, cnt; int32_t ds[3]; };
struct LaneEntry { int64_t G; int32_t p0, p1, p2, pad; };

// ---- guess-write path (icx_spec.hip k_gw_*; icx_spec_core.h gw_*) ----
// A guess lane decodes with the write tables and stores the blocks that start in its range
// itself; only lanes not synchronised at their start are decoded again (from the true entry, up
// to the first state they share with the guess). Blocks go to the group's coefficient pool:
// kGwStaticSlack x the image's average blocks per lane in a static region per lane, then chunks
// of kGwChunk blocks taken from the pool's tail by atomic add (flat areas hold thousands of
// blocks per lane), chained through GroupWs::chunk_next.
constexpr int kGwChunk = 32;
constexpr int kRecGw = kRec;    // MCU starts a guess-write lane records (the count lanes splice at the first
                                // they reach; a lane that cannot splice is count-decoded whole). (8 was
                                // tried in round 6: k_gw_lane -1%, but k_gw_count 0.64 -> 1.65 ms per 256
                                // images -- a few lanes of the C3 pool splice past record 7)
constexpr int64_t kGwMinPixels = 2048 * 2048;  // workspaces for larger images take the guess-write path
constexpr int kGwMaxWalk = 64;  // lanes a repair walk may re-derive before the image goes sequential
// Restart intervals on the guess-write path (round 6): an image whose intervals average at least
// kDriGwMin unstuffed bytes (ICX_DRI_GW: 0 never, 1 from kSubBytesSmall) has each interval cut into
// kint lanes of at most kSubBytes instead of one serial lane per interval (mode 3).
constexpr int kDriGwMin = 4096;
struct GwOut {
    uint64_t g0;     // first block start at or after the lane's start: pack_state(pos, b, 0)
    int32_t k;       // blocks the lane stored (slots 0 .. k-1)
    int32_t ds[3];   // lane-local DC sums over them (predictors relative to g0)
    int32_t err;     // slot of the first block whose decode failed since the last record (INT32_MAX: none)
    int32_t chunk0;  // first overflow chunk (pool block / kGwChunk), -1: none
    int32_t nrec;    // block-start records (RecState: MCU starts) taken after g0
    int16_t over;    // the pool ran out: the image goes sequential
    int16_t rerr;    // some record carries a failure of the stretch before it (RecState::b = its slot + 1)
};
static_assert(sizeof(GwOut) == 40, "the lane records size the workspace (ws_per_slot)");
struct GcRec {
    int32_t chunk0;  // the count lane's blocks: a chain of pool chunks (-1: none)
    int32_t pad_;
    int32_t c;       // blocks it stored: the true path from the previous lane's exit to the splice
    int32_t m;       // guess record it spliced at; -1: none (the c blocks are the whole lane); -2: the
                     // lane was synchronised at its start (no count decode)
    int32_t cds[3];  // DC sums over the c blocks
    int32_t err;     // first of the c blocks whose decode failed (INT32_MAX: none)
};

// Device workspace for one group of images processed together (slot i = image i of the
// group). Capacities are per slot and cover any sampling NanoJPEG accepts at max_w x max_h.
// Absolute quantized DC per block: stored in the block itself (natural index 0, never an AC
// position) as int16; values outside int16 (only corrupt streams) store kDcEscape there and the
// exact int32 in GroupWs::dc. Keeps the DC inside the block's 128-byte line (no scattered stores).
constexpr int16_t kDcEscape = INT16_MIN;
__host__ __device__ inline int16_t dc_cell(int32_t dc) {
    return (dc > -32768 && dc <= 32767) ? (int16_t)dc : kDcEscape;
}

constexpr int kPathStats = 5;  // GroupWs::stats: parallel, fallback, sequential, DRI guess-write, its fallback

struct GroupWs {
    int slots = 0;
    int max_w = 0, max_h = 0;
    int64_t coef_cap = 0;    // blocks per slot
    int64_t plane_cap = 0;   // bytes per slot (all components' IDCT planes)
    int64_t tmp_cap = 0;     // bytes per ping-pong buffer per component per slot
    Desc* desc = nullptr;    // [slots]
    int16_t* ac = nullptr;   // [pool_cap + kGwChunk][64] coefficient pool: quantized blocks, zig-zag order
    int32_t* dc = nullptr;   // [pool_cap + kGwChunk] int32 DC of pool blocks whose cell holds kDcEscape
    uint8_t* planes = nullptr;  // [slots][plane_cap]
    uint8_t* tmp = nullptr;     // [slots][3 comps][2 buffers][tmp_cap]; aliases `ac` unless that is too small
    // parallel entropy decode
    int64_t ucap = 0;           // unstuffed bytes per slot on average: U is one pool of (slots + 2) * ucap
                                // bytes, each image's stream at SpecImg::uoff (k_spec_plan), so one
                                // image may take several slots' worth (a noisy q100 4:4:4 scan ~2 B/px)
    int64_t upool = 0;          // bytes of the U pool: (slots + 2) * ucap
    int64_t tiles_cap = 0;      // flat tile records for the whole group
    int64_t lanes_cap = 0;      // flat lane records for the whole group
    SpecImg* spec = nullptr;    // [slots]
    int32_t* tilepre = nullptr; // [slots+1]
    int32_t* wgpre = nullptr;   // [slots+1] 256-lane groups
    int32_t* wg2pre = nullptr;  // [slots+1] kWriteLanesBig-lane groups (write pass, large images)
    int32_t* totals = nullptr;  // [4]: tiles, 256-lane groups, big write groups
    TileRec* tiles = nullptr;
    int32_t* tile_obase = nullptr;
    uint8_t* U = nullptr;       // [slots][ucap]
    uint64_t* X = nullptr;      // [lanes_cap] exit states (guess pass; repaired in place)
    uint64_t* Y = nullptr;      // [lanes_cap] exit states re-derived by the count pass
    RecState* rec = nullptr;    // [lanes_cap][kRec]
    int32_t* nrec = nullptr;    // [lanes_cap]
    int32_t* guess_cnt = nullptr;  // [lanes_cap][4]: DC codes and DC sums over the whole guess lane
    int32_t* repair = nullptr;  // [slots][kMaxRepair] lanes whose chain needs a serial repair
    SubRec* sub = nullptr;      // [lanes_cap]
    int64_t rst_cap = 0;        // restart markers recorded per slot (>= MCUs per image)
    int64_t* rst = nullptr;     // [slots][rst_cap] (U byte index << 3) | marker number
    int32_t* tile_rbase = nullptr;  // [tiles_cap] restart markers before the tile (per image)
    LaneEntry* ent = nullptr;   // [lanes_cap]
    struct StepSet* steps = nullptr;  // [slots] step tables (icx_step.h), built per group
    int32_t* stats = nullptr;   // [kPathStats] path counters (k_spec_finish), accumulated over a batch call
    // coefficient pool (Desc::acbase / mapped) and the guess-write path's records
    int64_t pool_cap = 0;              // pool blocks (+ kGwChunk scratch blocks allocated past it)
    uint2* map = nullptr;              // [pool_cap] block n of a mapped image: {pool block, DC offset} at acbase + n
    int32_t* chunk_next = nullptr;     // [pool_cap / kGwChunk + 1] overflow chunk chains
    unsigned long long* pool_next = nullptr;  // [1] next free pool block (k_spec_plan sets it past the static regions)
    GwOut* gw = nullptr;               // [lanes_cap]
    GcRec* crec = nullptr;             // [lanes_cap]
    int2* clist = nullptr;             // [lanes_cap] per image, in its lane-record range: (image, lane) to count-decode
    int32_t* h_defer = nullptr;        // pinned [3]: images the last k_spec_plan deferred, gave restart-interval lanes, gave
                                       // interval-aligned guess-write lanes
    int32_t* h_layout = nullptr;       // pinned: the group has an image outside the fused 4:2:0 layout (k_parse)
    hipEvent_t ev_defer = nullptr;     // after round 0's k_spec_plan
};

// Where block n of an image lives in its group's coefficient pool: the pool block and the offset
// to add to its DC cell (Desc::acbase / mapped).
struct BlkLoc {
    int64_t blk;
    int32_t dcoff;
};
__device__ __forceinline__ BlkLoc blk_loc(const Desc& d, const uint2* map, int64_t n) {
    if (!d.mapped) return BlkLoc{d.acbase + n, 0};
    const uint2 e = map[d.acbase + n];
    return BlkLoc{(int64_t)e.x, (int32_t)e.y};
}
// A block's absolute quantized DC: its cell (or the int32 escape) plus the location's offset.
// (The escape load sits in a wave-uniform branch that valid streams never take: as a per-lane
// select its s_waitcnt vmcnt(0) landed after the join, in every block's path, where it waited
// for every load and store the wave had in flight.)
__device__ __forceinline__ int32_t blk_dc(int16_t cell, const int32_t* dcv, const BlkLoc& l) {
    int32_t v = cell;
    if (__any(cell == kDcEscape)) {
        const int32_t e = dcv[l.blk];
        v = cell == kDcEscape ? e : v;
    }
    return wadd(v, l.dcoff);
}
// A block location whose map entry is still in flight: the entry is loaded unconditionally (for an
// image written in place the slot is in bounds and ignored) and resolved where the location is
// used, so the load's wait lands there and not right after the load (blk_loc's branch did that).
struct BlkPend {
    uint2 e;
    int64_t n;  // acbase + block index
};
__device__ __forceinline__ BlkPend blk_pend(const Desc& d, const uint2* map, int64_t n) {
    return BlkPend{map[d.acbase + n], d.acbase + n};
}
__device__ __forceinline__ BlkLoc blk_resolve(const Desc& d, const BlkPend& q) {
    return d.mapped ? BlkLoc{(int64_t)q.e.x, (int32_t)q.e.y} : BlkLoc{q.n, 0};
}


int64_t ws_coef_cap(int w, int h);
int64_t ws_plane_cap(int w, int h);
int64_t ws_tmp_cap(int w, int h);

// Stage hooks so the host can bracket each stage with HIP events.
enum Stage { kStParse = 0, kStUnstuff, kStEntropy, kStWrite, kStIdct, kStUpsample, kStConvert, kStCount };
extern const char* const kStageNames[kStCount];
struct StageHook {
    virtual void begin(Stage s, hipStream_t st) = 0;
    virtual void end(Stage s, hipStream_t st) = 0;
    virtual ~StageHook() = default;
};
// A launcher's hook (may be null) and stream.
struct Stages {
    StageHook* h;
    hipStream_t st;
    void begin(Stage s) const { if (h) h->begin(s, st); }
    void end(Stage s) const { if (h) h->end(s, st); }
};
// Workgroups per image of a kernel that takes rows in turn: at most max_h, about 16384 in all:
// max(1, min(max_h, 16384 / min(n, 16384))).
inline int rows_grid(int max_h, int n) {
    const int cap = n < 16384 ? 16384 / n : 1;
    return max_h < 1 ? 1 : max_h < cap ? max_h : cap;
}

// The two ends of a *_encode_batch (name: the entry's, for err); 0, or -1 with err set.
// jobs_upload: room for the job array in buf (a Buf<J>, icx_mem.h) and its copy to the device on st
// (the pageable array is read until encode_finish has synchronised). rest_ok: the writer's other
// buffers are reserved.
template <class B, class J>
int jobs_upload(const char* name, B& buf, const std::vector<J>& jobs, hipStream_t st, std::string& err, bool rest_ok = true) {
    const size_t bytes = jobs.size() * sizeof(J);
    const char* what = !rest_ok || !buf.reserve(bytes) ? ": allocation: " : nullptr;
    if (!what && hipMemcpyAsync(buf.p, jobs.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) what = ": copy: ";
    if (!what) return 0;
    (err = name) += what;
    err += hipGetErrorString(hipGetLastError());
    return -1;
}
// encode_finish: the launches' error, or the stream's once everything queued on it has run.
inline int encode_finish(const char* name, hipStream_t st, std::string& err) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    (err = name) += ": ";
    err += hipGetErrorString(e);
    return -1;
}
// The encoders' stage-time read-out: k = min(cap, n) names and accumulated ms copied out, every
// accumulator zeroed; returns k.
inline int stage_times_out(const char* const* stage, float* acc, int n, const char** names, float* ms, int cap) {
    const int k = cap < n ? cap : n;
    for (int i = 0; i < k; ++i) {
        if (names) names[i] = stage[i];
        if (ms) ms[i] = acc[i];
    }
    for (int i = 0; i < n; ++i) acc[i] = 0.f;
    return k;
}

// Enqueue the whole decode of `n` (<= ws.slots) images on `st`.
void launch_decode_group(const GroupWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off,
                         const uint64_t* d_size, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                         int32_t* d_dims, hipStream_t st, StageHook* hook);
// The same in two halves: front = parse, unstuff, entropy decode (latency-bound); back = IDCT,
// upsample, convert, statuses (HBM-bound). The batch scheduler overlaps one group's back with the
// next group's front on another stream.
// part: kFrontAll every entropy round; kFrontFirst parse + round 0 (ws.h_defer holds round 0's
// deferred-image count once ws.ev_defer has completed); kFrontRest the later rounds when that count
// is not 0 (the caller has waited for ws.ev_defer), then the sequential kernel.
enum { kFrontAll = 0, kFrontFirst = 1, kFrontRest = 2 };
void launch_decode_front(const GroupWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off,
                         const uint64_t* d_size, uint64_t out_stride, hipStream_t st, StageHook* hook,
                         int part = kFrontAll);
// known_layout: the host may wait for ws.ev_defer and read ws.h_layout (k_parse) to skip the
// other samplings' kernels when the group has only fused-layout 4:2:0 images.
void launch_decode_back(const GroupWs& ws, int n, uint8_t* d_out, uint64_t out_stride, int32_t* d_status,
                        int32_t* d_dims, hipStream_t st, StageHook* hook, bool known_layout = false);
void launch_spec_entropy(const GroupWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, hipStream_t st,
                         StageHook* hook, int part = kFrontAll);
// piece: kRoundAll the whole round; kRoundHead up to its restart-interval write; kRoundTail that
// write and the round's end; kRoundTailNoDri the end alone (no image got restart-interval lanes);
// kRoundTailGw that write on a small grid (only guess-write DRI images, whose lanes fall back to it
// when they cannot decide the image).
enum { kRoundAll = 0, kRoundHead = 1, kRoundTail = 2, kRoundTailNoDri = 3, kRoundTailGw = 4 };
void launch_spec_round(const GroupWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, hipStream_t st,
                       StageHook* hook, int round, int last, int piece = kRoundAll);

// Per-image result record (icx_records.hip; include/icx.h icx_record): status, dims and the
// 64-bit weighted word sum of the decoded bytes.
struct Record {
    int32_t status, w, h, c;
    uint64_t checksum;
};
static_assert(sizeof(Record) == 24, "icx_record layout");
void launch_records(int n, const uint8_t* d_out, uint64_t out_stride, const int32_t* d_status, const int32_t* d_dims,
                    Record* d_rec, int max_w, int max_h, hipStream_t st);

// tiny_jpeg-exact encode on the GPU (icx_encode.hip); `out` receives the whole file.
bool tje_encode_gpu(hipStream_t st, int quality, int w, int h, int comps, const uint8_t* src,
                    std::vector<uint8_t>& out);
// C4 extension encoder (4:4:4 / 4:2:0, IJG quality 1..100; oracle/tje_oracle.c or_jpeg_encode).
struct EncWs;
EncWs* enc_ws_create();
void enc_ws_destroy(EncWs* ws);
int enc_ws_stage_times(EncWs* ws, const char** names, float* ms, int cap);
bool jpeg_encode_gpu(hipStream_t st, int quality, int subsampling, int w, int h, int comps, const uint8_t* src,
                     std::vector<uint8_t>& out);
int jpeg_encode_device(hipStream_t st, EncWs* ws, int quality, int subsampling, int w, int h, int comps,
                       const uint8_t* d_src, uint8_t* d_out, uint64_t cap, uint64_t* size);
int jpeg_encode_device_batch(hipStream_t st, EncWs* ws, int n, int quality, int subsampling, int w, int h, int comps,
                             const uint8_t* const* d_srcs, uint8_t* d_out, uint64_t stride, uint64_t* sizes,
                             int32_t* status);

// PNG encoder (icx_png.hip): png_encoder::saveToFile's colour choice and filters, GPU deflate.
struct PngWs;
PngWs* png_ws_create();
void png_ws_destroy(PngWs* ws);
int png_ws_stage_times(PngWs* ws, const char** names, float* ms, int cap);
int png_encode_device_batch(int k, hipStream_t* sts, PngWs** wss, int n, int w, int h, int d,
                            const uint8_t* const* d_srcs, uint8_t* d_out, uint64_t stride, uint64_t* sizes,
                            int32_t* status);
int png_encode_device(hipStream_t st, PngWs* ws, int w, int h, int d, const uint8_t* d_src, uint8_t* d_out,
                      uint64_t cap, uint64_t* size);
bool png_encode_gpu(hipStream_t st, int w, int h, int d, const uint8_t* src, std::vector<uint8_t>& out);

// Radiance .hdr decode (icx_hdr.hip; Image::readHdr, codecs.cpp:706-777). Status codes match
// include/icx.h ICX_HDR_*; kHdrPending is internal.
enum : int32_t {
    kHdrOk = 0, kHdrNotRadiance = 1, kHdrBadHeader = 2, kHdrMalformed = 3, kHdrTruncated = 4, kHdrTooLarge = 5,
    kHdrPending = 6
};
struct HdrDesc {
    int32_t status, w, h, rows;
    int64_t ds, size;      // pixel data start, file size
    int32_t has_marker;    // an aligned old-style run marker exists (k_hdr_scan)
    int32_t not_flat;      // some row is not a plain RGBE row at ds + 4*w*y (k_hdr_flatcheck)
    int32_t ncand, new_ok; // new-style scanline starts found; they chain over all rows (k_hdr_link)
    int32_t mode;          // 0 failed, 1 all rows plain, 2 all rows new-style, 3 per-row table (k_hdr_walk)
    int32_t pad_;
};
struct HdrWs {
    int max_images = 0, max_w = 0, max_h = 0;
    HdrDesc* desc = nullptr;   // [max_images]
    int32_t* cq = nullptr;     // [max_images][kHdrCandCap] new-style scanline starts (relative to ds)
    int32_t* ce = nullptr;     // [max_images][kHdrCandCap] their ends (relative), or -1/-2/-3
    int64_t* start = nullptr;  // [max_images][max_h] row start (byte offset in the file)
    uint8_t* kind = nullptr;   // [max_images][max_h] row kind (mode 3)
    uint8_t* planes = nullptr; // [max_images][max_h][4][max_w] RGBE planes of run-length coded rows
};
int hdr_probe(const uint8_t* data, int64_t size, int* w, int* h);
int64_t hdr_ws_bytes(int max_images, int max_w, int max_h);
struct Blocks;  // icx_mem.h: owns the workspace's device memory
bool hdr_ws_alloc(HdrWs& ws, Blocks& mem, int max_images, int max_w, int max_h);
void launch_hdr_decode(const HdrWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       float* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);

// PNG read (icx_pngd.hip; Image::readPng, codecs.cpp:903-1020). Status codes: icx_pngd_core.h
// kPngr* = include/icx.h ICX_PNGR_*.
struct PngdDesc;
struct PngdWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t scap = 0, zcap = 0;  // bytes per image of scr and z (multiples of 16)
    PngdDesc* desc = nullptr;    // [max_images]
    uint8_t* scr = nullptr;      // [max_images][scap] filtered bytes, un-filtered in place
    uint8_t* z = nullptr;        // [max_images][zcap] the IDAT payloads as one zlib stream
};
int pngd_probe(const uint8_t* data, int64_t size, int* w, int* h);
bool pngd_ws_alloc(PngdWs& ws, Blocks& mem, int max_images, int max_w, int max_h);
void launch_pngd_decode(const PngdWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                        uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                        StageHook* hook);

// Targa read and write (icx_tga.hip; Image::readTga / writeTga, codecs.cpp:1304-1437). Status
// codes: icx_tga_core.h kTga* = include/icx.h ICX_TGA_*.
struct TgaDesc;
struct TgaWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t tiles_cap = 0;        // stream tiles per image (any stream of max_w x max_h pixels); 0: a
                                  // workspace for raw files only (an RLE file is TOO_LARGE there)
    TgaDesc* desc = nullptr;      // [max_images]
    uint32_t* summary = nullptr;  // [max_images][tiles_cap][kTgaEntries] chain summaries (k_tga_tiles)
    int32_t* entry = nullptr;     // [max_images][tiles_cap] offset of the tile's first packet (k_tga_chain)
    int32_t* pbase = nullptr;     // [max_images][tiles_cap] pixels decoded before it
};
int tga_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d);
bool tga_ws_alloc(TgaWs& ws, Blocks& mem, int max_images, int max_w, int max_h, bool rle = true);
void launch_tga_decode(const TgaWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);
// Netpbm read and write (icx_pnm.hip; Image::readPbm / writePbm, codecs.cpp:1034-1167). Status
// codes: icx_pnm_core.h kPnm* = include/icx.h ICX_PNM_*.
struct PnmDesc;
struct PnmWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t tiles_cap = 0;       // tiles of raster text per image; 0: a workspace for binary files only
                                 // (an ASCII file is TOO_LARGE there)
    PnmDesc* desc = nullptr;     // [max_images]
    int4* summary = nullptr;     // [max_images][tiles_cap] token starts, carried comment bit, first illegal byte (k_pnm_tiles)
    int64_t* tbase = nullptr;    // [max_images][tiles_cap] the tile's first sample index << 1 | starts in a comment (k_pnm_chain)
};
// The probe's code; for kPnmOk the header's values, and *raster_at = where the text of an ASCII
// file starts (-1 for a binary file).
int pnm_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* type, int* maxval, int64_t* raster_at);
int64_t pnm_default_tiles(int max_w, int max_h);
bool pnm_ws_alloc(PnmWs& ws, Blocks& mem, int max_images, int max_w, int max_h, int64_t tiles_cap);
void launch_pnm_decode(const PnmWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);
struct PnmwWs;  // grow-only buffers of the write
PnmwWs* pnmw_ws_create();
void pnmw_ws_destroy(PnmwWs* w);
// 0, or -1 for a HIP failure (err says which). Synchronises with `st`.
int pnm_encode_batch(hipStream_t st, PnmwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int type, int format, uint8_t* d_out, uint64_t out_stride,
                     uint64_t* d_sizes, int32_t* d_status, std::string& err);

// BMP read and write (icx_bmp.hip; Image::readBmp / writeBmp, codecs.cpp:255-375). Status codes:
// icx_bmp_core.h kBmp* = include/icx.h ICX_BMP_*.
struct BmpDesc;
struct BmpWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t tiles_cap = 0;        // stream tiles per image; 0: a workspace for raw files only (an RLE
                                  // file is TOO_LARGE there, as is a stream longer than the tiles cover)
    BmpDesc* desc = nullptr;      // [max_images]
    uint32_t* summary = nullptr;  // [max_images][tiles_cap][kBmpEntries] x 4 words: chain summaries (k_bmp_tiles)
    int32_t* entry = nullptr;     // [max_images][tiles_cap] slot of the tile's first packet (k_bmp_chain)
    int32_t* cur_x = nullptr;     // [max_images][tiles_cap] the cursor on entry
    int32_t* cur_y = nullptr;
};
// `stream` (may be null): 0 for a raw file, else 1 + the bytes from bfOffBits to the file's end.
int bmp_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int64_t* stream);
// The longest stream a batch workspace covers: every pixel its own 2-byte packet, an end-of-line
// per row and the end-of-bitmap.
int64_t bmp_stream_bound(int max_w, int max_h);
// stream_cap: stream bytes per image the tile tables cover; 0: raw files only.
bool bmp_ws_alloc(BmpWs& ws, Blocks& mem, int max_images, int max_w, int max_h, int64_t stream_cap);
void launch_bmp_decode(const BmpWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);
struct BmpwWs;  // grow-only buffers of the write
BmpwWs* bmpw_ws_create();
void bmpw_ws_destroy(BmpwWs* w);
// 0, or -1 for a HIP failure (err says which). Synchronises with `st`.
int bmp_encode_batch(hipStream_t st, BmpwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err);

// DDS read and write (icx_dds.hip; Image::readDds / writeDds). Status codes: icx_dds_core.h
// kDds* = include/icx.h ICX_DDS_*.
struct DdsDesc;
struct DdsWs {
    int max_images = 0, max_w = 0, max_h = 0;
    DdsDesc* desc = nullptr;  // [max_images]
};
int dds_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* type);
bool dds_ws_alloc(DdsWs& ws, Blocks& mem, int max_images, int max_w, int max_h);
void launch_dds_decode(const DdsWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);
struct DdswWs;  // grow-only buffers of the write
DdswWs* ddsw_ws_create();
void ddsw_ws_destroy(DdswWs* w);
// 0, or -1 for a HIP failure (err says which). Synchronises with `st`.
int dds_encode_batch(hipStream_t st, DdswWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int format, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err);

struct TgawWs;  // grow-only buffers of the write
TgawWs* tgaw_ws_create();
void tgaw_ws_destroy(TgawWs* w);
// 0, or -1 for a HIP failure (err says which). Synchronises with `st`.
int tga_encode_batch(hipStream_t st, TgawWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err);

// Radiance .hdr write (icx_hdrw.hip; arithmetic and codes in icx_hdrw_core.h).
struct HdrwWs;  // grow-only buffers of the write
HdrwWs* hdrw_ws_create();
void hdrw_ws_destroy(HdrwWs* w);
// 0, or -1 for a HIP failure (err says which). Synchronises with `st`.
int hdr_encode_batch(hipStream_t st, HdrwWs& ws, int n, const float* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err);

// GIF read (icx_gif.hip; Image::readGif, codecs.cpp:507-542). Status codes: icx_gif_core.h
// kGif* = include/icx.h ICX_GIF_*.
struct GifDesc;
struct GifWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t plane_stride = 0;  // bytes per image of plane (a multiple of 16)
    GifDesc* desc = nullptr;   // [max_images]
    uint8_t* plane = nullptr;  // [max_images][plane_stride] palette indices of the clipped frame rectangle
};
int gif_probe(const uint8_t* data, int64_t size, int* w, int* h);
bool gif_ws_alloc(GifWs& ws, Blocks& mem, int max_images, int max_w, int max_h);
void launch_gif_decode(const GifWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                       uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                       StageHook* hook);

// TIFF read (icx_tiff.hip; Image::readTiff, codecs.cpp:1439-1484). Status codes: icx_tiff_core.h
// kTiff* = include/icx.h ICX_TIFF_*.
struct TiffDesc;
struct TiffWs {
    int max_images = 0, max_w = 0, max_h = 0;
    int64_t slot = 0;            // bytes per image of scratch (tiff_scratch_slot: a multiple of 16)
    int unpack_grid = 0;         // workgroups of k_tiff_unpack (from the device's CU count)
    TiffDesc* desc = nullptr;    // [max_images]
    int32_t* count = nullptr;    // [max_images] chunks of each image that parsed
    int32_t* first = nullptr;    // [max_images + 1] their exclusive scan: the work list
    uint32_t* next = nullptr;    // the work list's next untaken item (k_tiff_unpack)
    uint8_t* scratch = nullptr;  // [max_images][slot] decompressed chunks, each in a room of its own
};
// pw, ph: the size padded to whole chunks
int tiff_probe(const uint8_t* data, int64_t size, int* w, int* h, int* d, int* pw, int* ph);
bool tiff_ws_alloc(TiffWs& ws, Blocks& mem, int device, int max_images, int max_w, int max_h);
void launch_tiff_decode(const TiffWs& ws, int n, const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_size,
                        uint8_t* d_out, uint64_t out_stride, int32_t* d_status, int32_t* d_dims, hipStream_t st,
                        StageHook* hook);

// ---- TIFF write (icx_tiffw.hip; contract in include/icx.h, serial part in icx_tiffw_core.h) ----
struct TiffwWs;
TiffwWs* tiffw_ws_create();
void tiffw_ws_destroy(TiffwWs* w);
// 0, or -1 with err set
int tiffw_encode_batch(hipStream_t st, TiffwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                       const int32_t* heights, int d, int comp, int pred, int rows_per_strip, uint8_t* d_out,
                       uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, std::string& err);

// ---- GIF write (icx_gifw.hip; contract in include/icx.h, serial part in icx_gifw_core.h) ----
struct GifwWs;
GifwWs* gifw_ws_create();
void gifw_ws_destroy(GifwWs* w);
// 0, or -1 with err set
int gifw_encode_batch(hipStream_t st, GifwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                      const int32_t* heights, int d, int segment_pixels, int dither, int palette_mode, uint8_t* d_out,
                      uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, std::string& err);

// ---- OpenEXR read (icx_exr.hip) ----
// tinyexr's LoadEXRFromMemory; returns its code (-100: HIP failure, err says which).
struct ExrWs;
ExrWs* exr_ws_create();
void exr_ws_destroy(ExrWs* w);
int exr_decode(hipStream_t st, ExrWs& ws, const uint8_t* data, size_t size, const uint8_t* d_file, float* d_out,
               size_t out_floats, float** out_rgba, int* width, int* height, std::string& err);
int exr_decode_batch(hipStream_t st, ExrWs& ws, int n, const uint8_t* const* data, const uint8_t* const* d_data,
                     const size_t* sizes, float* const* d_out, const size_t* out_floats, int32_t* codes, int32_t* widths,
                     int32_t* heights, std::string& err);
int exr_probe(const uint8_t* data, size_t size, int* width, int* height);

// ---- OpenEXR write (icx_exrw.hip) ----
// tinyexr's SaveEXR; codes are tinyexr's (-100: HIP failure, or a file that does not fit).
struct ExrwWs;
ExrwWs* exrw_ws_create();
void exrw_ws_destroy(ExrwWs* w);
bool exrw_args_ok(int width, int height, int components);
size_t exrw_encode_bound(int width, int height, int components, int fp16);
int exrw_encode_batch(hipStream_t st, ExrwWs& ws, int n, const float* const* d_src, const int32_t* widths,
                      const int32_t* heights, int components, int fp16, uint8_t* const* d_out, const size_t* caps,
                      int32_t* codes, size_t* sizes, std::string& err);
int exrw_save_to_memory(hipStream_t st, ExrwWs& ws, const float* data, int width, int height, int components, int fp16,
                        uint8_t** out, size_t* size, std::string& err);

}  // namespace icx
