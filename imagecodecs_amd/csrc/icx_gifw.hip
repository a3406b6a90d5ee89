// icx_gifw.hip -- GIF write on the MI355X: one GIF89a frame with a global table, its code stream
// cut into segments that end in a Clear, so that one image is coded by many waves. Contract:
// include/icx.h "GIF write"; the serial part and the bound: icx_gifw_core.h. All images of a call
// go through each kernel in one launch, nothing is read back.
//
//   k_gifw_colors   the image's colour set: a workgroup's set in LDS first, its keys then into the
//                   image's open-addressed set in memory; counting stops past 256 colours
//   k_gifw_palette  one workgroup per image: exact (rank the <= 256 keys) or the cube; mode, table
//                   bits, code size and the table's bytes into the image's record
//   k_gifw_index    pixels -> a 1 B/pixel index plane (rank lookup with the set in LDS, or the
//                   cube's arithmetic), 16-byte stores
//   k_gifw_lzw      one wave per segment: the chain appends (code, width) to an LDS list, all lanes
//                   stage, free the dictionary and pack LSB-first; the segment's bit length
//   k_gifw_scan     one workgroup per image: bit lengths -> bit offsets, the payload's and the
//                   file's size, TOO_LARGE; header, table and descriptor, terminator and trailer
//   k_gifw_merge    output-driven: every byte of the data area is a sub-block length or a payload
//                   byte assembled from the segments whose bits fall into it
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "icx_gifw_core.h"
#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_wave.h"

namespace icx {

namespace gifw {

constexpr int kInternal = -1;
constexpr int kSetSlots = 1024;  // an image's colour set: at most 257 keys are ever wanted
constexpr int kChunk = 16384;    // pixels per workgroup (colours, index), data bytes per workgroup (merge)

struct Img {
    const uint8_t* src;
    uint8_t* out;
    GifwGeom g;
    int32_t status;
    int32_t pad_;
    int64_t seg0;      // its segments in the bit-length table
    int64_t plane_at;  // its index plane (16-byte aligned)
    int64_t slot_at;   // its segments' rooms in the payload workspace
    int64_t slot;      // bytes per room (a multiple of 16)
    // written on the device
    int32_t cube, tb, m, pad2_;
    uint64_t total_bits, payload;
    uint8_t table[768];
};

__device__ __forceinline__ uint32_t set_hash(uint32_t key) { return (key * 2654435761u) >> 22; }

// Inserts key (stored + 1; 0: free) into a set of kSetSlots words. Returns 1 when the key is new,
// 0 when it was there, -1 when every slot is taken by other keys.
__device__ __forceinline__ int set_insert(uint32_t* set, uint32_t key) {
    uint32_t h = set_hash(key);
    for (int k = 0; k < kSetSlots; ++k) {
        const uint32_t e = atomicCAS(&set[h], 0u, key + 1u);
        if (e == 0u) return 1;
        if (e == key + 1u) return 0;
        h = (h + 1) & (kSetSlots - 1);
    }
    return -1;
}

// ------------------------------------------------------------------------------ colour set
// grid (x: chunks of kChunk pixels, y: image). sets: [n][kSetSlots], cnt / over: [n], all zeroed.
// The workgroup's own set never fills: its threads stop inserting once it holds more than 256 keys,
// and at most 256 inserts are in flight then. The image's set can: 1024 other keys in it say "more
// than 256 colours" as well as the count does. over[i] != 0 or cnt[i] > 256: the cube.
__global__ __launch_bounds__(256) void k_gifw_colors(const Img* __restrict__ imgs, uint32_t* __restrict__ sets,
                                                     uint32_t* __restrict__ cnt, uint32_t* __restrict__ over) {
    __shared__ uint32_t s_set[kSetSlots];
    __shared__ uint32_t s_n, s_skip;
    const Img& I = imgs[blockIdx.y];
    const int64_t p0 = (int64_t)blockIdx.x * kChunk;
    if (I.status != kGifOk || I.g.mode == kGifwCube || p0 >= I.g.N) return;  // (uniform)
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_n = 0;
        s_skip = atomicOr(&over[blockIdx.y], 0u);  // another workgroup has settled it
    }
    for (int i = tid; i < kSetSlots; i += 256) s_set[i] = 0;
    __syncthreads();
    if (s_skip) return;
    const int64_t p1 = min(I.g.N, p0 + kChunk);
    const int d = I.g.d;
    uint32_t last = 0xFFFFFFFFu;
    for (int64_t p = p0 + tid; p < p1; p += 256) {
        const uint32_t key = gifw_key(I.src, d, p);
        if (key == last) continue;
        last = key;
        if (atomicOr(&s_n, 0u) > 256u) break;
        if (set_insert(s_set, key) == 1) atomicAdd(&s_n, 1u);
    }
    __syncthreads();
    if (s_n > 256u) {
        if (tid == 0) atomicOr(&over[blockIdx.y], 1u);
        return;
    }
    uint32_t* G = sets + (size_t)blockIdx.y * kSetSlots;
    for (int i = tid; i < kSetSlots; i += 256) {
        const uint32_t e = s_set[i];
        if (!e) continue;
        const int r = set_insert(G, e - 1u);
        if (r == 1) atomicAdd(&cnt[blockIdx.y], 1u);
        else if (r < 0) atomicOr(&over[blockIdx.y], 1u);
    }
}

// One workgroup per image. rank: [n][kSetSlots] bytes, the rank of the key in the set's slot.
__global__ __launch_bounds__(256) void k_gifw_palette(Img* __restrict__ imgs, const uint32_t* __restrict__ sets,
                                                      const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ over,
                                                      uint8_t* __restrict__ rank) {
    __shared__ uint32_t s_key[256];
    __shared__ uint16_t s_slot[256];
    __shared__ uint32_t s_k;
    Img& I = imgs[blockIdx.x];
    if (I.status != kGifOk) return;
    const int tid = threadIdx.x;
    const uint32_t n = cnt[blockIdx.x];
    const bool cube = I.g.mode == kGifwCube || over[blockIdx.x] != 0 || n > 256u;
    for (int i = tid; i < 768; i += 256) I.table[i] = 0;
    if (tid == 0) s_k = 0;
    __syncthreads();
    if (cube) {
        const uint32_t k = gifw_cube_entry(tid);
        I.table[3 * tid] = (uint8_t)(k >> 16);
        I.table[3 * tid + 1] = (uint8_t)(k >> 8);
        I.table[3 * tid + 2] = (uint8_t)k;
        if (tid == 0) {
            I.cube = 1;
            I.tb = 8;
            I.m = 8;
        }
        return;
    }
    const uint32_t* G = sets + (size_t)blockIdx.x * kSetSlots;
    for (int i = tid; i < kSetSlots; i += 256) {
        const uint32_t e = G[i];
        if (!e) continue;
        const uint32_t at = atomicAdd(&s_k, 1u);
        if (at < 256u) {  // (the set holds n <= 256 keys)
            s_key[at] = e - 1u;
            s_slot[at] = (uint16_t)i;
        }
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
        const uint32_t mine = s_key[tid];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; ++j) r += s_key[j] < mine;
        I.table[3 * r] = (uint8_t)(mine >> 16);
        I.table[3 * r + 1] = (uint8_t)(mine >> 8);
        I.table[3 * r + 2] = (uint8_t)mine;
        rank[(size_t)blockIdx.x * kSetSlots + s_slot[tid]] = (uint8_t)r;
    }
    if (tid == 0) {
        const int tb = gifw_table_bits((int)n);
        I.cube = 0;
        I.tb = tb;
        I.m = tb < 2 ? 2 : tb;
    }
}

// grid (x: chunks of kChunk pixels, y: image): thread t's 16 pixels -> 16 indices, one store.
__global__ __launch_bounds__(256) void k_gifw_index(const Img* __restrict__ imgs, const uint32_t* __restrict__ sets,
                                                    const uint8_t* __restrict__ rank, uint8_t* __restrict__ plane) {
    __shared__ uint32_t s_set[kSetSlots];
    __shared__ uint8_t s_rank[kSetSlots];
    const Img& I = imgs[blockIdx.y];
    const int64_t c0 = (int64_t)blockIdx.x * kChunk;
    if (I.status != kGifOk || c0 >= I.g.N) return;  // (uniform)
    const int tid = threadIdx.x;
    const bool cube = I.cube != 0;
    if (!cube) {
        for (int i = tid; i < kSetSlots; i += 256) {
            s_set[i] = sets[(size_t)blockIdx.y * kSetSlots + i];
            s_rank[i] = rank[(size_t)blockIdx.y * kSetSlots + i];
        }
    }
    __syncthreads();
    const int64_t N = I.g.N, c1 = min(N, c0 + kChunk);
    const int d = I.g.d, w = I.g.w, dither = I.g.dither;
    uint8_t* P = plane + I.plane_at;
    for (int64_t p0 = c0 + tid * 16; p0 < c1; p0 += 256 * 16) {
        uint8_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t p = p0 + j;
            uint32_t idx = 0;
            if (p < N) {
                const uint32_t key = gifw_key(I.src, d, p);
                if (cube) {
                    const int64_t y = p / w;
                    idx = (uint32_t)gifw_cube_index(key, (int)(p - y * w), (int)y, dither);
                } else {
                    uint32_t h = set_hash(key);
                    for (int k = 0; k < kSetSlots && s_set[h] != key + 1u; ++k) h = (h + 1) & (kSetSlots - 1);
                    idx = s_rank[h];
                }
            }
            v[j] = (uint8_t)idx;
        }
        uint4 q;
        __builtin_memcpy(&q, v, 16);
        *reinterpret_cast<uint4*>(P + p0) = q;  // (the plane's room is N rounded up to 16)
    }
}

// -------------------------------------------------------------------------------- LZW
// One wave per segment, structured like k_tiffw_lzw: every lane runs the same chain over the same
// indices, so its state is wave-uniform, and lane 0 alone stores into the dictionary and the code
// list. All lanes stage kLzwIn indices, free the dictionary after a table-full Clear, and after
// each staged tile place the codes: a wave sum scan of the widths gives each code its bit, the
// lanes OR them LSB-first into an LDS image of the stream's words, whole bytes go to the segment's
// room and the last partial byte is carried into the next tile's image.
// LDS: 32768 (dictionary) + 1024 (input) + 2064 (codes) + 2048 (words) = 37904 bytes per wave.
constexpr int kLzwIn = 1024;
constexpr int kLzwCodes = kLzwIn + 8;  // a tile's codes: one per index at most, the leading Clear, a table-full Clear, the last code, the closing Clear / stop
constexpr int kLzwWords = 512;         // 7 carried bits + kLzwCodes * 12 bits: under 388 words
// grid (x: segment of the image, y: image). bits: the segments' bit lengths.
__global__ __launch_bounds__(64) void k_gifw_lzw(const Img* __restrict__ imgs, const uint8_t* __restrict__ plane,
                                                 uint8_t* __restrict__ Z, unsigned long long* __restrict__ bits_out) {
    __shared__ uint32_t dict[kGifwLzwSlots];
    __shared__ uint32_t wbuf[kLzwWords];
    __shared__ uint16_t cbuf[kLzwCodes];  // code | (width - 3) << 12
    __shared__ uint8_t ibuf[kLzwIn];
    const Img& I = imgs[blockIdx.y];
    const int64_t s = blockIdx.x;
    if (I.status != kGifOk || s >= I.g.nseg) return;
    const int lane = threadIdx.x;
    const int64_t p0 = s * I.g.seg;
    const uint32_t S = (uint32_t)min(I.g.seg, I.g.N - p0);
    const uint8_t* in = plane + I.plane_at + p0;
    uint8_t* dst = Z + I.slot_at + s * I.slot;
    const uint32_t room = (uint32_t)I.slot;
    for (int i = lane; i < kGifwLzwSlots; i += 64) dict[i] = kGifwLzwFree;
    for (int i = lane; i < kLzwWords; i += 64) wbuf[i] = 0;
    wave_sync();
    int nc = 0;             // codes in cbuf
    uint32_t bits = 0;      // bits of wbuf in use (< 8 between tiles: the carried partial byte)
    uint32_t written = 0;   // bytes of the string already in dst
    unsigned long long length = 0;  // the string's bits so far
    auto sink = [&](uint32_t code, int width) {
        if (lane == 0) cbuf[nc] = (uint16_t)(code | (uint32_t)(width - 3) << 12);
        ++nc;
    };
    auto pack = [&](bool last) {  // the tile's codes into wbuf, its whole bytes out
        wave_sync();
        for (int i0 = 0; i0 < nc; i0 += 64) {
            const int i = i0 + lane;
            uint32_t code = 0, w = 0;
            if (i < nc) {
                const uint32_t e = cbuf[i];
                code = e & 0xFFFu;
                w = 3 + (e >> 12);
            }
            const uint32_t inc = wave_sum_scan(w, lane);
            if (w) {
                const uint32_t pos = bits + inc - w, wi = pos >> 5, sh = pos & 31;  // bits [sh, sh + w) from the word's bottom
                atomicOr(&wbuf[wi], code << sh);
                if (sh + w > 32) atomicOr(&wbuf[wi + 1], code >> (32 - sh));
            }
            bits += __shfl(inc, 63);
            length += __shfl(inc, 63);
        }
        wave_sync();
        const uint32_t nbytes = last ? (bits + 7) >> 3 : bits >> 3, nwords = (bits + 31) >> 5;
        for (uint32_t k = lane; k < nbytes; k += 64)
            if (written + k < room) dst[written + k] = (uint8_t)(wbuf[k >> 2] >> (8 * (k & 3)));
        const uint32_t rem = last ? 0u : bits & 7u;
        const uint32_t carry = rem ? (wbuf[nbytes >> 2] >> (8 * (nbytes & 3))) & 255u : 0u;
        wave_sync();
        for (uint32_t k = lane; k < nwords; k += 64) wbuf[k] = k == 0 ? carry : 0u;
        wave_sync();
        written += nbytes;
        bits = rem;
        nc = 0;
    };
    GifwLzw z;
    z.init(I.m);
    if (s == 0) z.begin(sink);
    for (uint32_t i0 = 0; i0 < S; i0 += kLzwIn) {
        const int cnt = (int)min((uint32_t)kLzwIn, S - i0);
        for (int k = lane; k < cnt; k += 64) ibuf[k] = in[i0 + k];
        wave_sync();
        for (int k = 0; k < cnt; ++k) {
            const uint32_t b = ibuf[k];
            if (z.feed(dict, b, sink, lane == 0)) {  // (wave-uniform)
                wave_sync();
                for (int i = lane; i < kGifwLzwSlots; i += 64) dict[i] = kGifwLzwFree;
                wave_sync();
            }
        }
        const bool last = i0 + kLzwIn >= S;
        if (last) z.finish(sink, s == I.g.nseg - 1);
        pack(last);
    }
    if (lane == 0) bits_out[I.seg0 + s] = length;
}

// ------------------------------------------------------------------------------- scan
// One workgroup per image: thread t sums its run of the segments' bit lengths, thread 0 turns the
// 256 sums into offsets, every thread rewrites its run as offsets. Then the sizes; when the file
// fits its slot the workgroup writes the head (signature .. code size byte), the terminator and
// the trailer as byte stores (the slot may start at any address). Otherwise nothing is written.
__global__ __launch_bounds__(256) void k_gifw_scan(Img* __restrict__ imgs, unsigned long long* __restrict__ bits,
                                                   uint64_t out_stride, uint64_t* __restrict__ sizes,
                                                   int32_t* __restrict__ status) {
    __shared__ unsigned long long s_sum[256];
    __shared__ int s_st;
    Img& I = imgs[blockIdx.x];
    const int tid = threadIdx.x;
    if (I.status != kGifOk) {  // (uniform)
        if (tid == 0) {
            sizes[blockIdx.x] = 0;
            status[blockIdx.x] = I.status;
        }
        return;
    }
    const int64_t nseg = I.g.nseg, per = (nseg + 255) / 256;
    const int64_t a = min(nseg, (int64_t)tid * per), b = min(nseg, a + per);
    unsigned long long* B = bits + I.seg0;
    unsigned long long run = 0;
    for (int64_t k = a; k < b; ++k) run += B[k];
    s_sum[tid] = run;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < 256; ++k) {
            const unsigned long long v = s_sum[k];
            s_sum[k] = t;
            t += v;
        }
        const uint64_t P = (t + 7) / 8, total = gifw_file_size(I.tb, P);
        const uint64_t room = gifw_payload_bound((uint64_t)I.g.N, (uint64_t)I.g.nseg);
        s_st = P > room ? kInternal : total > out_stride ? kGifTooLarge : kGifOk;  // (the bound is proven: never kInternal)
        I.total_bits = t;
        I.payload = P;
        I.status = s_st;
        sizes[blockIdx.x] = s_st == kInternal ? 0 : total;
        status[blockIdx.x] = s_st;
    }
    __syncthreads();
    run = s_sum[tid];
    for (int64_t k = a; k < b; ++k) {
        const unsigned long long v = B[k];
        B[k] = run;
        run += v;
    }
    if (s_st != kGifOk) return;
    const uint32_t head = (uint32_t)gifw_head_size(I.tb);
    uint8_t* o = I.out;
    for (uint32_t i = tid; i < head; i += 256) o[i] = (uint8_t)gifw_head_byte(i, I.g.w, I.g.h, I.tb, I.m, I.table);
    if (tid == 0) {
        const uint64_t end = head + gifw_data_size(I.payload);
        o[end] = 0;
        o[end + 1] = ';';
    }
}

// ------------------------------------------------------------------------------- merge
// grid (x: chunks of kChunk bytes of the data area, y: image). Byte q of the data area is a
// sub-block length or payload byte j; payload byte j holds stream bits [8j, 8j + 8): those of the
// segment s that holds bit 8j, from its room at bit 8j - off[s], and -- where s ends inside the
// byte -- the first bits of the segments after it, shifted to where they start. (A segment but the
// last is 8 bits or more, so at most one follows; the loop takes what comes.) A thread's bytes
// ascend, so the segment it found last is tried first, then its successor, then a bisection.
__global__ __launch_bounds__(256) void k_gifw_merge(const Img* __restrict__ imgs, const unsigned long long* __restrict__ bits,
                                                    const uint8_t* __restrict__ Z) {
    const Img& I = imgs[blockIdx.y];
    if (I.status != kGifOk) return;
    const uint64_t P = I.payload, D = gifw_data_size(P), q0 = (uint64_t)blockIdx.x * kChunk;
    if (q0 >= D) return;
    const unsigned long long* off = bits + I.seg0;
    const int64_t nseg = I.g.nseg;
    const unsigned long long total = I.total_bits;
    const uint8_t* R = Z + I.slot_at;
    const int64_t slot = I.slot;
    auto end_of = [&](int64_t s) { return s + 1 < nseg ? off[s + 1] : total; };
    int64_t s = 0;
    auto payload = [&](uint64_t j) -> uint32_t {
        const unsigned long long b0 = 8ull * j;
        if (!(off[s] <= b0 && b0 < end_of(s))) {
            if (s + 1 < nseg && off[s + 1] <= b0 && b0 < end_of(s + 1)) {
                ++s;
            } else {
                int64_t lo = 0, hi = nseg - 1;  // the last segment with off <= b0
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (off[mid] <= b0) lo = mid;
                    else hi = mid - 1;
                }
                s = lo;
            }
        }
        const unsigned long long r = b0 - off[s], len = end_of(s) - off[s];
        const uint8_t* A = R + s * slot;
        const unsigned long long B = r >> 3;
        const uint32_t lo8 = A[B], hi8 = (B + 1) * 8 < len ? A[B + 1] : 0u;
        uint32_t v = ((lo8 | hi8 << 8) >> (r & 7)) & 255u;
        for (int64_t t = s + 1; t < nseg && off[t] < b0 + 8; ++t) v |= ((uint32_t)R[t * slot] << (off[t] - b0)) & 255u;
        return v;
    };
    const int nb = (int)min((uint64_t)kChunk, D - q0);
    store_segment(I.out + gifw_head_size(I.tb) + q0, nb, threadIdx.x,
                  [&](int q) { return gifw_data_byte(q0 + (uint64_t)q, P, payload); });
}

}  // namespace gifw

// Grow-only device buffers of one context's GIF writes (icx_ctx::gifw).
struct GifwWs {
    Buf<uint8_t> tables, plane, payload;
};
GifwWs* gifw_ws_create() { return new GifwWs(); }
void gifw_ws_destroy(GifwWs* w) { delete w; }

int gifw_encode_batch(hipStream_t st, GifwWs& ws, int n, const uint8_t* const* d_src, const int32_t* widths,
                      const int32_t* heights, int d, int segment_pixels, int dither, int palette_mode, uint8_t* d_out,
                      uint64_t out_stride, uint64_t* d_sizes, int32_t* d_status, std::string& err) {
    using namespace gifw;
    const char* name = "icx_gif_encode_device_batch";
    std::vector<Img> imgs((size_t)n);
    int64_t nseg = 0, plane_at = 0, slot_at = 0, max_n = 1, max_seg = 1;
    uint64_t max_data = 1;
    for (int i = 0; i < n; ++i) {
        Img& I = imgs[i];
        I = Img{};
        I.src = d_src[i];
        I.out = d_out + (uint64_t)i * out_stride;
        I.status = I.src && gifw_geom(widths[i], heights[i], d, segment_pixels, dither, palette_mode, &I.g) ? kGifOk : kGifInvalidArgument;
        if (I.status != kGifOk) continue;
        I.seg0 = nseg;
        I.plane_at = plane_at;
        I.slot_at = slot_at;
        I.slot = (int64_t)((gifw_segment_room((uint64_t)I.g.seg) + 15) & ~15ull);
        nseg += I.g.nseg;
        plane_at += (I.g.N + 15) & ~(int64_t)15;
        slot_at += I.slot * I.g.nseg;
        max_n = std::max(max_n, I.g.N);
        max_seg = std::max(max_seg, I.g.nseg);
        max_data = std::max(max_data, gifw_data_size(gifw_payload_bound((uint64_t)I.g.N, (uint64_t)I.g.nseg)));
        if (nseg > (1ll << 28)) {
            (err = name) += ": too many segments in one call";
            return -1;
        }
    }
    size_t tat = 0;
    auto take = [&](size_t bytes) {
        const size_t o = tat;
        tat += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_img = take(sizeof(Img) * (size_t)n), o_bits = take(sizeof(unsigned long long) * (size_t)std::max<int64_t>(nseg, 1)),
                 o_rank = take((size_t)kSetSlots * (size_t)n), o_zero = tat, o_set = take(sizeof(uint32_t) * kSetSlots * (size_t)n),
                 o_cnt = take(sizeof(uint32_t) * (size_t)n), o_over = take(sizeof(uint32_t) * (size_t)n);
    if (!ws.tables.reserve(tat) || !ws.plane.reserve((size_t)std::max<int64_t>(plane_at, 64)) ||
        !ws.payload.reserve((size_t)std::max<int64_t>(slot_at, 64))) {
        (err = name) += ": allocation: ";
        err += hipGetErrorString(hipGetLastError());
        return -1;
    }
    uint8_t* A = ws.tables.p;
    Img* d_img = reinterpret_cast<Img*>(A + o_img);
    unsigned long long* d_bits = reinterpret_cast<unsigned long long*>(A + o_bits);
    uint8_t* d_rank = A + o_rank;
    uint32_t* d_set = reinterpret_cast<uint32_t*>(A + o_set);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(A + o_cnt);
    uint32_t* d_over = reinterpret_cast<uint32_t*>(A + o_over);
    if (hipMemcpyAsync(d_img, imgs.data(), sizeof(Img) * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(A + o_zero, 0, tat - o_zero, st) != hipSuccess) {
        (err = name) += ": copy: ";
        err += hipGetErrorString(hipGetLastError());
        return -1;
    }
    const dim3 pix((unsigned)((max_n + kChunk - 1) / kChunk), (unsigned)n);
    if (nseg > 0) {
        if (palette_mode != kGifwCube) hipLaunchKernelGGL(k_gifw_colors, pix, dim3(256), 0, st, d_img, d_set, d_cnt, d_over);
        hipLaunchKernelGGL(k_gifw_palette, dim3((unsigned)n), dim3(256), 0, st, d_img, d_set, d_cnt, d_over, d_rank);
        hipLaunchKernelGGL(k_gifw_index, pix, dim3(256), 0, st, d_img, d_set, d_rank, ws.plane.p);
        hipLaunchKernelGGL(k_gifw_lzw, dim3((unsigned)max_seg, (unsigned)n), dim3(64), 0, st, d_img, ws.plane.p, ws.payload.p, d_bits);
    }
    hipLaunchKernelGGL(k_gifw_scan, dim3((unsigned)n), dim3(256), 0, st, d_img, d_bits, out_stride, d_sizes, d_status);
    if (nseg > 0)
        hipLaunchKernelGGL(k_gifw_merge, dim3((unsigned)((max_data + kChunk - 1) / kChunk), (unsigned)n), dim3(256), 0, st, d_img,
                           d_bits, ws.payload.p);
    return encode_finish(name, st, err);
}

}  // namespace icx
