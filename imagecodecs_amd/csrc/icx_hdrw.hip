// icx_hdrw.hip -- Radiance .hdr (RGBE) write on gfx950: Image::writeHdr (codecs.cpp:779-818) by the
// contract of include/icx.h ("Radiance .hdr write"); the arithmetic is icx_hdrw_core.h.
//
// Flat files (what the reference writes) are one streaming kernel:
//   k_hdrw_flat      float pixels -> RGBE, straight into the file. The payload starts after a header
//                    of 59+ bytes, so its pixels are rarely dword aligned: a lane owns one 16-byte
//                    aligned chunk of the *file*, converts the 4 (5 when the payload is not dword
//                    aligned) pixels that touch it, shifts their dwords into place with alignbyte
//                    and leaves one 16-byte store. Only the first and last chunk of an image are
//                    written byte by byte.
// Run-length coded files (rle != 0 and 8 <= w <= 32767) go through component planes:
//   k_hdrw_planes    float pixels -> the rows' R, G, B, E planes (4 pixels per lane, dword stores)
//   k_hdrw_sizes     one wave per (row, component): the packed size of that plane
//   k_hdrw_prefix    one wave per image: row sizes -> the offset of every packed plane in the file;
//                    the file's size, status and header (flat files too). Each image is scanned on
//                    its own.
//   k_hdrw_emit      one wave per (row, component): the packets, and the row's 2, 2, hi, lo marker
// hdrw_rle_plane is hdrw_pack_plane in parallel form (the derivation is at the function).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "icx_hdrw_core.h"
#include "icx_internal.h"
#include "icx_mem.h"
#include "icx_wave.h"

namespace icx {

struct HdrwJob {
    const float* src;
    int32_t w, h;
    int32_t status;
    int32_t packed;   // the rows are run-length coded
    int32_t head;     // header bytes
    int32_t wp;       // plane pitch: w rounded up to 4
    uint64_t row0;    // the image's first row in HdrwWs::psz / poff (packed images)
    uint64_t plane0;  // the image's first byte in HdrwWs::planes
};

template <int D>
struct alignas(4) HdrwPx {
    float v[D];
};

// Pixel q of the image. A16: d = 4 and a 16-byte aligned base, one float4 load; otherwise D floats
// from a dword-aligned pixel. Loading and converting are apart so that a lane's loads are all
// issued before the first conversion waits for one.
template <int D, bool A16>
__device__ __forceinline__ HdrwPx<4> hdrw_load_px(const float* src, int64_t q) {
    HdrwPx<4> r;
    r.v[3] = 0.f;
    if (D == 4 && A16) {
        const float4 t = reinterpret_cast<const float4*>(src)[q];
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        const HdrwPx<D> t = reinterpret_cast<const HdrwPx<D>*>(src)[q];
#pragma unroll
        for (int c = 0; c < D; ++c) r.v[c] = t.v[c];
    }
    return r;
}
// ... as RGBE, R in the low byte.
template <int D>
__device__ __forceinline__ uint32_t hdrw_to_rgbe(const HdrwPx<4>& p) {
    return D == 4 ? hdrw_rgbe4(p.v) : hdrw_rgbe3(p.v);
}

// The flat payload of one image: chunk c is the 16 aligned bytes of the file that hold payload
// bytes [16c - lead, 16c - lead + 16), lead = the payload's address mod 16. Its first pixel is
// q0 = 4c - ceil(lead / 4) and the chunk starts `sh` bytes into that pixel.
template <int D, bool A16>
__device__ __forceinline__ void hdrw_flat_image(const HdrwJob& J, uint8_t* file) {
    uint8_t* const P = file + J.head;
    const int64_t npix = (int64_t)J.w * J.h, nbytes = 4 * npix;
    const int lead = (int)(reinterpret_cast<uintptr_t>(P) & 15);
    const int back = (lead + 3) >> 2;
    const uint32_t sh = (uint32_t)(4 * back - lead);
    const int64_t nch = (lead + nbytes + 15) >> 4;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q0 = 4 * c - back, b0 = 16 * c - lead;
        // (an index outside the image is clamped into it: those bytes are never stored)
        HdrwPx<4> px[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = hdrw_load_px<D, A16>(J.src, min<int64_t>(max<int64_t>(q0 + k, 0), npix - 1));
        if (sh) px[4] = hdrw_load_px<D, A16>(J.src, min<int64_t>(q0 + 4, npix - 1));  // uniform per image
        uint32_t v[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = hdrw_to_rgbe<D>(px[k]);
        v[4] = sh ? hdrw_to_rgbe<D>(px[4]) : 0u;
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = sh ? __builtin_amdgcn_alignbyte(v[k + 1], v[k], sh) : v[k];
        if (b0 >= 0 && b0 + 16 <= nbytes) {
            *reinterpret_cast<uint4*>(P + b0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b0 + b >= 0 && b0 + b < nbytes) P[b0 + b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// grid (x: chunks of 256 lanes, y: image)
template <int D>
__global__ __launch_bounds__(256) void k_hdrw_flat(const HdrwJob* __restrict__ jobs, uint8_t* __restrict__ out,
                                                   uint64_t out_stride) {
    const HdrwJob J = jobs[blockIdx.y];
    if (J.status != kHdrwOk || J.packed) return;
    uint8_t* file = out + (uint64_t)blockIdx.y * out_stride;
    if (D == 4 && (reinterpret_cast<uintptr_t>(J.src) & 15) == 0) hdrw_flat_image<D, true>(J, file);  // uniform per image
    else hdrw_flat_image<D, false>(J, file);
}

// Rows of one image -> their component planes: row y's four planes of pitch wp at plane0 + 4*wp*y.
// A lane takes 4 pixels and stores one dword per plane (pixels past the row end are zero bytes in
// the pitch's padding).
template <int D, bool A16>
__device__ __forceinline__ void hdrw_planes_image(const HdrwJob& J, uint8_t* planes) {
    const int w = J.w, wp = J.wp;
    for (int y = blockIdx.x; y < J.h; y += gridDim.x) {
        const int64_t q0 = (int64_t)y * w;
        uint8_t* pr = planes + J.plane0 + (uint64_t)y * 4 * wp;
        for (int x = threadIdx.x * 4; x < w; x += blockDim.x * 4) {
            HdrwPx<4> px[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = hdrw_load_px<D, A16>(J.src, q0 + min(x + k, w - 1));
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = x + k < w ? hdrw_to_rgbe<D>(px[k]) : 0u;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t word = ((v[0] >> (8 * c)) & 255u) | ((v[1] >> (8 * c)) & 255u) << 8 |
                                      ((v[2] >> (8 * c)) & 255u) << 16 | ((v[3] >> (8 * c)) & 255u) << 24;
                *reinterpret_cast<uint32_t*>(pr + (int64_t)c * wp + x) = word;
            }
        }
    }
}

// grid (x: rows, y: image)
template <int D>
__global__ __launch_bounds__(256) void k_hdrw_planes(const HdrwJob* __restrict__ jobs, uint8_t* __restrict__ planes) {
    const HdrwJob J = jobs[blockIdx.y];
    if (J.status != kHdrwOk || !J.packed) return;
    if (D == 4 && (reinterpret_cast<uintptr_t>(J.src) & 15) == 0) hdrw_planes_image<D, true>(J, planes);
    else hdrw_planes_image<D, false>(J, planes);
}

// The highest set bit of m at or below this lane as a position of the chunk at c0, or `carry`.
__device__ __forceinline__ int hdrw_last_flag(uint64_t m, uint64_t le, int c0, int carry) {
    const uint64_t t = m & le;
    return t ? c0 + 63 - __clzll((long long)t) : carry;
}

// hdrw_pack_plane in parallel form, one wave per plane, 64 bytes at a time. A stretch of equal
// bytes is cut into blocks of 127 from its start; with j = a byte's offset in its block, the block
// is a run packet when it has 4 bytes or more and literal bytes otherwise (only a stretch's last
// block can be short). A byte with j >= 3 is in a run; one with j < 3 is in a run exactly when the
// bytes up to its block's fourth are equal and inside the row, which the next 3 bytes tell. Literal
// bytes that touch form a zone, cut into packets of 128 from its start. A run packet is written by
// its block's last byte, a literal packet's count by its last byte; both know the length. Sizes are
// attributed the same way (2 at a run's last byte, 1 per literal byte, 1 more where a literal
// packet starts), so one prefix sum gives every position. Every per-byte fact is a flag, so the
// three scans (stretch start, zone start, size) are ballots: the last flag at or below a lane is
// a count of leading zeros, the prefix sum three population counts. Returns the plane's bytes.
template <bool EMIT>
__device__ __forceinline__ uint32_t hdrw_rle_plane(const uint8_t* p, int w, uint8_t* out, int lane) {
    const uint64_t le = ~0ull >> (63 - lane);  // lanes 0 .. lane
    int s_carry = 0, ls_carry = -1;
    uint64_t lit_carry = 0;
    uint32_t last = 256, bytes = 0;
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int k = c0 + lane;
        const bool valid = k < w;
        uint32_t b[5];  // p[k .. k+4]; past the row end a value no byte equals
#pragma unroll
        for (int i = 0; i < 5; ++i) b[i] = k + i < w ? p[k + i] : 256u;
        uint32_t prev = __shfl_up(b[0], 1);
        if (lane == 0) prev = last;
        const uint64_t m_start = __ballot(valid && prev != b[0]);  // stretch starts
        const int s = hdrw_last_flag(m_start, le, c0, s_carry);
        const int j = (k - s) % 127;
        const bool e1 = b[1] == b[0], e2 = e1 && b[2] == b[0], e3 = e2 && b[3] == b[0];
        const bool run = valid && (j >= 3 || (j == 2 ? e1 : j == 1 ? e2 : e3));
        const bool lit = valid && !run;
        // the same for byte k + 1
        const int j1 = e1 && j != 126 ? j + 1 : 0;
        const bool f1 = b[2] == b[1], f2 = f1 && b[3] == b[1], f3 = f2 && b[4] == b[1];
        const bool lit1 = k + 1 < w && !(j1 >= 3 || (j1 == 2 ? f1 : j1 == 1 ? f2 : f3));
        const bool run_end = run && (j == 126 || !e1);
        const uint64_t m_lit = __ballot(lit);
        const uint64_t m_zone = m_lit & ~(m_lit << 1 | lit_carry);  // literal bytes after a byte that is none
        const int ls = hdrw_last_flag(m_zone, le, c0, ls_carry);
        const int lo = (k - ls) & 127;
        const uint64_t m_head = __ballot(lit && lo == 0), m_end = __ballot(run_end);
        const uint32_t incl = bytes + __popcll(m_lit & le) + __popcll(m_head & le) + 2 * __popcll(m_end & le);
        if (EMIT) {
            if (lit) {
                out[incl - 1] = (uint8_t)b[0];
                if (lo == 127 || !lit1) out[incl - (lo + 1) - 1] = (uint8_t)(lo + 1);
            } else if (run_end) {
                out[incl - 2] = (uint8_t)(128 + j + 1);
                out[incl - 1] = (uint8_t)b[0];
            }
        }
        s_carry = hdrw_last_flag(m_start, ~0ull, c0, s_carry);
        ls_carry = hdrw_last_flag(m_zone, ~0ull, c0, ls_carry);
        lit_carry = m_lit >> 63;
        last = __shfl(b[0], 63);
        bytes += __popcll(m_lit) + __popcll(m_head) + 2 * __popcll(m_end);
    }
    return bytes;
}

// grid (x: groups of 4 planes, y: image); plane t = 4*row + component
__global__ __launch_bounds__(256) void k_hdrw_sizes(const HdrwJob* __restrict__ jobs, const uint8_t* __restrict__ planes,
                                                    uint32_t* __restrict__ psz) {
    const HdrwJob J = jobs[blockIdx.y];
    if (J.status != kHdrwOk || !J.packed) return;
    const int lane = threadIdx.x & 63;
    const int64_t nt = 4 * (int64_t)J.h;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += (int64_t)gridDim.x * 4) {
        const uint32_t n = hdrw_rle_plane<false>(planes + J.plane0 + (uint64_t)t * J.wp, J.w, nullptr, lane);
        if (lane == 0) psz[4 * J.row0 + t] = n;
    }
}

// One wave per image: plane sizes -> plane offsets in the file; size, status and header.
__global__ __launch_bounds__(64) void k_hdrw_prefix(HdrwJob* __restrict__ jobs, const uint32_t* __restrict__ psz,
                                                    uint64_t* __restrict__ poff, uint8_t* __restrict__ out,
                                                    uint64_t out_stride, uint64_t* __restrict__ sizes,
                                                    int32_t* __restrict__ status) {
    const int i = blockIdx.x, lane = threadIdx.x;
    HdrwJob& J = jobs[i];
    if (J.status != kHdrwOk) {
        if (lane == 0) { sizes[i] = 0; status[i] = J.status; }
        return;
    }
    uint64_t total = (uint64_t)J.head;
    if (!J.packed) {
        total += 4 * (uint64_t)J.w * J.h;
    } else {
        for (int y0 = 0; y0 < J.h; y0 += 64) {
            const int y = y0 + lane;
            uint32_t s[4] = {0, 0, 0, 0};
            if (y < J.h)
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = psz[4 * (J.row0 + y) + c];
            const uint64_t v = y < J.h ? 4ull + s[0] + s[1] + s[2] + s[3] : 0;
            const uint64_t incl = wave_sum_scan(v, lane);
            if (y < J.h) {
                uint64_t at = total + incl - v + 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    poff[4 * (J.row0 + y) + c] = at;
                    at += s[c];
                }
            }
            total += __shfl(incl, 63);
        }
    }
    if (lane == 0) {
        const bool fits = total <= out_stride;
        sizes[i] = total;
        status[i] = fits ? kHdrwOk : kHdrwTooLarge;
        if (fits) hdrw_write_header(out + (uint64_t)i * out_stride, J.w, J.h);
        else J.status = kHdrwTooLarge;  // k_hdrw_emit / k_hdrw_flat skip it
    }
}

__global__ __launch_bounds__(256) void k_hdrw_emit(const HdrwJob* __restrict__ jobs, const uint8_t* __restrict__ planes,
                                                   const uint64_t* __restrict__ poff, uint8_t* __restrict__ out,
                                                   uint64_t out_stride) {
    const HdrwJob J = jobs[blockIdx.y];
    if (J.status != kHdrwOk || !J.packed) return;
    const int lane = threadIdx.x & 63;
    uint8_t* file = out + (uint64_t)blockIdx.y * out_stride;
    const int64_t nt = 4 * (int64_t)J.h;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += (int64_t)gridDim.x * 4) {
        uint8_t* o = file + poff[4 * J.row0 + t];
        if ((t & 3) == 0 && lane < 4) o[lane - 4] = (uint8_t)(lane < 2 ? 2 : lane == 2 ? J.w >> 8 : J.w & 255);
        hdrw_rle_plane<true>(planes + J.plane0 + (uint64_t)t * J.wp, J.w, o, lane);
    }
}

// ------------------------------------------------------------------------------- host
struct HdrwWs {
    Buf<HdrwJob> jobs;
    Buf<uint8_t> planes;
    Buf<uint32_t> psz;
    Buf<uint64_t> poff;
};
HdrwWs* hdrw_ws_create() { return new HdrwWs(); }
void hdrw_ws_destroy(HdrwWs* w) { delete w; }

int hdr_encode_batch(hipStream_t st, HdrwWs& ws, int n, const float* const* d_src, const int32_t* widths,
                     const int32_t* heights, int d, int rle, uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes,
                     int32_t* d_status, std::string& err) {
    std::vector<HdrwJob> jobs((size_t)n);
    uint64_t rows = 0, plane_bytes = 0;
    int max_h_packed = 0;
    int64_t max_flat_px = 0;
    for (int i = 0; i < n; ++i) {
        HdrwJob& J = jobs[i];
        J = HdrwJob{};
        J.src = d_src[i];
        J.w = widths[i];
        J.h = heights[i];
        J.status = J.src && hdrw_args_ok(J.w, J.h, d) ? kHdrwOk : kHdrwInvalidArgument;
        if (J.status != kHdrwOk) continue;
        J.head = hdrw_header_len(J.w, J.h);
        J.packed = hdrw_row_rle(J.w, rle);
        if (!J.packed) {
            max_flat_px = std::max(max_flat_px, (int64_t)J.w * J.h);
            continue;
        }
        J.wp = (J.w + 3) & ~3;
        J.row0 = rows;
        J.plane0 = plane_bytes;
        rows += (uint64_t)J.h;
        plane_bytes += 4ull * J.wp * J.h;
        max_h_packed = std::max(max_h_packed, J.h);
    }
    const bool rest = ws.planes.reserve(plane_bytes) && ws.psz.reserve(rows * 16) && ws.poff.reserve(rows * 32);
    if (jobs_upload("hdr_encode_batch", ws.jobs, jobs, st, err, rest)) return -1;
    const int cap = std::max(1, 16384 / std::min(n, 16384));  // blocks per image
    const dim3 g_rows(std::max(1, std::min(max_h_packed, cap)), n), g_planes(std::max(1, std::min(max_h_packed, cap)), n);
    if (max_h_packed) {
        if (d == 4) hipLaunchKernelGGL(k_hdrw_planes<4>, g_rows, dim3(256), 0, st, ws.jobs.p, ws.planes.p);
        else hipLaunchKernelGGL(k_hdrw_planes<3>, g_rows, dim3(256), 0, st, ws.jobs.p, ws.planes.p);
        hipLaunchKernelGGL(k_hdrw_sizes, g_planes, dim3(256), 0, st, ws.jobs.p, ws.planes.p, ws.psz.p);
    }
    hipLaunchKernelGGL(k_hdrw_prefix, dim3(n), dim3(64), 0, st, ws.jobs.p, ws.psz.p, ws.poff.p, d_out, out_stride, d_sizes,
                       d_status);
    if (max_h_packed)
        hipLaunchKernelGGL(k_hdrw_emit, g_planes, dim3(256), 0, st, ws.jobs.p, ws.planes.p, ws.poff.p, d_out, out_stride);
    if (max_flat_px) {
        const int64_t blocks = (max_flat_px / 4 + 2 + 255) / 256;  // 4 pixels per lane and the two end chunks
        const dim3 g_flat((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, cap)), n);
        if (d == 4) hipLaunchKernelGGL(k_hdrw_flat<4>, g_flat, dim3(256), 0, st, ws.jobs.p, d_out, out_stride);
        else hipLaunchKernelGGL(k_hdrw_flat<3>, g_flat, dim3(256), 0, st, ws.jobs.p, d_out, out_stride);
    }
    return encode_finish("hdr_encode_batch", st, err);
}

}  // namespace icx
