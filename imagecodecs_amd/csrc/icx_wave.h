// icx_wave.h -- the device building blocks the format kernels (TGA, BMP, Netpbm, GIF, TIFF, HDR)
// share: ordering LDS traffic inside one wave, staging file bytes through an LDS window, wave-wide
// inclusive scans, and storing a row segment at the destination's 16-byte alignment. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icx {

// What the wave's lanes wrote to LDS before is visible to every lane after.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// win[0, len) = file bytes [base, base + len), zero outside [0, fsize). d + base is 16-byte
// aligned, len a multiple of 16, win 16-byte aligned. Bytes outside the file are never read.
// Thread tid of nthreads takes every nthreads-th 16-byte chunk.
__device__ __forceinline__ void fill_window(uint8_t* win, const uint8_t* d, int64_t fsize, int64_t base, int len, int tid,
                                            int nthreads) {
    for (int o = tid * 16; o < len; o += nthreads * 16) {
        const int64_t a = base + o;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a >= 0 && a + 16 <= fsize) {
            v = *reinterpret_cast<const uint4*>(d + a);
        } else {
            uint32_t t[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16; ++b)
                if (a + b >= 0 && a + b < fsize) t[b >> 2] |= (uint32_t)d[a + b] << (8 * (b & 3));
            v = make_uint4(t[0], t[1], t[2], t[3]);
        }
        *reinterpret_cast<uint4*>(win + o) = v;
    }
}

// Inclusive scans over the 64 lanes of a wave.
template <class T>
__device__ __forceinline__ T wave_sum_scan(T v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T t = __shfl_up(v, s);
        if (lane >= s) v += t;
    }
    return v;
}
__device__ __forceinline__ int wave_max_scan(int v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(v, s);
        if (lane >= s) v = max(v, t);
    }
    return v;
}

// optr[q] = byte_at(q) for q in [0, nb), by the 256 threads of a workgroup: single bytes up to
// optr's 16-byte boundary, 16-byte stores of 16 assembled bytes, single bytes after.
template <class ByteAt>
__device__ __forceinline__ void store_segment(uint8_t* optr, int nb, int tid, ByteAt byte_at) {
    const int head = min(nb, (int)((16 - (reinterpret_cast<uintptr_t>(optr) & 15)) & 15));
    const int nv = (nb - head) / 16;
    for (int v = tid; v < nv; v += 256) {
        const int b0 = head + 16 * v;
        uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) wd[b >> 2] |= byte_at(b0 + b) << (8 * (b & 3));
        *reinterpret_cast<uint4*>(optr + b0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    const int tail0 = head + 16 * nv;
    for (int b = tid; b < head + (nb - tail0); b += 256) {
        const int q = b < head ? b : tail0 + (b - head);
        optr[q] = (uint8_t)byte_at(q);
    }
}

}  // namespace icx
