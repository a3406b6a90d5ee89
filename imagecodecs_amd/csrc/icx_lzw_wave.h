// icx_lzw_wave.h -- the three wave-level helpers the GIF and TIFF LZW kernels (icx_gif.hip
// k_gif_lzw, icx_tiff.hip k_tiff_unpack) have in common, moved here unchanged from icx_gif.hip
// (hence the names): ordering LDS traffic inside one wave, staging file bytes through an LDS
// window, and a wave-wide inclusive sum. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icx {

__device__ __forceinline__ void gif_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// win[0, len) = file bytes [base, base + len), zero outside [0, fsize). d + base is 16-byte
// aligned, len a multiple of 16, win 16-byte aligned. Bytes outside the file are never read.
__device__ __forceinline__ void gif_fill(uint8_t* win, const uint8_t* d, int64_t fsize, int64_t base, int len, int lane) {
    for (int o = lane * 16; o < len; o += 64 * 16) {
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

__device__ __forceinline__ uint32_t gif_wave_sum_scan(uint32_t v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(v, s);
        if (lane >= s) v += t;
    }
    return v;
}

}  // namespace icx
