// icx_lzw_wave.h -- one round of the wave LZW decoder: 64 lanes hold 64 consecutive codes of one
// stretch between two clear codes. Written for the two formats that decode LZW this way: GIF
// (icx_gif.hip k_gif_lzw) is built from these pieces; TIFF (icx_tiff.hip tiff_lzw_wave) is the same
// round line for line but keeps it written out. A caller keeps its own outer loop, input
// staging, code fetch (LSB first from a ring / MSB first from a window) and event handling (clear,
// stop, invalid, missing code); it hands the lanes before the first event (`act`) to
//   lzw_resolve  string length and first byte of every code, from the table or -- for entries made by
//                the same 64 codes -- by pointer doubling over the lanes; a wave scan gives every
//                string its place in the output, `need` the lanes that start before the output's end
//   lzw_enter    the table entries those codes make
//   lzw_walk     a lane's own chain back to front, each byte handed to the caller's put(k, byte)
//   lzw_carry    what the next round needs to know of this one
// The table is the classic one: tab[e] = prefix code | suffix << 12 | string length << 20 (16 KiB) and
// first[e] = the string's first byte (4 KiB). Code number t >= 1 after a clear makes entry
// clear + 1 + t from code t - 1 and its own first byte. Device code only.
#pragma once
#include "icx_wave.h"

namespace icx {

struct LzwCarry {
    uint32_t base = 0;                 // output bytes produced
    int prev_code = 0, prev_F = 0;     // of code t0 - 1 (t0 > 0)
    uint32_t prev_L = 0;
};

struct LzwRound {
    uint32_t L, incl, excl;  // the lane's string length, and its inclusive / exclusive sum over the lanes
    uint32_t rem;            // output bytes still missing before this round
    int F;                   // the string's first byte
    bool need;               // the code starts before the last output byte: a prefix of the lanes
    int m;                   // how many lanes that is
    __device__ __forceinline__ uint32_t cut() const { return min(L, rem - excl); }  // string bytes inside the output
};

// t0: the number of lane 0's code after the last clear; want: the output's length.
__device__ __forceinline__ LzwRound lzw_resolve(int code, bool act, uint32_t t0, int clear, uint32_t want, const LzwCarry& C,
                                                const uint32_t* tab, const uint8_t* first, int lane) {
    const int j = code - (clear + 2);  // the code's entry was made from code number j and its successor
    uint32_t A = 0;
    int D = -1, F = 0;
    if (act) {
        if (code < clear) { A = 1; F = code; }
        else if ((uint32_t)j >= t0) { A = 1; D = (int)((uint32_t)j - t0); }      // made by this round's codes: a lower lane
        else if ((uint32_t)j + 1 == t0) { A = C.prev_L + 1; F = C.prev_F; }      // made by lane 0 of this round
        else { A = tab[code] >> 20; F = first[code]; }
    }
    while (__any(D >= 0)) {
        const int src = D < 0 ? lane : D;
        const uint32_t a2 = __shfl(A, src);
        const int f2 = __shfl(F, src), d2 = __shfl(D, src);
        if (D >= 0) { A += a2; F = f2; D = d2; }
    }
    LzwRound R;
    R.L = A;
    R.F = F;
    R.incl = wave_sum_scan(R.L, lane);
    R.excl = R.incl - R.L;
    R.rem = want - C.base;
    R.need = act && R.excl < R.rem;
    R.m = __popcll(__ballot(R.need));
    return R;
}

// t = t0 + lane. Ends with the entries visible to every lane.
__device__ __forceinline__ void lzw_enter(const LzwRound& R, int code, uint32_t t, int clear, const LzwCarry& C, uint32_t* tab,
                                          uint8_t* first, int lane) {
    int pc = __shfl_up(code, 1), pF = __shfl_up(R.F, 1);
    uint32_t pL = __shfl_up(R.L, 1);
    if (lane == 0) { pc = C.prev_code; pF = C.prev_F; pL = C.prev_L; }
    if (R.need && t >= 1 && (uint32_t)clear + 1 + t < 4096u) {
        tab[clear + 1 + t] = (uint32_t)pc | (uint32_t)(R.F & 255) << 12 | (pL + 1) << 20;
        first[clear + 1 + t] = (uint8_t)pF;
    }
    wave_sync();
}

// For a lane with R.need: put(k, byte k of the code's string) for k = L - 1 .. 0.
template <class Put>
__device__ __forceinline__ void lzw_walk(const LzwRound& R, int code, const uint32_t* tab, Put put) {
    int c = code;
    for (uint32_t k = R.L - 1;; --k) {
        int s = c;
        if (k > 0) {
            const uint32_t e = tab[c];
            s = (e >> 12) & 255;
            c = e & 0xFFF;
        }
        put(k, s);
        if (k == 0) break;
    }
}

// After the walks: the table is read before the next round's entries go in.
__device__ __forceinline__ void lzw_carry(LzwCarry& C, const LzwRound& R, int code, uint32_t want) {
    wave_sync();
    if (R.m > 0) {
        const uint32_t total = __shfl(R.incl, R.m - 1);
        C.base = total >= R.rem ? want : C.base + total;
        C.prev_code = __shfl(code, R.m - 1);
        C.prev_F = __shfl(R.F, R.m - 1);
        C.prev_L = __shfl(R.L, R.m - 1);
    }
}

}  // namespace icx
