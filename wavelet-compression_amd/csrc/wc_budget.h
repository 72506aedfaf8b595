// wc_budget.h — what the size-budget select (wc_budget.hip) shares with the
// compressed-domain thinning (wc_thin.hip): the key of a candidate, the walk of
// one wave over a digit's counts, and the thresholds of a boundary key T.  The
// code is wc_budget.hip's, moved here unchanged.  Internal: not installed.
#pragma once

#include "wc_leveltol.h"

namespace wc {

constexpr uint32_t kBgInf = 0x7f800000u;
constexpr uint32_t kBgLevelStep = (uint32_t)WC_LTOL_SHIFT << kHistShift;  // a level's offset in the key
constexpr int kBgMidBins = 4096, kBgLowBins = 128;
static_assert(kBgMidBins == kHistBins && kHistShift == 19, "digits of 12 + 12 + 7 bits over a 16 KiB bin set");

// magnitude bits m of a candidate at level index lv (level - 1)
__device__ __forceinline__ bool bg_candidate(uint32_t m) { return m - 1u < kBgInf; }  // 1 <= m <= 0x7F800000
__device__ __forceinline__ uint32_t bg_key(uint32_t m, uint32_t lv) { return m + lv * kBgLevelStep; }

// The walk by one full wave (lane ln) over cnt(d), d = nbins - 1 down to 0, 64
// values per round (lane 0 the largest): true with d* and above += #(d > d*)
// when above + #(d >= d*) > K for some d, else false with above += every count.
// Counts and above stay below 2^31 (N < 2^31).
template <class F>
__device__ __forceinline__ bool bg_walk(F cnt, int nbins, uint32_t K, int ln, uint32_t& above, int& dstar) {
    for (int top = nbins - 1; top >= 0; top -= kWave) {
        const int d = top - ln;
        const uint32_t c = d >= 0 ? cnt(d) : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, kWave);
            if (ln >= o) incl += t;
        }
        const unsigned long long over = __ballot(above + incl > K);
        if (over) {  // uniform
            const int j = __ffsll((long long)over) - 1;
            above += __shfl(incl - c, j, kWave);
            dstar = top - j;
            return true;
        }
        above += __shfl(incl, kWave - 1, kWave);
    }
    return false;
}

// thresh_l of T (include/wavelet_amd.h, wc_budget_thresholds); entries past L are 0.0f
__device__ __forceinline__ void bg_write(uint32_t T, int L, float* __restrict__ thresh, uint32_t* __restrict__ key) {
#pragma unroll
    for (int l = 0; l < WC_MAX_LEVELS; ++l) {
        const long long d = (long long)T - (long long)((uint32_t)l * kBgLevelStep);
        thresh[l] = l >= L || d <= 0 ? 0.0f : d >= (long long)kBgInf ? __uint_as_float(kBgInf) : __uint_as_float((uint32_t)d);
    }
    if (key) *key = T;
}

}  // namespace wc
