// wc_budget.h — the three-digit radix select (12 + 12 + 7 bits of a 32-bit key)
// that the size-budget mode (wc_budget.hip: keys of the staged coefficients) and
// the pair selection (wc_thin.hip: keys in a scratch row) both run: the key of a
// candidate, the walk of one wave over a digit's counts, the thresholds of a
// boundary key T, and the skeleton of the select in its three forms:
//   bg_solo      one workgroup, one unit: the three digits in one launch
//   bg_pick<P>   one wave, one split unit: the walk over digit P's global bins,
//                between the launches that fill them
//   bg_passes<P> host: memset, digit P, pick P, and on through digit 3
// A user supplies where a key comes from (its binning callables) and how the first
// digit's count of a value is formed (per-level bin sets, or one plain set).
// Internal: not installed.
#pragma once

#include "wc_leveltol.h"

#include <type_traits>

namespace wc {

constexpr uint32_t kBgInf = 0x7f800000u;
constexpr uint32_t kBgLevelStep = (uint32_t)WC_LTOL_SHIFT << kHistShift;  // a level's offset in the key
constexpr int kBgMidBins = 4096, kBgLowBins = 128;
static_assert(kBgMidBins == kHistBins && kHistShift == 19, "digits of 12 + 12 + 7 bits over a 16 KiB bin set");

// magnitude bits m of a candidate at level index lv (level - 1)
__device__ __forceinline__ bool bg_candidate(uint32_t m) { return m - 1u < kBgInf; }  // 1 <= m <= 0x7F800000
__device__ __forceinline__ uint32_t bg_key(uint32_t m, uint32_t lv) { return m + lv * kBgLevelStep; }
__device__ __forceinline__ int bg_top_bins(int L) { return kHistBins + WC_LTOL_SHIFT * (L - 1); }  // the first digit's values

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

// The select of one unit of L levels with budget K by one workgroup of kLtThreads.
//   first()              zeroes the bins, bins the first digit of every key and ends on a barrier
//   top(s)               the first digit's count of the value s, s < bg_top_bins(L)
//   mid(s), low(prefix)  bin digit 2 of the keys with first digit s, digit 3 of the keys with
//                        key >> 7 == prefix, into h (zeroed here)
//   write(T)             called by one thread: T = 0 where the unit has at most K candidates
// h: LDS bins of at least kBgMidBins words; st: three LDS words outside h[0, kBgMidBins) that
// first() leaves free (found, digit, above: the walks' hand-off between the waves).
template <class First, class Top, class Mid, class Low, class Write>
__device__ __forceinline__ void bg_solo(uint32_t* h, uint32_t* st, int L, uint32_t K, First first, Top top, Mid mid,
                                        Low low, Write write) {
    const int ln = (int)threadIdx.x;
    first();
    if (ln < kWave) {
        uint32_t above = 0u;
        int d = 0;
        const bool found = bg_walk(top, bg_top_bins(L), K, ln, above, d);
        if (ln == 0) {
            st[0] = found ? 1u : 0u;
            st[1] = (uint32_t)d;
            st[2] = above;
        }
    }
    __syncthreads();
    if (!st[0]) {  // uniform: at most K candidates
        if (ln == 0) write(0u);
        return;
    }
    // a later digit: `bits` more bits of the prefix in st[1]; the last one writes T instead
    auto digit = [&](int nbins, int bits, auto bin, bool last) {
        const uint32_t prefix = st[1];
        lt_zero(h, nbins);  // (its barrier: st has been read)
        bin(prefix);
        __syncthreads();
        if (ln < kWave) {
            uint32_t above = st[2];
            int d = 0;
            (void)bg_walk([&](int i) { return h[i]; }, nbins, K, ln, above, d);
            if (ln == 0 && last) {
                write((prefix << bits) | (uint32_t)d);
            } else if (ln == 0) {
                st[1] = (prefix << bits) | (uint32_t)d;
                st[2] = above;
            }
        }
        if (!last) __syncthreads();
    };
    digit(kBgMidBins, 12, mid, false);
    digit(kBgLowBins, 7, low, true);
}

// Step P of a split unit's select by one wave, between the launches that fill digit P's global
// bins: top(s) as in bg_solo (P == 1), h the one bin set of digit 2 or 3; S: the unit's state.
template <int P, class Top, class Write>
__device__ __forceinline__ void bg_pick(BudgetState* __restrict__ S, int L, uint32_t K, Top top,
                                        const uint32_t* __restrict__ h, Write write) {
    const int ln = (int)threadIdx.x;
    BudgetState s = *S;
    int d = 0;
    if (P == 1) {
        uint32_t above = 0u;
        const bool found = bg_walk(top, bg_top_bins(L), K, ln, above, d);
        if (ln == 0) {
            *S = {(uint32_t)d, above, found ? 0u : 1u, 0u};
            if (!found) write(0u);
        }
        return;
    }
    if (s.done) return;  // uniform
    (void)bg_walk([&](int i) { return h[i]; }, P == 2 ? kBgMidBins : kBgLowBins, K, ln, s.above, d);
    if (ln != 0) return;
    if (P == 2) {
        *S = {(s.prefix << 12) | (uint32_t)d, s.above, 0u, 0u};
    } else {
        *S = {s.prefix, s.above, 1u, 0u};
        write((s.prefix << 7) | (uint32_t)d);
    }
}

// Host: the split units' passes from digit P on: the global bins cleared, digit(P) fills them,
// pick(P) walks them.  digit and pick launch their kernel's instantiation for the
// std::integral_constant they are given.
template <int P, class Digit, class Pick>
hipError_t bg_passes(hipStream_t st, uint32_t* gbins, size_t bytes, Digit digit, Pick pick) {
    hipError_t e;
    if ((e = hipMemsetAsync(gbins, 0, bytes, st)) != hipSuccess) return e;
    digit(std::integral_constant<int, P>{});
    if ((e = hipGetLastError()) != hipSuccess) return e;
    pick(std::integral_constant<int, P>{});
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if constexpr (P < 3) return bg_passes<P + 1>(st, gbins, bytes, digit, pick);
    return hipSuccess;
}

}  // namespace wc
