// wc_budget.hip — the size-budget mode of the opt-in multi-level transform
// (wc_forward_levels_budget in include/wavelet_amd.h): per unit, the threshold T
// that keeps the max_pairs largest weighted coefficients and never more, by a
// three-digit radix select on the 32-bit key
//   key(c) = bits of |c| + ((WC_LTOL_SHIFT * (lvl - 1)) << WC_HIST_SHIFT)
// over the candidates (1 <= bits of |c| <= 0x7F800000: +-0 and NaN are none).
//
// Not part of the reference's codec.  Three passes over the staged final array,
// each HBM-bound at 4 B per coefficient, with the level of a position, the LDS
// bins and the tile pipeline of wc_leveltol.h:
//   digit 1  key >> 19        per-level bins of the magnitude (as k_ltol_solo,
//                             zeros not counted); the walk goes down over
//                             total[s] = sum_l cnt[l][s - 24 (l - 1)]
//   digit 2  (key >> 7) & 0xFFF  only keys whose first digit is the boundary s*
//   digit 3  key & 0x7F          only keys with key >> 7 == (s*, second digit)
// A walk over a digit's counts, downward from the largest value, finds d* with
//   above + #(d > d*) <= K < above + #(d >= d*)
// and adds #(d > d*) to `above`; after the third digit T = the (K + 1)-th
// largest key and above = #(key > T) <= K.  A unit with at most K candidates is
// done after the first digit with T = 0.  Only integer counts enter.
//   k_budget_solo<NL>   one workgroup per unit of up to WC_OPT_TOL_SOLO_TILES
//                       flat tiles: the three digits in one launch (the second
//                       and third read find the unit in the caches), then
//                       thresh[u][1..L] / key[u]
//   k_budget_split<NL>  larger units, a run of tiles per workgroup: digit 1's LDS
//                       bins, the nonzero ones added to the unit's NL x 16 KiB
//                       global bins
//   k_budget_digit<P>   the same tile runs for digit P = 2, 3: one 16 KiB bin
//                       set (few keys pass the filter, so few atomics); leaves
//                       at once when the unit's state says done
//   k_budget_pick<P>    one wave per split unit (a later launch): the walk over
//                       the unit's global bins, its state {prefix, above, done}
//                       and, at the end, thresh / key
// The select's skeleton (bg_solo, bg_pick, bg_passes) is wc_budget.h's, shared with
// wc_thin.hip: here a key is a staged coefficient's and the first digit's count
// sums per-level bin sets.
// The mask pass and the emit are wc_leveltol.hip's and wc_emit.hip's, unchanged.
// LDS per workgroup as k_ltol_solo: (NL + 1) x 16 KiB.
#include "wc_budget.h"

namespace wc {

// Tiles [t0, t1) of unit U, f(m, lv) on every coefficient; the loads of tile
// t + 1 are issued before tile t is visited (lt_bin_tiles).
template <class F>
__device__ __forceinline__ void bg_tiles(const float* __restrict__ coef, const UnitDev& U, const LtGeom& G,
                                         uint32_t t0, uint32_t t1, F f) {
    if (t0 >= t1) return;
    float4 cur[kLtIt], nxt[kLtIt];
    uint32_t len = lt_load(cur, coef, U, t0), nlen = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;  // uniform
        if (more) nlen = lt_load(nxt, coef, U, t + 1);
#pragma unroll
        for (int it = 0; it < kLtIt; ++it) {
            const uint32_t e = 4 * (it * kLtThreads + threadIdx.x);
            if (e >= len) continue;  // len % 4 == 0: the load is inside the unit or outside it
            const uint32_t lv = lt_levels4(G, t * (uint32_t)kFlatTile + e);
            f(__float_as_uint(cur[it].x) & 0x7fffffffu, lv & 3u);
            f(__float_as_uint(cur[it].y) & 0x7fffffffu, (lv >> 2) & 3u);
            f(__float_as_uint(cur[it].z) & 0x7fffffffu, (lv >> 4) & 3u);
            f(__float_as_uint(cur[it].w) & 0x7fffffffu, lv >> 6);
        }
        if (more) {
#pragma unroll
            for (int it = 0; it < kLtIt; ++it) cur[it] = nxt[it];
            len = nlen;
        }
    }
}

// digit 1 into the per-level LDS bins (lt_add1 without the zeros)
__device__ __forceinline__ void bg_bin_top(uint32_t* h, const float* __restrict__ coef, const UnitDev& U,
                                           const LtGeom& G, uint32_t t0, uint32_t t1) {
    const uint32_t set = threadIdx.x & 1u;
    bg_tiles(coef, U, G, t0, t1, [&](uint32_t m, uint32_t lv) {
        if (!bg_candidate(m)) return;
        const uint32_t b = m >> kHistShift;
        const uint32_t i = lv ? (lv + 1u) * kHistBins + b : set ? kHistBins + ((b + kLtRot) & (kHistBins - 1)) : b;
        atomicAdd(h + i, 1u);
    });
}
// digit 2 of the keys with first digit s
__device__ __forceinline__ void bg_bin_mid(uint32_t* h, const float* __restrict__ coef, const UnitDev& U,
                                           const LtGeom& G, uint32_t t0, uint32_t t1, uint32_t s) {
    bg_tiles(coef, U, G, t0, t1, [&](uint32_t m, uint32_t lv) {
        const uint32_t k = bg_key(m, lv);
        if (bg_candidate(m) && (k >> kHistShift) == s) atomicAdd(h + ((k >> 7) & (kBgMidBins - 1)), 1u);
    });
}
// digit 3 of the keys with key >> 7 == prefix
__device__ __forceinline__ void bg_bin_low(uint32_t* h, const float* __restrict__ coef, const UnitDev& U,
                                           const LtGeom& G, uint32_t t0, uint32_t t1, uint32_t prefix) {
    bg_tiles(coef, U, G, t0, t1, [&](uint32_t m, uint32_t lv) {
        const uint32_t k = bg_key(m, lv);
        if (bg_candidate(m) && (k >> 7) == prefix) atomicAdd(h + (k & (kBgLowBins - 1)), 1u);
    });
}

// digit 1's count of s over the levels: level 1's bins at h, level l >= 2's at
// h + off2 + (l - 2) * kHistBins (lt_pick's layout)
__device__ __forceinline__ uint32_t bg_top_count(const uint32_t* h, int off2, int L, int s) {
    uint32_t c = 0u;
#pragma unroll
    for (int l = 0; l < WC_MAX_LEVELS; ++l) {
        const int b = s - WC_LTOL_SHIFT * l;
        if (l < L && b >= 0 && b < kHistBins) c += h[(l ? off2 + (l - 1) * kHistBins : 0) + b];
    }
    return c;
}

// Workgroup u owns unit u unless the unit is split (lt[u].slot != kLtSolo).
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_budget_solo(const UnitDev* __restrict__ units,
                                                          const LtUnit* __restrict__ lt,
                                                          const uint32_t* __restrict__ max_pairs,
                                                          const float* __restrict__ coef, float* __restrict__ thresh,
                                                          uint32_t* __restrict__ key) {
    const uint32_t u = blockIdx.x;
    const LtUnit T = lt[u];
    if (T.slot != kLtSolo) return;  // uniform
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    // bg_solo's state words: in level 1's second bin set, free once lt_fold has summed it into the first
    // (a word more of LDS than k_ltol_solo's would cost a workgroup per CU at NL = 1 and NL = 4)
    uint32_t* st = h + kHistBins;
    const UnitDev& U = units[u];
    const LtGeom G = lt_geom(U, T);
    const uint32_t nt = U.nftiles;
    const int L = (int)T.levels;
    bg_solo(
        h, st, L, max_pairs[u],
        [&] {
            lt_zero(h, (NL + 1) * kHistBins);
            bg_bin_top(h, coef, U, G, 0u, nt);
            lt_fold(h);
        },
        [&](int s) { return bg_top_count(h, 2 * kHistBins, L, s); },
        [&](uint32_t s) { bg_bin_mid(h, coef, U, G, 0u, nt, s); },
        [&](uint32_t prefix) { bg_bin_low(h, coef, U, G, 0u, nt, prefix); },
        [&](uint32_t Tk) { bg_write(Tk, L, thresh + (size_t)u * WC_MAX_LEVELS, key ? key + u : nullptr); });
}

// Work item i: tiles [items[i].y, + chunk) of split unit items[i].x, digit 1's
// bins added to the unit's global bins gbins + slot * NL * kHistBins
// (level-major, zeroed by the caller).
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_budget_split(const UnitDev* __restrict__ units,
                                                           const LtUnit* __restrict__ lt,
                                                           const uint2* __restrict__ items, uint32_t chunk,
                                                           const float* __restrict__ coef,
                                                           uint32_t* __restrict__ gbins) {
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    lt_zero(h, (NL + 1) * kHistBins);
    const uint2 it = items[blockIdx.x];
    const UnitDev& U = units[it.x];
    const LtUnit T = lt[it.x];
    bg_bin_top(h, coef, U, lt_geom(U, T), it.y, min(it.y + chunk, U.nftiles));
    lt_fold(h);
    uint32_t* __restrict__ g = gbins + (size_t)T.slot * NL * kHistBins;
    for (int l = 1; l <= (int)T.levels; ++l) {
        const uint32_t* hl = h + lt_base(l);
        for (int i = threadIdx.x; i < kHistBins; i += kLtThreads)
            if (hl[i]) atomicAdd(g + (l - 1) * kHistBins + i, hl[i]);
    }
}

// The same work items for digit P (2 or 3) of the keys that share the unit's
// prefix, added to the unit's one bin set gbins + slot * kHistBins (zeroed by
// the caller).
template <int P>
__global__ __launch_bounds__(kLtThreads) void k_budget_digit(const UnitDev* __restrict__ units,
                                                           const LtUnit* __restrict__ lt,
                                                           const uint2* __restrict__ items, uint32_t chunk,
                                                           const float* __restrict__ coef,
                                                           const BudgetState* __restrict__ state,
                                                           uint32_t* __restrict__ gbins) {
    constexpr int kBins = P == 2 ? kBgMidBins : kBgLowBins;
    const uint2 it = items[blockIdx.x];
    const LtUnit T = lt[it.x];
    const BudgetState S = state[T.slot];
    if (S.done) return;  // uniform
    __shared__ uint32_t h[kBins];
    lt_zero(h, kBins);
    const UnitDev& U = units[it.x];
    const uint32_t t1 = min(it.y + chunk, U.nftiles);
    if (P == 2)
        bg_bin_mid(h, coef, U, lt_geom(U, T), it.y, t1, S.prefix);
    else
        bg_bin_low(h, coef, U, lt_geom(U, T), it.y, t1, S.prefix);
    __syncthreads();
    uint32_t* __restrict__ g = gbins + (size_t)T.slot * kHistBins;
    for (int i = threadIdx.x; i < kBins; i += kLtThreads)
        if (h[i]) atomicAdd(g + i, h[i]);
}

// Workgroup s (one wave): the walk of split unit split_units[s] over digit P's
// global bins (P = 1: nl level sets per unit; P = 2, 3: one set per unit).
template <int P>
__global__ __launch_bounds__(kWave) void k_budget_pick(const LtUnit* __restrict__ lt,
                                                     const uint32_t* __restrict__ split_units,
                                                     const uint32_t* __restrict__ max_pairs,
                                                     const uint32_t* __restrict__ gbins, int nl,
                                                     BudgetState* __restrict__ state, float* __restrict__ thresh,
                                                     uint32_t* __restrict__ key) {
    const uint32_t u = split_units[blockIdx.x];
    const int L = (int)lt[u].levels;
    const uint32_t* h = gbins + (size_t)blockIdx.x * (P == 1 ? nl : 1) * kHistBins;
    bg_pick<P>(
        state + blockIdx.x, L, max_pairs[u], [&](int s) { return bg_top_count(h, kHistBins, L, s); }, h,
        [&](uint32_t T) { bg_write(T, L, thresh + (size_t)u * WC_MAX_LEVELS, key ? key + u : nullptr); });
}

// lt[n]: the units' descriptors (tol unused); max_pairs[n]; items[nitems]: the
// split units' tile runs of `chunk` tiles; split_units[nsplit]; gbins: nsplit x
// maxl x kHistBins; state[nsplit]; thresh: n x WC_MAX_LEVELS floats; key: n
// uint32 or null.  Every grid follows from the plan: nothing is read back.
hipError_t launch_budget(hipStream_t st, const UnitDev* units, int n, const LtUnit* lt, const uint32_t* max_pairs,
                         const uint2* items, uint32_t nitems, uint32_t chunk, const uint32_t* split_units,
                         uint32_t nsplit, int maxl, const float* coef, uint32_t* gbins, BudgetState* state,
                         float* thresh, uint32_t* key) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if ((uint32_t)n > nsplit) {
        switch (maxl) {
            case 1: k_budget_solo<1><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, max_pairs, coef, thresh, key); break;
            case 2: k_budget_solo<2><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, max_pairs, coef, thresh, key); break;
            case 3: k_budget_solo<3><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, max_pairs, coef, thresh, key); break;
            default: k_budget_solo<4><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, max_pairs, coef, thresh, key); break;
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!nsplit) return e;
    const size_t set_bytes = sizeof(uint32_t) * kHistBins * (size_t)nsplit;
    if ((e = hipMemsetAsync(gbins, 0, set_bytes * maxl, st)) != hipSuccess) return e;
    switch (maxl) {
        case 1: k_budget_split<1><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
        case 2: k_budget_split<2><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
        case 3: k_budget_split<3><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
        default: k_budget_split<4><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    k_budget_pick<1><<<nsplit, kWave, 0, st>>>(lt, split_units, max_pairs, gbins, maxl, state, thresh, key);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return bg_passes<2>(
        st, gbins, set_bytes,
        [&](auto P) {
            k_budget_digit<decltype(P)::value><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, state, gbins);
        },
        [&](auto P) {
            k_budget_pick<decltype(P)::value><<<nsplit, kWave, 0, st>>>(lt, split_units, max_pairs, gbins, maxl, state,
                                                                       thresh, key);
        });
}

}  // namespace wc
