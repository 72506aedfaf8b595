// wc_leveltol.hip — per-level thresholds of the RMSE tolerance on the opt-in
// multi-level transform (wc_forward_levels_tol in include/wavelet_amd.h).
//
// Not part of the reference's codec.  The siblings of wc_tol.hip for units with
// L >= 1 levels: the basis vectors of level l have squared norm 8^l, so each
// level gets its own magnitude bins and its own threshold.  A coefficient's
// level follows from its flat position p = (I*H + J)*D + K alone: the largest j
// < L with (I, J, K) inside (W, H, D) >> j, plus one.  D % 4 == 0 whenever
// L >= 2, so the four coefficients of a 16-B load share I and J: one row
// decomposition (two magic divisions, wc_device.h div_rows) per load, then K
// against D >> j per element (a D >> j boundary may fall inside a load).  An
// L = 1 unit skips the decomposition.  With even dimensions W*H*D % 8 == 0:
// every 16-B load of a unit lies inside it.
//
// HBM-bound: the bins read 4 B/coefficient, the mask pass reads 4 B and writes
// back only the 16-B groups it changed.
//   k_ltol_solo<NL>   one workgroup per unit of up to WC_OPT_TOL_SOLO_TILES flat
//                   tiles: LDS bins, pick, thresh[u][1..L] / bound[u]
//   k_ltol_split<NL>  larger units, a run of tiles per workgroup: LDS bins, then
//                   the nonzero ones added to the unit's NL x 16 KB global bins
//   k_ltol_pick     one wave per split unit (a later launch): the pick over the
//                   unit's global bins
//   k_ltol_mask     one workgroup per flat tile: every coefficient with
//                   !(|c| > thresh[lvl]) becomes +0.0f in the staged array, so
//                   the unchanged emit keeps the rest with threshold 0.0f
// NL = the largest L of the call.  LDS per workgroup: level 1 has two bin sets
// (thread & 1 picks one, as wc_tol.hip; the second is stored rotated by 17 bins
// instead of padded, which puts the same bin of the two sets 17 banks apart at
// no cost in bytes); levels >= 2 hold at most 1/8 of a unit's coefficients and
// have one set each: (NL + 1) x 16 KiB = 32 / 48 / 64 / 80 KiB for NL = 1..4,
// which leaves 5 / 3 / 2 / 2 workgroups per CU of the 160 KiB.
// (LtGeom, lt_levels4, the LDS bins and the flat-tile loads: wc_leveltol.h, shared with wc_budget.hip;
// lt_pick, the rule's walk: there too, shared with wc_thin.hip's tolerance form)
#include "wc_leveltol.h"

namespace wc {

// Workgroup u owns unit u unless the unit is split (lt[u].slot != kLtSolo).
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_ltol_solo(const UnitDev* __restrict__ units,
                                                        const LtUnit* __restrict__ lt,
                                                        const float* __restrict__ coef, float* __restrict__ thresh,
                                                        double* __restrict__ bound) {
    const uint32_t u = blockIdx.x;
    const LtUnit T = lt[u];
    if (T.slot != kLtSolo) return;  // uniform
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    lt_zero(h, (NL + 1) * kHistBins);
    const UnitDev& U = units[u];
    lt_bin_tiles(h, coef, U, lt_geom(U, T), 0u, U.nftiles);
    lt_fold(h);
    if (threadIdx.x < kWave)
        lt_pick(h, 2 * kHistBins, (int)T.levels, U.ncells, T.tol, (int)threadIdx.x, thresh + (size_t)u * WC_MAX_LEVELS,
                bound ? bound + u : nullptr);
}

// Work item i: tiles [items[i].y, + chunk) of split unit items[i].x, added to
// the unit's global bins gbins + slot * NL * kHistBins (level-major, zeroed by
// the caller).
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_ltol_split(const UnitDev* __restrict__ units,
                                                         const LtUnit* __restrict__ lt,
                                                         const uint2* __restrict__ items, uint32_t chunk,
                                                         const float* __restrict__ coef,
                                                         uint32_t* __restrict__ gbins) {
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    lt_zero(h, (NL + 1) * kHistBins);
    const uint2 it = items[blockIdx.x];
    const UnitDev& U = units[it.x];
    const LtUnit T = lt[it.x];
    lt_bin_tiles(h, coef, U, lt_geom(U, T), it.y, min(it.y + chunk, U.nftiles));
    lt_fold(h);
    uint32_t* __restrict__ g = gbins + (size_t)T.slot * NL * kHistBins;
    for (int l = 1; l <= (int)T.levels; ++l) {
        const uint32_t* hl = h + lt_base(l);
        for (int i = threadIdx.x; i < kHistBins; i += kLtThreads)
            if (hl[i]) atomicAdd(g + (l - 1) * kHistBins + i, hl[i]);
    }
}

// Workgroup s (one wave): the pick of split unit split_units[s] over its global bins.
__global__ __launch_bounds__(kWave) void k_ltol_pick(const UnitDev* __restrict__ units,
                                                   const LtUnit* __restrict__ lt,
                                                   const uint32_t* __restrict__ split_units,
                                                   const uint32_t* __restrict__ gbins, int nl,
                                                   float* __restrict__ thresh, double* __restrict__ bound) {
    const uint32_t u = split_units[blockIdx.x];
    const LtUnit T = lt[u];
    lt_pick(gbins + (size_t)blockIdx.x * nl * kHistBins, kHistBins, (int)T.levels, units[u].ncells, T.tol,
            (int)threadIdx.x, thresh + (size_t)u * WC_MAX_LEVELS, bound ? bound + u : nullptr);
}

// Workgroup t: flat tile tiles[t] of its unit, masked in place.
__global__ __launch_bounds__(kLtThreads) void k_ltol_mask(const UnitDev* __restrict__ units,
                                                        const LtUnit* __restrict__ lt,
                                                        const FTile* __restrict__ tiles, float* __restrict__ coef,
                                                        const float* __restrict__ thresh) {
    const FTile ft = tiles[blockIdx.x];
    const UnitDev& U = units[ft.unit];
    const LtGeom G = lt_geom(U, lt[ft.unit]);
    const float* th = thresh + (size_t)ft.unit * WC_MAX_LEVELS;
    const float t0 = th[0], t1 = th[1], t2 = th[2], t3 = th[3];
    const uint64_t start = (uint64_t)ft.index * kFlatTile;
    const uint32_t len = (uint32_t)min((uint64_t)kFlatTile, U.ncells - start);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(coef + U.coef_off + start);
    float4 v[kLtIt];
#pragma unroll
    for (int it = 0; it < kLtIt; ++it) {
        const uint32_t q = it * kLtThreads + threadIdx.x;
        v[it] = 4 * q < len ? p4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < kLtIt; ++it) {
        const uint32_t q = it * kLtThreads + threadIdx.x;
        if (4 * q >= len) continue;
        const uint32_t lv = lt_levels4(G, (uint32_t)start + 4 * q);
        float c[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        bool changed = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t l = (lv >> (2 * e)) & 3u;
            const float t = l == 0u ? t0 : l == 1u ? t1 : l == 2u ? t2 : t3;
            if (!(fabsf(c[e]) > t)) {  // NaN goes too
                changed |= __float_as_uint(c[e]) != 0u;
                c[e] = 0.0f;
            }
        }
        if (changed) p4[q] = make_float4(c[0], c[1], c[2], c[3]);
    }
}

// lt[n]: the units' descriptors; items[nitems]: the split units' tile runs of
// `chunk` tiles; split_units[nsplit]; gbins: nsplit x maxl x kHistBins, zeroed;
// thresh: n x WC_MAX_LEVELS floats.
hipError_t launch_leveltol(hipStream_t st, const UnitDev* units, int n, const LtUnit* lt, const uint2* items,
                           uint32_t nitems, uint32_t chunk, const uint32_t* split_units, uint32_t nsplit, int maxl,
                           const float* coef, uint32_t* gbins, float* thresh, double* bound) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if ((uint32_t)n > nsplit) {
        switch (maxl) {
            case 1: k_ltol_solo<1><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, coef, thresh, bound); break;
            case 2: k_ltol_solo<2><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, coef, thresh, bound); break;
            case 3: k_ltol_solo<3><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, coef, thresh, bound); break;
            default: k_ltol_solo<4><<<(uint32_t)n, kLtThreads, 0, st>>>(units, lt, coef, thresh, bound); break;
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (nsplit) {
        switch (maxl) {
            case 1: k_ltol_split<1><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
            case 2: k_ltol_split<2><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
            case 3: k_ltol_split<3><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
            default: k_ltol_split<4><<<nitems, kLtThreads, 0, st>>>(units, lt, items, chunk, coef, gbins); break;
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ltol_pick<<<nsplit, kWave, 0, st>>>(units, lt, split_units, gbins, maxl, thresh, bound);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_leveltol_mask(hipStream_t st, const UnitDev* units, const LtUnit* lt, const FTile* tiles,
                                uint32_t ntiles, float* coef, const float* thresh) {
    if (!ntiles) return hipSuccess;
    k_ltol_mask<<<ntiles, kLtThreads, 0, st>>>(units, lt, tiles, coef, thresh);
    return hipGetLastError();
}

}  // namespace wc
