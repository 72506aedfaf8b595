// wc_tol.hip — per-unit thresholds of the opt-in RMSE-tolerance mode
// (wc_forward_tol / wc_forward_emit_tol in include/wavelet_amd.h).
//
// Not part of the reference's codec: src/compressor.cpp:212-216 thresholds
// every box at (its own max) * (1 - keep), so the error of a box follows from
// its largest coefficient.  This mode takes the tolerated RMSE of each unit
// and picks the unit's threshold from the unit's own magnitude histogram (the
// bins of wc_hist.hip): with even W, H and D the one-level transform is
// orthogonal with squared basis norm 8, so dropping the coefficient set S
// costs SSE = 8 * sum_S c^2.  Bins are dropped from the smallest magnitudes up
// while the energy bound of the dropped bins (count * 8 * upper edge^2, summed
// in double in bin order) stays within tol^2 * N.  The choice depends on
// integer counts only: it does not depend on the order of any atomic, and the
// host restatement (wc_tol_threshold) gives the same bits.  Payload format,
// run-length rule and decoder are unchanged; only the threshold differs.
//
// HBM-bound: one 16-B load per 4 staged coefficients (4 B/coefficient read).
//   k_tol_solo   one workgroup per unit of up to WC_OPT_TOL_SOLO_TILES flat
//                tiles: LDS bins (two sets, summed at the end), pick,
//                thresh[u] / bound[u].  No global bins, no global atomics.
//   k_tol_split  larger units, a run of tiles per workgroup: LDS bins, then the
//                nonzero ones added to the unit's global bins (integer atomics).
//   k_tol_pick   one wave per split unit (a later launch: nothing waits on
//                another workgroup): the pick over the unit's global bins.
#include "wc_device.h"

namespace wc {

constexpr int kTolThreads = 256;
constexpr uint32_t kTolSolo = 0xffffffffu;  // slot[] of a unit that k_tol_solo owns
// LDS bin sets per workgroup (thread & 1 picks one): lanes of a wave that hit
// the same bin serialize, two sets halve that; 17 words apart in banks.  With
// the next tile's loads issued before a tile is counted: the bin pass of C2
// 0.308 -> 0.267 ms; four sets (64 KB, 2 workgroups per CU) 0.40 ms
// (profiles/r07/experiments/tol_variants.txt).
constexpr int kTolCopies = 2;
constexpr int kTolStride = kHistBins + 17;

__device__ __forceinline__ void tol_zero(uint32_t* h) {
    for (int i = threadIdx.x; i < kTolCopies * kTolStride; i += kTolThreads) h[i] = 0u;
    __syncthreads();
}
// after the last add: the copies summed into the first
__device__ __forceinline__ void tol_fold(uint32_t* h) {
    __syncthreads();
    for (int i = threadIdx.x; i < kHistBins; i += kTolThreads) {
        uint32_t s = h[i];
#pragma unroll
        for (int c = 1; c < kTolCopies; ++c) s += h[c * kTolStride + i];
        h[i] = s;
    }
    __syncthreads();
}

// Flat tile `tile` of unit U (kFlatTile coefficients): the loads of k_hist,
// every load of the tile in flight at once.  Returns the tile's length.
constexpr int kTolIt = kFlatTile / (4 * kTolThreads);
__device__ __forceinline__ uint32_t tol_load(float4 (&v)[kTolIt], const float* __restrict__ coef, const UnitDev& U,
                                             uint32_t tile) {
    const uint64_t start = (uint64_t)tile * kFlatTile;
    const uint32_t len = (uint32_t)min((uint64_t)kFlatTile, U.ncells - start);
    // coef_off is 16-B aligned and kFlatTile a multiple of 4: float4 loads (the
    // scratch keeps kFlatTile floats of slack past the last unit)
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(coef + U.coef_off + start);
#pragma unroll
    for (int it = 0; it < kTolIt; ++it) {
        const uint32_t q = it * kTolThreads + threadIdx.x;
        v[it] = 4 * q < len ? p4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return len;
}

__device__ __forceinline__ void tol_add(uint32_t* h, const float4 (&v)[kTolIt], uint32_t len) {
#pragma unroll
    for (int it = 0; it < kTolIt; ++it) {
        const uint32_t e = 4 * (it * kTolThreads + threadIdx.x);
        hist_add(h, v[it].x, e < len);
        hist_add(h, v[it].y, e + 1 < len);
        hist_add(h, v[it].z, e + 2 < len);
        hist_add(h, v[it].w, e + 3 < len);
    }
}

// Tiles [t0, t1) of unit U into the LDS bins h; the loads of tile t + 1 are
// issued before tile t is counted (the LDS adds run under the next loads).
__device__ __forceinline__ void tol_bin_tiles(uint32_t* h, const float* __restrict__ coef, const UnitDev& U,
                                              uint32_t t0, uint32_t t1) {
    if (t0 >= t1) return;
    float4 cur[kTolIt], nxt[kTolIt];
    uint32_t len = tol_load(cur, coef, U, t0), nlen = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;  // uniform
        if (more) nlen = tol_load(nxt, coef, U, t + 1);
        tol_add(h, cur, len);
        if (more) {
#pragma unroll
            for (int it = 0; it < kTolIt; ++it) cur[it] = nxt[it];
            len = nlen;
        }
    }
}

// The selection rule (include/wavelet_amd.h, wc_tol_threshold) on the kHistBins
// counts at h, by one full wave (lane l): 64 bins per round, each lane its
// bin's energy bound; the nonempty bins are then taken in bin order (the sum S
// is rounded after every add, so the order is part of the rule).  Separate
// double multiplies and adds (-ffp-contract=off).
__device__ __forceinline__ void tol_pick(const uint32_t* h, uint64_t N, double tol, int l, float* thresh,
                                         double* bound) {
    const double budget = (tol * tol) * (double)N;
    double S = 0.0;
    int bstar = kHistBins;
    for (int base = 0; base < kHistBins && bstar == kHistBins; base += kWave) {
        const int b = base + l;
        const uint32_t cnt = h[b];
        // every |c| of bin b is below hi: the float with bits (b + 1) << 19, +inf from the last finite bin on
        const double hi = b < 0xFEF ? (double)__uint_as_float((uint32_t)(b + 1) << kHistShift)
                                    : (double)__builtin_inff();
        const double term = (double)cnt * (8.0 * (hi * hi));
        unsigned long long m = __ballot(cnt != 0u);
        while (m) {  // uniform
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double t = S + __shfl(term, j, kWave);
            if (!(t <= budget)) {
                bstar = base + j;
                break;
            }
            S = t;
        }
    }
    if (l == 0) {
        // the emit keeps |c| > thresh: exactly the bins >= bstar
        float t;
        if (bstar == 0) t = 0.0f;
        else if (bstar >= 0xFF0) t = __uint_as_float(0x7f7fffffu);  // FLT_MAX: only +-inf is kept
        else t = __uint_as_float(((uint32_t)bstar << kHistShift) - 1u);
        *thresh = t;
        if (bound) *bound = N ? sqrt(S / (double)N) : 0.0;
    }
}

// Workgroup u owns unit u unless the unit is split (slot[u] != kTolSolo).
__global__ __launch_bounds__(kTolThreads) void k_tol_solo(const UnitDev* __restrict__ units,
                                                        const uint32_t* __restrict__ slot,
                                                        const float* __restrict__ coef,
                                                        const double* __restrict__ tol, float* __restrict__ thresh,
                                                        double* __restrict__ bound) {
    const uint32_t u = blockIdx.x;
    if (slot[u] != kTolSolo) return;  // uniform
    __shared__ uint32_t h[kTolCopies * kTolStride];
    tol_zero(h);
    uint32_t* hc = h + (threadIdx.x & (kTolCopies - 1)) * kTolStride;
    const UnitDev& U = units[u];
    tol_bin_tiles(hc, coef, U, 0u, U.nftiles);
    tol_fold(h);
    if (threadIdx.x < kWave) tol_pick(h, U.ncells, tol[u], (int)threadIdx.x, thresh + u, bound ? bound + u : nullptr);
}

// Work item i: tiles [items[i].y, + chunk) of split unit items[i].x, added to
// the unit's global bins gbins + slot * kHistBins (zeroed by the caller).
__global__ __launch_bounds__(kTolThreads) void k_tol_split(const UnitDev* __restrict__ units,
                                                         const uint32_t* __restrict__ slot,
                                                         const uint2* __restrict__ items, uint32_t chunk,
                                                         const float* __restrict__ coef,
                                                         uint32_t* __restrict__ gbins) {
    __shared__ uint32_t h[kTolCopies * kTolStride];
    tol_zero(h);
    uint32_t* hc = h + (threadIdx.x & (kTolCopies - 1)) * kTolStride;
    const uint2 it = items[blockIdx.x];
    const UnitDev& U = units[it.x];
    tol_bin_tiles(hc, coef, U, it.y, min(it.y + chunk, U.nftiles));
    tol_fold(h);
    uint32_t* __restrict__ g = gbins + (size_t)slot[it.x] * kHistBins;
    for (int i = threadIdx.x; i < kHistBins; i += kTolThreads)
        if (h[i]) atomicAdd(g + i, h[i]);
}

// Workgroup s (one wave): the pick of split unit split_units[s] over its global bins.
__global__ __launch_bounds__(kWave) void k_tol_pick(const UnitDev* __restrict__ units,
                                                  const uint32_t* __restrict__ split_units,
                                                  const uint32_t* __restrict__ gbins,
                                                  const double* __restrict__ tol, float* __restrict__ thresh,
                                                  double* __restrict__ bound) {
    const uint32_t u = split_units[blockIdx.x];
    tol_pick(gbins + (size_t)blockIdx.x * kHistBins, units[u].ncells, tol[u], (int)threadIdx.x, thresh + u,
             bound ? bound + u : nullptr);
}

// slot[n]: kTolSolo, or the unit's index among the split units (= its row of
// gbins and its position in split_units[nsplit]); items[nitems]: the split
// units' tile runs of `chunk` tiles.
hipError_t launch_tol(hipStream_t st, const UnitDev* units, int n, const uint32_t* slot, const uint2* items,
                      uint32_t nitems, uint32_t chunk, const uint32_t* split_units, uint32_t nsplit,
                      const float* coef, uint32_t* gbins, const double* tol, float* thresh, double* bound) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if ((uint32_t)n > nsplit) {
        k_tol_solo<<<(uint32_t)n, kTolThreads, 0, st>>>(units, slot, coef, tol, thresh, bound);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (nsplit) {
        k_tol_split<<<nitems, kTolThreads, 0, st>>>(units, slot, items, chunk, coef, gbins);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_tol_pick<<<nsplit, kWave, 0, st>>>(units, split_units, gbins, tol, thresh, bound);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace wc
