// wc_leveltol.h — device helpers shared by the kernels that read a staged
// multi-level array per unit and per level: wc_leveltol.hip (the RMSE tolerance)
// and wc_budget.hip (the size budget).  The level of a flat position, the
// per-level LDS bins, the flat-tile loads and the tolerance rule's walk over a
// unit's bins (lt_pick, which wc_thin.hip's tolerance form runs too).  Internal:
// not installed.
#pragma once

#include "wc_device.h"

#include "wavelet_amd.h"

namespace wc {

constexpr int kLtThreads = 256;
constexpr int kLtRot = 17;  // rotation of level 1's second bin set
constexpr int kLtIt = kFlatTile / (4 * kLtThreads);
static_assert(WC_MAX_LEVELS == 4, "two bits per level index, four bin-set instantiations");
static_assert(WC_HIST_BINS == kHistBins && WC_HIST_SHIFT == kHistShift, "the bins of wc_hist.hip");

// What the level of a position needs of its unit.
struct LtGeom {
    uint64_t dmagic, hmagic;
    uint32_t W, H, D;
    int L;
};

__device__ __forceinline__ LtGeom lt_geom(const UnitDev& U, const LtUnit& T) {
    return {T.dmagic, T.hmagic, (uint32_t)U.nx, (uint32_t)U.ny, (uint32_t)U.nz, (int)T.levels};
}

// Level index (level - 1, two bits each) of the coefficients p .. p + 3 of one
// 16-B load, p % 4 == 0.
__device__ __forceinline__ uint32_t lt_levels4(const LtGeom& G, uint32_t p) {
    if (G.L == 1) return 0u;  // uniform
    const uint32_t row = div_rows(p, G.dmagic), K0 = p - row * G.D;
    const uint32_t I = div_rows(row, G.hmagic), J = row - I * G.H;
    // the boxes (W, H, D) >> j are nested: the count of the j that hold is j*
    int lij = 0;
#pragma unroll
    for (int j = 1; j < WC_MAX_LEVELS; ++j) lij += (j < G.L && I < (G.W >> j) && J < (G.H >> j)) ? 1 : 0;
    if (lij == 0) return 0u;
    uint32_t r = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t lv = 0u;
#pragma unroll
        for (int j = 1; j < WC_MAX_LEVELS; ++j) lv += (j <= lij && K0 + e < (G.D >> j)) ? 1u : 0u;
        r |= lv << (2 * e);
    }
    return r;
}

// LDS bins: [level 1, set 0 | level 1, set 1 rotated | level 2 | ... | level NL]
__device__ __forceinline__ void lt_zero(uint32_t* h, int words) {
    for (int i = threadIdx.x; i < words; i += kLtThreads) h[i] = 0u;
    __syncthreads();
}
// after the last add: level 1's second set summed into the first.  Level l's
// bins are then at h + lt_base(l).
__device__ __forceinline__ void lt_fold(uint32_t* h) {
    __syncthreads();
    for (int i = threadIdx.x; i < kHistBins; i += kLtThreads) h[i] += h[kHistBins + ((i + kLtRot) & (kHistBins - 1))];
    __syncthreads();
}
__device__ __forceinline__ int lt_base(int l) { return l == 1 ? 0 : l * kHistBins; }

__device__ __forceinline__ void lt_add1(uint32_t* h, uint32_t set, float v, uint32_t lv) {
    const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
    if (m > 0x7f800000u) return;  // NaN is not counted
    const uint32_t b = m >> kHistShift;
    const uint32_t i = lv ? (lv + 1u) * kHistBins + b : set ? kHistBins + ((b + kLtRot) & (kHistBins - 1)) : b;
    atomicAdd(h + i, 1u);
}

// Flat tile `tile` of unit U: every load of the tile in flight at once (wc_tol.hip tol_load).
__device__ __forceinline__ uint32_t lt_load(float4 (&v)[kLtIt], const float* __restrict__ coef, const UnitDev& U,
                                            uint32_t tile) {
    const uint64_t start = (uint64_t)tile * kFlatTile;
    const uint32_t len = (uint32_t)min((uint64_t)kFlatTile, U.ncells - start);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(coef + U.coef_off + start);
#pragma unroll
    for (int it = 0; it < kLtIt; ++it) {
        const uint32_t q = it * kLtThreads + threadIdx.x;
        v[it] = 4 * q < len ? p4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return len;
}

__device__ __forceinline__ void lt_add(uint32_t* h, const LtGeom& G, const float4 (&v)[kLtIt], uint32_t tile,
                                       uint32_t len) {
    const uint32_t set = threadIdx.x & 1u;
#pragma unroll
    for (int it = 0; it < kLtIt; ++it) {
        const uint32_t e = 4 * (it * kLtThreads + threadIdx.x);
        if (e >= len) continue;  // len % 4 == 0: the load is inside the unit or outside it
        const uint32_t lv = lt_levels4(G, tile * (uint32_t)kFlatTile + e);
        lt_add1(h, set, v[it].x, lv & 3u);
        lt_add1(h, set, v[it].y, (lv >> 2) & 3u);
        lt_add1(h, set, v[it].z, (lv >> 4) & 3u);
        lt_add1(h, set, v[it].w, lv >> 6);
    }
}

// Tiles [t0, t1) of unit U into the LDS bins; the loads of tile t + 1 are issued
// before tile t is counted (wc_tol.hip tol_bin_tiles).  Steps of two tiles (twice
// the bytes in flight per workgroup) did not pay where only two workgroups fit a
// CU: k_ltol_solo<3> on C2 0.468 -> 0.457 ms (profiles/r11/README.md).
__device__ __forceinline__ void lt_bin_tiles(uint32_t* h, const float* __restrict__ coef, const UnitDev& U,
                                             const LtGeom& G, uint32_t t0, uint32_t t1) {
    if (t0 >= t1) return;
    float4 cur[kLtIt], nxt[kLtIt];
    uint32_t len = lt_load(cur, coef, U, t0), nlen = 0;
    for (uint32_t t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;  // uniform
        if (more) nlen = lt_load(nxt, coef, U, t + 1);
        lt_add(h, G, cur, t, len);
        if (more) {
#pragma unroll
            for (int it = 0; it < kLtIt; ++it) cur[it] = nxt[it];
            len = nlen;
        }
    }
}

__device__ __forceinline__ float lt_bin_threshold(int bstar) {
    if (bstar <= 0) return 0.0f;
    if (bstar >= 0xFF0) return __uint_as_float(0x7f7fffffu);  // FLT_MAX: only +-inf is kept
    return __uint_as_float(((uint32_t)bstar << kHistShift) - 1u);
}

// The selection rule (include/wavelet_amd.h, wc_tol_levels_threshold) by one
// full wave (lane ln): level 1's counts at h, level l >= 2's at h + off2 +
// (l - 2) * kHistBins.  64 values of s per round, each lane the energy bounds
// of its s at every level; the nonempty pairs are then taken in (s, l) order
// (S is rounded after every add, so the order is part of the rule).  Separate
// double multiplies and adds (-ffp-contract=off).  thresh: WC_MAX_LEVELS floats.
// Returns the pair the walk stopped at, (s*, l*), uniform over the wave; x < 0:
// it never stopped.
__device__ __forceinline__ int2 lt_pick(const uint32_t* h, int off2, int L, uint64_t N, double tol, int ln,
                                        float* thresh, double* bound) {
    const double budget = (tol * tol) * (double)N;
    double S = 0.0;
    int sstar = -1, lstar = 0;
    const int send = kHistBins + WC_LTOL_SHIFT * (L - 1);
    for (int base = 0; base < send && sstar < 0; base += kWave) {
        const int s = base + ln;
        double term[WC_MAX_LEVELS];
        unsigned long long m[WC_MAX_LEVELS], any = 0ull;
        double w = 8.0;  // 8^l, exact
#pragma unroll
        for (int l = 0; l < WC_MAX_LEVELS; ++l, w *= 8.0) {
            const int b = s - WC_LTOL_SHIFT * l;
            const bool in = l < L && b >= 0 && b < kHistBins;
            const uint32_t cnt = in ? h[(l ? off2 + (l - 1) * kHistBins : 0) + b] : 0u;
            // every |c| of bin b is below hi: the float with bits (b + 1) << 19, +inf from the last finite bin on
            const double hi = in && b < 0xFEF ? (double)__uint_as_float((uint32_t)(b + 1) << kHistShift)
                                              : (double)__builtin_inff();
            term[l] = (double)cnt * (w * (hi * hi));
            m[l] = __ballot(cnt != 0u);
            any |= m[l];
        }
        while (any && sstar < 0) {  // uniform
            const int j = __ffsll((long long)any) - 1;
            any &= any - 1;
#pragma unroll
            for (int l = 0; l < WC_MAX_LEVELS; ++l) {
                if (sstar >= 0 || !((m[l] >> j) & 1ull)) continue;  // uniform
                const double t = S + __shfl(term[l], j, kWave);
                if (!(t <= budget)) {
                    sstar = base + j;
                    lstar = l + 1;
                } else {
                    S = t;
                }
            }
        }
    }
    if (ln == 0) {
#pragma unroll
        for (int l = 1; l <= WC_MAX_LEVELS; ++l) {
            int bstar = kHistBins;
            if (sstar >= 0) bstar = min(max(sstar + (l < lstar ? 1 : 0) - WC_LTOL_SHIFT * (l - 1), 0), kHistBins);
            thresh[l - 1] = l <= L ? lt_bin_threshold(bstar) : 0.0f;
        }
        if (bound) *bound = N ? sqrt(S / (double)N) : 0.0;
    }
    return make_int2(sstar, lstar);
}

}  // namespace wc
