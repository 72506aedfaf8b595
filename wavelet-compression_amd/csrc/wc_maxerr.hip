// wc_maxerr.hip — the pointwise (max-abs) error bound on the opt-in multi-level
// transform (wc_forward_levels_maxerr in include/wavelet_amd.h) and the L-inf
// sibling of the RMSE metric (wc_maxerr).
//
// Not part of the reference's codec.  The rule probes thresholds thr(b): every
// probe is the unit's masked inverse and the max of |x - R_b| over its cells,
// 16 probes per pass, three passes (radix 16 over the 4096 bins).  Haar is
// block-local: a cell tile aligned to 2^L on every axis depends on the
// coefficients of the tile's own index range on each level and on nothing
// else, so a workgroup inverts its tile alone and the whole search never
// leaves the device.
//
//   k_maxerr_probe<NL, T>  one pass.  Workgroup = one cell tile of TX x TY x TZ
//                  cells (x, y, z; clipped to the unit, so its extents stay
//                  multiples of 2^L): 16 x 8 x 32 for NL <= 3, 16 x 16 x 32 for
//                  NL = 4 (a 2^4 multiple on every axis).  Cells are x fastest,
//                  the flat array is x slowest (K fastest): 16 cells along x are
//                  a 64-B row piece in fp32, 32 cells along z are 16 level-1
//                  coefficients of each sub-band, a 64-B run.
//                  The tile's cells and its level-1 details are loaded ONCE into
//                  registers (NB = 2 or 4 blocks of 2x2x2 per thread); the
//                  tile's level-1 low-pass octant, which holds every level >= 2
//                  of the tile in the tile's own Mallat layout, is loaded once
//                  into LDS (sC).  Per batch of CB candidates: sW[c] = sC masked
//                  by thr_c; the level syntheses L..2 run on sW for all CB
//                  candidates at once (one read phase, a barrier, one write
//                  phase per level); then each candidate's level-1 synthesis in
//                  registers, |x - R| in double, a wave max, and after the last
//                  batch one atomicMax per (workgroup, candidate) on the uint64
//                  bits of the double (non-negative doubles order as their
//                  bits; NaN is never sent, 0 need not be).
//                  LDS: sC + CB x sC, rows padded by 4 floats so that the 8 x 4
//                  (bi, bk) lanes of a half wave hit 32 banks: 37 KiB (NL <= 3,
//                  CB = 16: 4 workgroups per CU) and 38 KiB (NL = 4, CB = 8).
//                  The pass's lo comes from the earlier passes' maxima and E in
//                  the prologue (uniform loads): nothing goes to the host.
//   k_maxerr_pick  one wave per unit after pass 3: b*, thr(b*) into the unit's
//                  internal threshold slots (entries 0..L-1, for the mask pass)
//                  and d_thresh[u], err(b*) into d_err[u].
//   k_maxerr<T>    the metric: one workgroup per flat tile (cell order), the
//                  same atomicMax into d_err[u] (zeroed by the caller).
// The mask pass and the emit are wc_leveltol.hip's and wc_emit.hip's, unchanged.
#include "wavelet_amd.h"
#include "wc_xform.h"

namespace wc {

constexpr int kMxCand = 16;  // candidates per pass: b = lo + i * stride, i = 0..15

__device__ __forceinline__ float mx_thr(uint32_t b) {
    return b == 0u ? 0.0f : b >= 0xFF0u ? __uint_as_float(0x7f7fffffu) : __uint_as_float((b << WC_HIST_SHIFT) - 1u);
}

// lo after `npass` passes of unit u, from their maxima (state[(q * n + u) * 16 + i] = err(lo_q + i * stride_q));
// *jlast: the last pass's j*.
__device__ __forceinline__ uint32_t mx_lo(const unsigned long long* state, int n, uint32_t u, int npass, double E,
                                          uint32_t* jlast) {
    uint32_t lo = 0u, j = 0u;
    for (int q = 0; q < npass; ++q) {
        const unsigned long long* s = state + ((size_t)q * n + u) * kMxCand;
        j = 0u;
        for (uint32_t i = 1u; i < (uint32_t)kMxCand; ++i) {
            if (!(__longlong_as_double((long long)s[i]) <= E)) break;
            j = i;
        }
        lo += j << (8 - 4 * q);
    }
    if (jlast) *jlast = j;
    return lo;
}

template <int NL>
struct MxTile {
    static constexpr int TX = 16, TY = NL == 4 ? 16 : 8, TZ = 32;
    static constexpr int NB = TX * TY * TZ / 8 / kThreads;           // level-1 blocks per thread
    static constexpr int CB = NL == 4 ? 8 : 16;                      // candidates per batch
    static constexpr int CMAX = (TX / 2) * ((TY / 2) * (TZ / 2) + 4);  // the padded low-pass octant
    static constexpr int MAXI = CB * (TX * TY * TZ / 64) / kThreads;  // level-pass items per thread
};

uint32_t maxerr_tiles(int maxl, int32_t nx, int32_t ny, int32_t nz) {
    const uint32_t ty = maxl == 4 ? 16 : 8;
    return (uint32_t)((nx + 15) / 16) * (((uint32_t)ny + ty - 1) / ty) * (uint32_t)((nz + 31) / 32);
}

template <int NL, typename T>
__global__ __launch_bounds__(kThreads) void k_maxerr_probe(const UnitDev* __restrict__ units,
                                                         const LtUnit* __restrict__ lt,
                                                         const uint32_t* __restrict__ prefix, int n, int pass,
                                                         const T* __restrict__ cells, const float* __restrict__ coef,
                                                         unsigned long long* state) {
    using M = MxTile<NL>;
    __shared__ float sC[M::CMAX];
    __shared__ float sW[M::CB * M::CMAX];
    __shared__ unsigned long long sred[4][kMxCand];
    __shared__ float sthr[kMxCand];

    // the unit of this tile: prefix[u] <= blockIdx.x < prefix[u + 1]
    uint32_t ua = 0u, ub = (uint32_t)n;
    while (ub - ua > 1u) {
        const uint32_t m = (ua + ub) >> 1;
        if (prefix[m] <= blockIdx.x) ua = m; else ub = m;
    }
    const uint32_t u = ua;
    const UnitDev& U = units[u];
    const LtUnit Tu = lt[u];
    const int L = (int)Tu.levels;
    const int W = U.nx, H = U.ny, D = U.nz;
    uint32_t t = blockIdx.x - prefix[u];
    const uint32_t ntz = (uint32_t)(D + M::TZ - 1) / M::TZ, nty = (uint32_t)(H + M::TY - 1) / M::TY;
    const int z0 = (int)(t % ntz) * M::TZ;
    t /= ntz;
    const int y0 = (int)(t % nty) * M::TY, x0 = (int)(t / nty) * M::TX;
    const int ex = min(M::TX, W - x0), ey = min(M::TY, H - y0), ez = min(M::TZ, D - z0);
    const int cx = ex >> 1, cy = ey >> 1, cz = ez >> 1;  // level-1 blocks = the low-pass octant
    const int S = cy * cz + 4;
    const int nb1 = cx * cy * cz;

    const uint32_t lo = mx_lo(state, n, u, pass, Tu.tol, nullptr);
    if (threadIdx.x < kMxCand) sthr[threadIdx.x] = mx_thr(lo + (threadIdx.x << (8 - 4 * pass)));

    const float* __restrict__ A = coef + U.coef_off;
    const T* __restrict__ X = cells + U.cell_off;
    // the octant: element (i, j, k) of the tile's own pyramid is of level l, the count of the corner boxes
    // (ex, ey, ez) >> 1..L-1 that hold it plus one; it sits in the unit's half (sx, sy, sz) of that level
    for (int idx = threadIdx.x; idx < nb1; idx += kThreads) {
        const int k = idx % cz, r = idx / cz, j = r % cy, i = r / cy;
        int l = 1;
        while (l < L && i < (ex >> l) && j < (ey >> l) && k < (ez >> l)) ++l;
        const int lx = ex >> l, ly = ey >> l, lz = ez >> l;
        const int64_t I = (x0 >> l) + (i >= lx ? i - lx + (W >> l) : i);
        const int64_t J = (y0 >> l) + (j >= ly ? j - ly + (H >> l) : j);
        const int64_t K = (z0 >> l) + (k >= lz ? k - lz + (D >> l) : k);
        sC[i * S + j * cz + k] = A[(I * H + J) * D + K];
    }

    // this thread's level-1 blocks: bi fastest (x pairs of a cell row side by side), then bk, then bj
    float det[M::NB][2][2][2];  // [0][0][0] unused: the low-pass comes from sW
    T xv[M::NB][2][2][2];
    int lp[M::NB];              // the block's low-pass in the octant, -1: no block
    const bool vec = (reinterpret_cast<uintptr_t>(X) % (2 * sizeof(T))) == 0;  // uniform; W is even
#pragma unroll
    for (int q = 0; q < M::NB; ++q) {
        const int b = threadIdx.x + q * kThreads;
        lp[q] = -1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            det[q][e >> 2][(e >> 1) & 1][e & 1] = 0.0f;
            xv[q][e >> 2][(e >> 1) & 1][e & 1] = (T)0;
        }
        if (b >= nb1) continue;
        const int bi = b % cx, r = b / cx, bk = r % cz, bj = r / cz;
        lp[q] = bi * S + bj * cz + bk;
        const int64_t I = (x0 >> 1) + bi, J = (y0 >> 1) + bj, K = (z0 >> 1) + bk;
#pragma unroll
        for (int e = 1; e < 8; ++e) {
            const int sx = e >> 2, sy = (e >> 1) & 1, sz = e & 1;
            det[q][sx][sy][sz] = A[((I + sx * (W >> 1)) * H + J + sy * (H >> 1)) * D + K + sz * (D >> 1)];
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const T* p = X + ((int64_t)(z0 + 2 * bk + dz) * H + (y0 + 2 * bj + dy)) * W + (x0 + 2 * bi);
                if (vec) {
                    typedef T T2 __attribute__((ext_vector_type(2)));
                    const T2 v = *reinterpret_cast<const T2*>(p);
                    xv[q][0][dy][dz] = v.x;
                    xv[q][1][dy][dz] = v.y;
                } else {
                    xv[q][0][dy][dz] = p[0];
                    xv[q][1][dy][dz] = p[1];
                }
            }
    }
    __syncthreads();  // sC, sthr

    const int plane = cy * cz;
    for (int c0 = 0; c0 < kMxCand; c0 += M::CB) {
        // sW[c] = the octant masked by candidate c0 + c
        for (int it = threadIdx.x; it < M::CB * nb1; it += kThreads) {
            const int c = it / nb1, idx = it - c * nb1;
            const int loc = (idx / plane) * S + idx % plane;
            const float v = sC[loc];
            sW[c * M::CMAX + loc] = fabsf(v) > sthr[c0 + c] ? v : 0.0f;
        }
        __syncthreads();
        // level syntheses l = L..2 on the corner (cx, cy, cz) >> (l - 2), every candidate of the batch at once
        for (int l = L; l >= 2; --l) {
            const int hw = cx >> (l - 1), hh = cy >> (l - 1), hd = cz >> (l - 1);
            const int nbl = hw * hh * hd, items = M::CB * nbl;
            float v[M::MAXI][2][2][2];
#pragma unroll
            for (int r = 0; r < M::MAXI; ++r) {
                const int it = threadIdx.x + r * kThreads;
                if (it >= items) continue;
                const int c = it / nbl, blk = it - c * nbl;
                const int bk = blk % hd, rr = blk / hd, bj = rr % hh, bi = rr / hh;
                const float* w = sW + c * M::CMAX;
                float cc[2][2][2];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int sx = e >> 2, sy = (e >> 1) & 1, sz = e & 1;
                    cc[sx][sy][sz] = w[(bi + sx * hw) * S + (bj + sy * hh) * cz + bk + sz * hd];
                }
                haar8_inv(cc, v[r]);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < M::MAXI; ++r) {
                const int it = threadIdx.x + r * kThreads;
                if (it >= items) continue;
                const int c = it / nbl, blk = it - c * nbl;
                const int bk = blk % hd, rr = blk / hd, bj = rr % hh, bi = rr / hh;
                float* w = sW + c * M::CMAX;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int dx = e >> 2, dy = (e >> 1) & 1, dz = e & 1;
                    w[(2 * bi + dx) * S + (2 * bj + dy) * cz + 2 * bk + dz] = v[r][dx][dy][dz];
                }
            }
            __syncthreads();
        }
        // level 1 in registers, one candidate after another
        for (int c = 0; c < M::CB; ++c) {
            const float th = sthr[c0 + c];
            const float* w = sW + c * M::CMAX;
            double m = 0.0;
#pragma unroll
            for (int q = 0; q < M::NB; ++q) {
                float cc[2][2][2], R[2][2][2];
#pragma unroll
                for (int e = 1; e < 8; ++e) {
                    const float d = det[q][e >> 2][(e >> 1) & 1][e & 1];
                    cc[e >> 2][(e >> 1) & 1][e & 1] = fabsf(d) > th ? d : 0.0f;
                }
                cc[0][0][0] = lp[q] >= 0 ? w[lp[q]] : 0.0f;
                haar8_inv(cc, R);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const double d =
                        fabs((double)xv[q][e >> 2][(e >> 1) & 1][e & 1] - (double)R[e >> 2][(e >> 1) & 1][e & 1]);
                    if (d > m) m = d;  // false for NaN
                }
            }
            const unsigned long long wm = wave_max_u64_u((unsigned long long)__double_as_longlong(m));
            if ((threadIdx.x & (kWave - 1)) == 0) sred[threadIdx.x >> 6][c0 + c] = wm;
        }
        __syncthreads();  // sW is free again; after the last batch: sred
    }
    if (threadIdx.x < kMxCand) {
        unsigned long long m = sred[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = sred[w][threadIdx.x] > m ? sred[w][threadIdx.x] : m;
        if (m) atomicMax(state + ((size_t)pass * n + u) * kMxCand + threadIdx.x, m);
    }
}

// Workgroup u (one wave): unit u's b* from the three passes' maxima.
__global__ __launch_bounds__(kWave) void k_maxerr_pick(const UnitDev* __restrict__ units, const LtUnit* __restrict__ lt,
                                                     int n, const unsigned long long* __restrict__ state,
                                                     float* __restrict__ slots, float* __restrict__ thresh,
                                                     double* __restrict__ err) {
    const uint32_t u = blockIdx.x;
    if (threadIdx.x != 0) return;
    const LtUnit Tu = lt[u];
    float th = 0.0f;
    double e = 0.0;
    if (units[u].ncells) {
        uint32_t j = 0u;
        th = mx_thr(mx_lo(state, n, u, 3, Tu.tol, &j));
        e = __longlong_as_double((long long)state[((size_t)2 * n + u) * kMxCand + j]);  // err(lo_3 + j) = err(b*)
    }
    for (uint32_t l = 0; l < Tu.levels; ++l) slots[(size_t)u * WC_MAX_LEVELS + l] = th;
    if (thresh) thresh[u] = th;
    if (err) err[u] = e;
}

// Workgroup t: the cells of flat tile tiles[t] (cell order) of its unit.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_maxerr(const T* __restrict__ orig, const float* __restrict__ regen,
                                                   const UnitDev* __restrict__ units, const FTile* __restrict__ tiles,
                                                   unsigned long long* __restrict__ err) {
    __shared__ unsigned long long s_w[4];
    const FTile ft = tiles[blockIdx.x];
    const UnitDev& U = units[ft.unit];
    const int64_t start = (int64_t)ft.index * kFlatTile;
    const int len = (int)min((int64_t)kFlatTile, (int64_t)U.ncells - start);
    const T* __restrict__ a = orig + U.cell_off + start;
    const float* __restrict__ b = regen + U.cell_off + start;
    double m = 0.0;
    for (int i = threadIdx.x; i < len; i += kThreads) {
        const double d = fabs((double)a[i] - (double)b[i]);
        if (d > m) m = d;  // false for NaN
    }
    const unsigned long long wm = wave_max_u64_u((unsigned long long)__double_as_longlong(m));
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x >> 6] = wm;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = s_w[0];
        for (int w = 1; w < 4; ++w) r = s_w[w] > r ? s_w[w] : r;
        if (r) atomicMax(err + ft.unit, r);
    }
}

template <int NL>
static hipError_t probe_passes(hipStream_t st, const UnitDev* units, const LtUnit* lt, const uint32_t* prefix, int n,
                               uint32_t ntiles, const void* cells, int dtype, const float* coef,
                               unsigned long long* state) {
    for (int pass = 0; pass < 3; ++pass) {
        if (dtype == WC_F64)
            k_maxerr_probe<NL, double>
                <<<ntiles, kThreads, 0, st>>>(units, lt, prefix, n, pass, (const double*)cells, coef, state);
        else
            k_maxerr_probe<NL, float>
                <<<ntiles, kThreads, 0, st>>>(units, lt, prefix, n, pass, (const float*)cells, coef, state);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// prefix[n + 1]: the units' first probe tiles (maxerr_tiles of maxl); state: 3 x n x 16 words, zeroed;
// slots: n x WC_MAX_LEVELS floats for the mask pass.
hipError_t launch_maxerr_select(hipStream_t st, const UnitDev* units, int n, const LtUnit* lt, const uint32_t* prefix,
                                uint32_t ntiles, int maxl, const void* cells, int dtype, const float* coef,
                                unsigned long long* state, float* slots, float* thresh, double* err) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (ntiles) {
        switch (maxl) {
            case 1: e = probe_passes<1>(st, units, lt, prefix, n, ntiles, cells, dtype, coef, state); break;
            case 2: e = probe_passes<2>(st, units, lt, prefix, n, ntiles, cells, dtype, coef, state); break;
            case 3: e = probe_passes<3>(st, units, lt, prefix, n, ntiles, cells, dtype, coef, state); break;
            default: e = probe_passes<4>(st, units, lt, prefix, n, ntiles, cells, dtype, coef, state); break;
        }
        if (e != hipSuccess) return e;
    }
    k_maxerr_pick<<<(uint32_t)n, kWave, 0, st>>>(units, lt, n, state, slots, thresh, err);
    return hipGetLastError();
}

// err: n doubles, zeroed.
hipError_t launch_maxerr(hipStream_t st, const void* orig, int dtype, const float* regen, const UnitDev* units,
                         const FTile* ftiles, uint32_t nft, double* err) {
    if (!nft) return hipSuccess;
    if (dtype == WC_F64)
        k_maxerr<double><<<nft, kThreads, 0, st>>>((const double*)orig, regen, units, ftiles, (unsigned long long*)err);
    else
        k_maxerr<float><<<nft, kThreads, 0, st>>>((const float*)orig, regen, units, ftiles, (unsigned long long*)err);
    return hipGetLastError();
}

}  // namespace wc
