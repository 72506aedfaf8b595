// wc_levels.hip — level passes of the opt-in multi-level transform
// (wc_forward_levels / wc_inverse_levels in include/wavelet_amd.h).
//
// Not part of the reference's codec, which transforms each box once
// (src/compressor.cpp:85-185).  A unit with L >= 2 levels repeats that
// one-level transform on the low-pass corner of its flat array A (x-slowest
// order (I*H + J)*D + K): level l = 2..L takes the sub-box
//     S(x, y, z) = A[(x*H + y)*D + z],  x < w, y < h, z < d,  (w, h, d) = (W, H, D) >> (l-1)
// as cells, transforms it (Z, then Y, then X sweeps: pairs along K, then J,
// then I; low at m, high at n/2 + m; haar_lo / haar_hi) and writes the result
// back into the same corner.  The inverse runs l = L..2 with the synthesis of
// k_inverse (X, then Y, then Z; avg +- diff).
//
// In-place hazard: output (i + sx*w/2, j + sy*h/2, k + sz*d/2) of block (i, j,
// k) lands on the inputs (2i.., 2j.., 2k..) of other blocks, which other
// workgroups may not have read yet.  So a pass never writes A: it writes the
// sub-box COMPACTLY (index (I*h + J)*d + K) into a side scratch of the context
// (unit u's part at coef_off / 8: N/8 floats hold level 2, later levels are
// smaller), and a second launch copies it back.  Every hand-off between
// workgroups is a kernel boundary.
//
//   k_level<true>   the analysis, one 2x2x2 block per thread (two along K with
//                 16-B loads when d % 4 == 0): A -> side
//   k_level<false>  the synthesis: A -> side
//   k_level_copy  side -> A's corner (16-B accesses when d % 4 == 0, else 8-B;
//                 d is even at every level and coef_off is 128-B aligned)
//   k_level_key   the unit's max key (wc_xform.h coef_key) over the FINAL staged
//                 array: K1's key describes the one-level array
//   k_level_headers  ncoeff = -L into the headers the emit wrote
//   k_level_flat  coefficient scratch <-> a caller's flat buffer (transform-only calls)
//
// Work lists (unit, chunk) come from the host per call (the levels are not part
// of the cached plan): a chunk is kLvBlocks 2x2x2 blocks of one unit's sub-box.
#include "wc_xform.h"

namespace wc {

constexpr int kLvBlocks = 4096;  // 2x2x2 blocks of a sub-box per workgroup (32768 coefficients)

// Analysis of one block, v[dx][dy][dz] -> c[sx][sy][sz]: the sweeps of
// xform_generic_p1 (src/compressor.cpp:98-175) with the flat axes as cells.
__device__ __forceinline__ void haar8_fwd(const float (&v)[2][2][2], float (&c)[2][2][2]) {
    float a[2][2][2], b[2][2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            a[x][y][0] = haar_lo(v[x][y][0], v[x][y][1]);
            a[x][y][1] = haar_hi(v[x][y][0], v[x][y][1]);
        }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            b[x][0][s] = haar_lo(a[x][0][s], a[x][1][s]);
            b[x][1][s] = haar_hi(a[x][0][s], a[x][1][s]);
        }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            c[0][t][s] = haar_lo(b[0][t][s], b[1][t][s]);
            c[1][t][s] = haar_hi(b[0][t][s], b[1][t][s]);
        }
}

// The sub-box of a unit at one level and this workgroup's run of its blocks.
struct LvBox {
    int H, D;        // the unit's flat strides
    int h, d;        // sub-box extents along J and K
    int hw, hh, hd;  // blocks per axis
    uint32_t b0, b1; // this workgroup's blocks [b0, b1)
};

__device__ __forceinline__ LvBox lv_box(const UnitDev& U, int shift, uint32_t chunk) {
    LvBox B;
    B.H = U.ny;
    B.D = U.nz;
    B.h = U.ny >> shift;
    B.d = U.nz >> shift;
    B.hw = U.nx >> (shift + 1);
    B.hh = B.h >> 1;
    B.hd = B.d >> 1;
    const uint32_t nblk = (uint32_t)B.hw * (uint32_t)B.hh * (uint32_t)B.hd;
    B.b0 = min(chunk * (uint32_t)kLvBlocks, nblk);
    B.b1 = min(B.b0 + (uint32_t)kLvBlocks, nblk);
    return B;
}

// FWD: blocks of A's corner -> their 8 sub-band positions of the compact side
// array.  !FWD: the 8 sub-band positions of A's corner -> the block's cells in
// the compact side array.
template <bool FWD>
__global__ __launch_bounds__(kThreads) void k_level(const UnitDev* __restrict__ units, const uint2* __restrict__ items,
                                                   int shift, const float* __restrict__ coef,
                                                   float* __restrict__ side, unsigned long long* __restrict__ key,
                                                   const uint32_t* __restrict__ bad) {
    const uint2 it = items[blockIdx.x];
    if (bad && bad[it.x] != kUnitRun) return;  // inverse: the decode refused the unit or its corner is its result
    const UnitDev& U = units[it.x];
    const LvBox B = lv_box(U, shift, it.y);
    const float* __restrict__ A = coef + U.coef_off;
    float* __restrict__ T = side + (U.coef_off >> 3);
    // K1's key describes the one-level array: k_level_key (a later launch) takes
    // the final array's from zero
    if (key && it.y == 0 && threadIdx.x == 0) key[it.x] = 0ull;
    const int64_t H = B.H, D = B.D, h = B.h, d = B.d;
    if ((B.hd & 1) == 0) {
        // two blocks along K per thread: 4 consecutive K of the cell side (16 B),
        // 2 consecutive K of each sub-band (8 B); kLvBlocks is even, so is hd
        const uint32_t hq = (uint32_t)B.hd >> 1;
        for (uint32_t q = (B.b0 >> 1) + threadIdx.x; q < (B.b1 >> 1); q += kThreads) {
            const uint32_t kq = q % hq, r = q / hq;
            const int64_t bj = r % (uint32_t)B.hh, bi = r / (uint32_t)B.hh;
            float v[2][2][2][2], c[2][2][2][2];  // [block along K][..]
            if constexpr (FWD) {
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        const float4 f =
                            *reinterpret_cast<const float4*>(A + ((2 * bi + x) * H + 2 * bj + y) * D + 4 * kq);
                        v[0][x][y][0] = f.x;
                        v[0][x][y][1] = f.y;
                        v[1][x][y][0] = f.z;
                        v[1][x][y][1] = f.w;
                    }
                haar8_fwd(v[0], c[0]);
                haar8_fwd(v[1], c[1]);
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            *reinterpret_cast<float2*>(T + ((bi + x * B.hw) * h + bj + y * B.hh) * d + s * B.hd +
                                                       2 * kq) = make_float2(c[0][x][y][s], c[1][x][y][s]);
            } else {
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
#pragma unroll
                        for (int s = 0; s < 2; ++s) {
                            const float2 f = *reinterpret_cast<const float2*>(
                                A + ((bi + x * B.hw) * H + bj + y * B.hh) * D + s * B.hd + 2 * kq);
                            c[0][x][y][s] = f.x;
                            c[1][x][y][s] = f.y;
                        }
                haar8_inv(c[0], v[0]);
                haar8_inv(c[1], v[1]);
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        *reinterpret_cast<float4*>(T + ((2 * bi + x) * h + 2 * bj + y) * d + 4 * kq) =
                            make_float4(v[0][x][y][0], v[0][x][y][1], v[1][x][y][0], v[1][x][y][1]);
            }
        }
        return;
    }
    // odd hd (the unit's last level when D / 2^L is odd): one block per thread,
    // 8-B accesses on the cell side, scalar ones on the sub-band side
    for (uint32_t b = B.b0 + threadIdx.x; b < B.b1; b += kThreads) {
        const uint32_t bk = b % (uint32_t)B.hd, r = b / (uint32_t)B.hd;
        const int64_t bj = r % (uint32_t)B.hh, bi = r / (uint32_t)B.hh;
        float v[2][2][2], c[2][2][2];
        if constexpr (FWD) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const float2 f = *reinterpret_cast<const float2*>(A + ((2 * bi + x) * H + 2 * bj + y) * D + 2 * bk);
                    v[x][y][0] = f.x;
                    v[x][y][1] = f.y;
                }
            haar8_fwd(v, c);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        T[((bi + x * B.hw) * h + bj + y * B.hh) * d + s * B.hd + bk] = c[x][y][s];
        } else {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        c[x][y][s] = A[((bi + x * B.hw) * H + bj + y * B.hh) * D + s * B.hd + bk];
            haar8_inv(c, v);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                    *reinterpret_cast<float2*>(T + ((2 * bi + x) * h + 2 * bj + y) * d + 2 * bk) =
                        make_float2(v[x][y][0], v[x][y][1]);
        }
    }
}

// The compact side array of a pass back into A's corner: chunk c of a unit is
// the 8 * kLvBlocks coefficients from 8 * kLvBlocks * c on (the items of k_level).
template <typename V>
__device__ __forceinline__ void level_copy_run(const float* __restrict__ T, float* __restrict__ A, const LvBox& B) {
    constexpr uint32_t N = sizeof(V) / sizeof(float);
    const uint32_t dv = (uint32_t)B.d / N;
    const uint32_t e1 = 8u * B.b1 / N;
    for (uint32_t e = 8u * B.b0 / N + threadIdx.x; e < e1; e += kThreads) {
        const uint32_t k = (e % dv) * N, r = e / dv;
        const int64_t j = r % (uint32_t)B.h, i = r / (uint32_t)B.h;
        *reinterpret_cast<V*>(A + (i * B.H + j) * B.D + k) = *reinterpret_cast<const V*>(T + (uint64_t)e * N);
    }
}

__global__ __launch_bounds__(kThreads) void k_level_copy(const UnitDev* __restrict__ units,
                                                       const uint2* __restrict__ items, int shift,
                                                       const float* __restrict__ side, float* __restrict__ coef,
                                                       const uint32_t* __restrict__ bad) {
    const uint2 it = items[blockIdx.x];
    if (bad && bad[it.x] != kUnitRun) return;
    const UnitDev& U = units[it.x];
    const LvBox B = lv_box(U, shift, it.y);
    const float* __restrict__ T = side + (U.coef_off >> 3);
    float* __restrict__ A = coef + U.coef_off;
    // 8 * b0 is a multiple of 4 and of d's vector width: runs of whole vectors
    if ((B.d & 3) == 0)
        level_copy_run<float4>(T, A, B);
    else
        level_copy_run<float2>(T, A, B);
}

// Flat tiles [items.y, + chunk) of unit items.x: the max key of the final
// staged array, one atomicMax per workgroup (the key was zeroed by the
// level-2 pass).  Largest |c|, then the smallest flat index: the order of the
// atomics does not matter.
constexpr int kKeyIt = kFlatTile / (4 * kThreads);
__global__ __launch_bounds__(kThreads) void k_level_key(const UnitDev* __restrict__ units,
                                                      const uint2* __restrict__ items, uint32_t chunk,
                                                      const float* __restrict__ coef,
                                                      unsigned long long* __restrict__ key) {
    __shared__ unsigned long long s[4];
    const uint2 it = items[blockIdx.x];
    const UnitDev& U = units[it.x];
    const uint32_t t1 = min(it.y + chunk, U.nftiles);
    unsigned long long kmax = 0;
    for (uint32_t t = it.y; t < t1; ++t) {
        const uint64_t start = (uint64_t)t * kFlatTile;
        const uint32_t len = (uint32_t)min((uint64_t)kFlatTile, U.ncells - start);
        // coef_off is 16-B aligned; the scratch keeps kFlatTile floats of slack
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(coef + U.coef_off + start);
#pragma unroll
        for (int i = 0; i < kKeyIt; ++i) {
            const uint32_t e = 4 * (i * kThreads + threadIdx.x);
            if (e >= len) continue;
            const float4 v = p4[e >> 2];
            const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < len) {
                    const unsigned long long k = coef_key(x[j], (uint32_t)(start + e + j));
                    kmax = k > kmax ? k : kmax;
                }
        }
    }
    block_key_max(kmax, s, key + it.x);
}

// items: (unit, L) of the units with L >= 2, after the emit wrote their
// headers in their slots.
__global__ __launch_bounds__(kThreads) void k_level_headers(const UnitDev* __restrict__ units,
                                                          const uint2* __restrict__ items, uint32_t nitems,
                                                          uint8_t* __restrict__ payload) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nitems) return;
    const uint2 it = items[i];
    reinterpret_cast<int32_t*>(payload + units[it.x].pay_off)[3] = -(int32_t)it.y;
}

// One flat tile of a unit between the coefficient scratch (at coef_off) and a
// caller's flat buffer (at cell_off, any element alignment).
__global__ __launch_bounds__(kThreads) void k_level_flat(const UnitDev* __restrict__ units,
                                                       const FTile* __restrict__ tiles, float* __restrict__ coef,
                                                       float* __restrict__ flat, int to_flat) {
    const FTile ft = tiles[blockIdx.x];
    const UnitDev& U = units[ft.unit];
    const uint64_t start = (uint64_t)ft.index * kFlatTile;
    const uint32_t len = (uint32_t)min((uint64_t)kFlatTile, U.ncells - start);
    float* __restrict__ a = coef + U.coef_off + start;
    float* __restrict__ b = flat + U.cell_off + start;
    for (uint32_t e = threadIdx.x; e < len; e += kThreads) {
        if (to_flat)
            b[e] = a[e];
        else
            a[e] = b[e];
    }
}

hipError_t launch_level(hipStream_t st, bool fwd, const UnitDev* units, const uint2* items, uint32_t nitems, int shift,
                        float* coef, float* side, unsigned long long* key, const uint32_t* bad) {
    if (!nitems) return hipSuccess;
    if (fwd)
        k_level<true><<<nitems, kThreads, 0, st>>>(units, items, shift, coef, side, key, bad);
    else
        k_level<false><<<nitems, kThreads, 0, st>>>(units, items, shift, coef, side, key, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_level_copy<<<nitems, kThreads, 0, st>>>(units, items, shift, side, coef, bad);
    return hipGetLastError();
}

hipError_t launch_level_key(hipStream_t st, const UnitDev* units, const uint2* items, uint32_t nitems, uint32_t chunk,
                            const float* coef, unsigned long long* key) {
    if (!nitems) return hipSuccess;
    k_level_key<<<nitems, kThreads, 0, st>>>(units, items, chunk, coef, key);
    return hipGetLastError();
}

hipError_t launch_level_headers(hipStream_t st, const UnitDev* units, const uint2* items, uint32_t nitems,
                                uint8_t* payload) {
    if (!nitems) return hipSuccess;
    k_level_headers<<<(nitems + kThreads - 1) / kThreads, kThreads, 0, st>>>(units, items, nitems, payload);
    return hipGetLastError();
}

hipError_t launch_level_flat(hipStream_t st, const UnitDev* units, const FTile* tiles, uint32_t ntiles, float* coef,
                             float* flat, int to_flat) {
    if (!ntiles) return hipSuccess;
    k_level_flat<<<ntiles, kThreads, 0, st>>>(units, tiles, coef, flat, to_flat);
    return hipGetLastError();
}

uint32_t level_chunk_blocks() { return (uint32_t)kLvBlocks; }

}  // namespace wc
