// wc_maxerrrule.cpp — the selection rule of the pointwise (max-abs) error bound
// on one unit (wc_maxerr_select in include/wavelet_amd.h): the host restatement
// of wc_maxerr.hip's probe passes and pick.  Every probe is a full masked
// inverse of the unit's final flat array (the level syntheses L..2 on the
// low-pass corner, then the one-level inverse: X, then Y, then Z sweeps, avg +
// diff and avg - diff in fp32) and a max over |x - R| in double.
//
// Plain C++ without the HIP runtime, so that tests/cpp/test_maxerr.cpp links
// this file alone under a sanitizer.
#include "wavelet_amd.h"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

// thr(b): wc_tol_threshold's threshold from a first kept bin
float thr_of_bin(uint32_t b) {
    if (b == 0u) return 0.0f;
    if (b >= 0xFF0u) return FLT_MAX;
    const uint32_t bits = (b << WC_HIST_SHIFT) - 1u;
    float t;
    std::memcpy(&t, &bits, 4);
    return t;
}

// One synthesis on the corner (w, h, d) of A (strides H * D, D, 1): sub-band (sx, sy, sz) of block (i, j, k) at
// (i + sx*w/2, j + sy*h/2, k + sz*d/2) -> the block's cells at (2i + dx, 2j + dy, 2k + dz) of `out`, with
// strides (so, to, 1): compact (h * d, d) for a level pass, or the cell order for the last one.
template <class Put>
void synth(const float* A, size_t H, size_t D, size_t w, size_t h, size_t d, Put put) {
    const size_t hw = w / 2, hh = h / 2, hd = d / 2;
    for (size_t i = 0; i < hw; ++i)
        for (size_t j = 0; j < hh; ++j)
            for (size_t k = 0; k < hd; ++k) {
                float c[2][2][2], X[2][2][2], Y[2][2][2];
                for (int sx = 0; sx < 2; ++sx)
                    for (int sy = 0; sy < 2; ++sy)
                        for (int sz = 0; sz < 2; ++sz)
                            c[sx][sy][sz] = A[((i + sx * hw) * H + j + sy * hh) * D + k + sz * hd];
                for (int t = 0; t < 2; ++t)
                    for (int s = 0; s < 2; ++s) {
                        X[0][t][s] = c[0][t][s] + c[1][t][s];
                        X[1][t][s] = c[0][t][s] - c[1][t][s];
                    }
                for (int x = 0; x < 2; ++x)
                    for (int s = 0; s < 2; ++s) {
                        Y[x][0][s] = X[x][0][s] + X[x][1][s];
                        Y[x][1][s] = X[x][0][s] - X[x][1][s];
                    }
                for (int x = 0; x < 2; ++x)
                    for (int y = 0; y < 2; ++y) {
                        put(2 * i + x, 2 * j + y, 2 * k, Y[x][y][0] + Y[x][y][1]);
                        put(2 * i + x, 2 * j + y, 2 * k + 1, Y[x][y][0] - Y[x][y][1]);
                    }
            }
}

struct Unit {
    const float* flat;
    const void* cells;
    int dtype;
    size_t W, H, D;
    int L;
    std::vector<float> A, side;

    // err(b): the max over the non-NaN |x - R_b|, 0.0 without any
    double err(uint32_t b) {
        const float t = thr_of_bin(b);
        const size_t n = W * H * D;
        for (size_t p = 0; p < n; ++p) A[p] = std::fabs(flat[p]) > t ? flat[p] : 0.0f;  // strict: NaN goes
        for (int l = L; l >= 2; --l) {
            const size_t w = W >> (l - 1), h = H >> (l - 1), d = D >> (l - 1);
            synth(A.data(), H, D, w, h, d, [&](size_t x, size_t y, size_t z, float v) { side[(x * h + y) * d + z] = v; });
            for (size_t x = 0; x < w; ++x)
                for (size_t y = 0; y < h; ++y)
                    std::memcpy(&A[(x * H + y) * D], &side[(x * h + y) * d], sizeof(float) * d);
        }
        double m = 0.0;
        synth(A.data(), H, D, W, H, D, [&](size_t x, size_t y, size_t z, float v) {
            const size_t q = (z * H + y) * W + x;  // the cells are x fastest
            const double o = dtype == WC_F64 ? ((const double*)cells)[q] : (double)((const float*)cells)[q];
            const double e = std::fabs(o - (double)v);
            if (e > m) m = e;  // false for NaN
        });
        return m;
    }
};

}  // namespace

extern "C" int wc_maxerr_select(const float* flat, const void* cells, int dtype, int32_t nx, int32_t ny, int32_t nz,
                                int levels, double maxerr, float* thresh, double* err, uint32_t* bstar) {
    if (levels < 1 || levels > WC_MAX_LEVELS || nx < 0 || ny < 0 || nz < 0) return WC_ERR_INVALID;
    if (dtype != WC_F32 && dtype != WC_F64) return WC_ERR_INVALID;
    if (!(maxerr >= 0.0)) return WC_ERR_INVALID;  // NaN or negative
    const uint64_t n = (uint64_t)nx * ny * nz;
    if (n >= (uint64_t(1) << 31) || (n && (!flat || !cells))) return WC_ERR_INVALID;
    if (n && ((nx | ny | nz) & ((1 << levels) - 1))) return WC_ERR_INVALID;
    uint32_t lo = 0u;
    double e = 0.0;
    if (n) {
        Unit U{flat, cells, dtype, (size_t)nx, (size_t)ny, (size_t)nz, levels, {}, {}};
        U.A.resize(n);
        U.side.resize(n / 8 + 1);
        uint32_t at = 0xffffffffu;  // the bin e belongs to
        for (uint32_t stride = 256u; stride; stride >>= 4) {
            uint32_t j = 0u;
            for (uint32_t i = 1u; i <= 15u; ++i) {
                const double ei = U.err(lo + i * stride);
                if (!(ei <= maxerr)) break;
                j = i;
                e = ei;
                at = lo + i * stride;
            }
            lo += j * stride;
        }
        if (at != lo) e = U.err(lo);  // b* = 0: accepted unverified
    }
    if (thresh) *thresh = n ? thr_of_bin(lo) : 0.0f;
    if (err) *err = e;
    if (bstar) *bstar = lo;
    return WC_OK;
}
