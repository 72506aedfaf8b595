// wc_regionrule.cpp — the host-only helpers of the sub-box decode
// (include/wavelet_amd.h "Opt-in sub-box decode"): wc_region_align and
// wc_region_units.  Plain C++ without HIP: tests/cpp/test_regionrule.cpp links
// this file alone, with the index map of wc_regionmap.h, under ASan + UBSan.
#include "wavelet_amd.h"

#include <stdint.h>

namespace {

// one axis: [x0, x0 + n) inside [0, N), rounded outward to multiples of m + 1 (N is one)
bool align_axis(int32_t N, int32_t x0, int32_t n, int32_t m, int32_t* a0, int32_t* an) {
    if (x0 < 0 || n < 0 || (int64_t)x0 + n > (int64_t)N) return false;
    const int32_t lo = x0 & ~m;
    const int32_t hi = n == 0 ? lo : (int32_t)(((int64_t)x0 + n + m) & ~(int64_t)m);  // <= N: m + 1 divides N
    *a0 = lo;
    *an = hi - lo;
    return true;
}

}  // namespace

extern "C" {

int wc_region_align(int32_t nx, int32_t ny, int32_t nz, int levels, const wc_region* want, wc_region* aligned) {
    if (!want || !aligned || nx < 0 || ny < 0 || nz < 0 || levels < 1 || levels > WC_MAX_LEVELS) return WC_ERR_INVALID;
    const int32_t m = (1 << levels) - 1;
    const bool cells = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz != 0;
    if (cells && ((nx | ny | nz) & m)) return WC_ERR_INVALID;
    wc_region a{0, 0, 0, 0, 0, 0};
    if (!cells) {  // a box without cells holds the all-zero region only
        if (want->x0 | want->y0 | want->z0 | want->nx | want->ny | want->nz) return WC_ERR_INVALID;
    } else if (!align_axis(nx, want->x0, want->nx, m, &a.x0, &a.nx) ||
               !align_axis(ny, want->y0, want->ny, m, &a.y0, &a.ny) ||
               !align_axis(nz, want->z0, want->nz, m, &a.z0, &a.nz)) {
        return WC_ERR_INVALID;
    }
    *aligned = a;
    return WC_OK;
}

int wc_region_units(const wc_unit* units, const wc_region* regions, const int32_t* reduce, int n, wc_unit* out,
                    uint64_t* extent) {
    if (n < 0 || (n > 0 && (!units || !regions || !out)) || !extent) return WC_ERR_INVALID;
    uint64_t cur = 0, ext = 0;
    for (int i = 0; i < n; ++i) {
        const wc_region& g = regions[i];
        const int r = reduce ? reduce[i] : 0;
        if (g.nx < 0 || g.ny < 0 || g.nz < 0 || r < 0 || r > WC_MAX_LEVELS) return WC_ERR_INVALID;
        cur = (cur + 3) & ~uint64_t(3);
        out[i] = wc_unit{cur, g.nx >> r, g.ny >> r, g.nz >> r, 0};
        cur += (uint64_t)out[i].nx * (uint64_t)out[i].ny * (uint64_t)out[i].nz;
        ext = cur;
    }
    *extent = ext;
    return WC_OK;
}

}  // extern "C"
