// wc_leveltolrule.cpp — the selection rule of the multi-level RMSE-tolerance
// mode on one unit's per-level bin counts (wc_tol_levels_threshold in
// include/wavelet_amd.h): the host restatement of wc_leveltol.hip's lt_pick.
//
// Plain C++ without the HIP runtime, so that tests/cpp/test_leveltol.cpp links
// this file alone under a sanitizer.  With levels = 1 it is wc_tol_threshold
// (wc_tolhost.cpp) operation for operation.
#include "wavelet_amd.h"

#include <cmath>
#include <cstring>

namespace {

// the threshold that keeps exactly the bins >= bstar under the emit's strict |c| > thresh
float bin_threshold(int bstar) {
    uint32_t bits;
    if (bstar <= 0) bits = 0u;                                      // 0.0f: every non-zero coefficient kept
    else if (bstar >= 0xFF0) bits = 0x7f7fffffu;                    // FLT_MAX: only +-inf kept
    else bits = ((uint32_t)bstar << WC_HIST_SHIFT) - 1u;
    float t;
    std::memcpy(&t, &bits, 4);
    return t;
}

}  // namespace

extern "C" int wc_tol_levels_threshold(const uint64_t* counts, int levels, uint64_t ncoeff, double tol, float* thresh,
                                       double* bound) {
    if (!counts || !thresh || !(tol >= 0.0)) return WC_ERR_INVALID;
    if (levels < 1 || levels > WC_MAX_LEVELS) return WC_ERR_INVALID;
    const double budget = (tol * tol) * (double)ncoeff;
    double S = 0.0;
    int sstar = -1, lstar = 0;  // the pair the walk stopped at (none: sstar < 0)
    const int send = WC_HIST_BINS + WC_LTOL_SHIFT * (levels - 1);
    for (int s = 0; s < send && sstar < 0; ++s) {
        double w = 8.0;  // 8^l, exact
        for (int l = 1; l <= levels; ++l, w *= 8.0) {
            const int b = s - WC_LTOL_SHIFT * (l - 1);
            if (b < 0 || b >= WC_HIST_BINS) continue;
            const uint64_t cnt = counts[(size_t)(l - 1) * WC_HIST_BINS + b];
            if (!cnt) continue;
            double hi = (double)__builtin_inff();
            if (b < 0xFEF) {
                const uint32_t bits = (uint32_t)(b + 1) << WC_HIST_SHIFT;
                float f;
                std::memcpy(&f, &bits, 4);
                hi = (double)f;
            }
            const double t = S + (double)cnt * (w * (hi * hi));
            if (!(t <= budget)) {
                sstar = s;
                lstar = l;
                break;
            }
            S = t;
        }
    }
    for (int l = 1; l <= levels; ++l) {
        int bstar = WC_HIST_BINS;
        if (sstar >= 0) {
            bstar = sstar + (l < lstar ? 1 : 0) - WC_LTOL_SHIFT * (l - 1);
            bstar = bstar < 0 ? 0 : bstar > WC_HIST_BINS ? WC_HIST_BINS : bstar;
        }
        thresh[l - 1] = bin_threshold(bstar);
    }
    if (bound) *bound = ncoeff ? std::sqrt(S / (double)ncoeff) : 0.0;
    return WC_OK;
}
