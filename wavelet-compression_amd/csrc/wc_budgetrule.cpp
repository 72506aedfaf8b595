// wc_budgetrule.cpp — the selection rule of the size-budget mode on one unit's
// final flat array (wc_budget_select, wc_budget_thresholds in
// include/wavelet_amd.h): the host restatement of wc_budget.hip's radix select,
// by a partial sort of the keys.
//
// Plain C++ without the HIP runtime, so that tests/cpp/test_budget.cpp links
// this file alone under a sanitizer.
#include "wavelet_amd.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

extern "C" int wc_budget_thresholds(uint32_t key, int levels, float* thresh) {
    if (!thresh || levels < 1 || levels > WC_MAX_LEVELS) return WC_ERR_INVALID;
    for (int l = 1; l <= levels; ++l) {
        const int64_t d = (int64_t)key - (int64_t)((uint32_t)(WC_LTOL_SHIFT * (l - 1)) << WC_HIST_SHIFT);
        const uint32_t bits = d <= 0 ? 0u : d >= 0x7f800000 ? 0x7f800000u : (uint32_t)d;
        std::memcpy(thresh + (l - 1), &bits, 4);
    }
    return WC_OK;
}

extern "C" int wc_budget_select(const float* flat, int32_t nx, int32_t ny, int32_t nz, int levels, uint32_t max_pairs,
                                uint32_t* key, float* thresh, uint32_t* kept) {
    if (!key || levels < 1 || levels > WC_MAX_LEVELS || nx < 0 || ny < 0 || nz < 0) return WC_ERR_INVALID;
    const uint64_t n = (uint64_t)nx * ny * nz;
    if (n >= (uint64_t(1) << 31) || (n && !flat)) return WC_ERR_INVALID;
    if (n && ((nx | ny | nz) & ((1 << levels) - 1))) return WC_ERR_INVALID;
    std::vector<uint32_t> keys;
    keys.reserve(n);
    for (int32_t i = 0; i < nx; ++i)
        for (int32_t j = 0; j < ny; ++j)
            for (int32_t k = 0; k < nz; ++k) {
                uint32_t m;
                std::memcpy(&m, flat + ((size_t)i * ny + j) * nz + k, 4);
                m &= 0x7fffffffu;
                if (m < 1u || m > 0x7f800000u) continue;  // +-0 and NaN are no candidates
                int lv = 0;  // level - 1: the count of the j in 1..L-1 whose corner box holds the position
                for (int s = 1; s < levels; ++s) lv += (i < (nx >> s) && j < (ny >> s) && k < (nz >> s)) ? 1 : 0;
                keys.push_back(m + ((uint32_t)(WC_LTOL_SHIFT * lv) << WC_HIST_SHIFT));
            }
    uint32_t T = 0u;
    if (keys.size() > max_pairs) {  // the (K + 1)-th largest, with multiplicity
        std::nth_element(keys.begin(), keys.begin() + max_pairs, keys.end(), std::greater<uint32_t>());
        T = keys[max_pairs];
    }
    *key = T;
    if (thresh) (void)wc_budget_thresholds(T, levels, thresh);
    if (kept) *kept = (uint32_t)std::count_if(keys.begin(), keys.end(), [T](uint32_t k) { return k > T; });
    return WC_OK;
}
