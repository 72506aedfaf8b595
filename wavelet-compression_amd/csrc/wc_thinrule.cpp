// wc_thinrule.cpp — the rule of the compressed-domain thinning on one standard
// payload (wc_thin_unit in include/wavelet_amd.h): the host restatement of
// wc_thin.hip.  The pairs' positions from the runs, the level of a position, the
// size-budget key (wc_budgetrule.cpp's) or the per-level threshold test on the
// kept pairs alone, and the reference's run rule on what is left.
//
// Plain C++ without the HIP runtime, so that tests/cpp/test_thin.cpp links it
// under a sanitizer.
#include "wavelet_amd.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

extern "C" int wc_thin_unit(const uint8_t* payload, size_t len, const uint32_t* max_pairs, const float* thresh,
                            uint8_t* out, size_t cap, size_t* written, uint32_t* key, float* thresh_out) {
    if (!payload || !out || !written || len < 20 || (max_pairs != nullptr) == (thresh != nullptr))
        return WC_ERR_INVALID;
    int L = 0;
    const int rc = wc_payload_levels(payload, 20, &L);  // a packed unit's tag is no level count: WC_ERR_FORMAT
    if (rc != WC_OK) return rc;
    int32_t h[5];
    std::memcpy(h, payload, sizeof h);
    if (h[4] < 0) return WC_ERR_FORMAT;
    const uint64_t N = (uint64_t)h[0] * (uint64_t)h[1] * (uint64_t)h[2], n = (uint64_t)h[4];
    if (N > 0x7fffffffull) return WC_ERR_FORMAT;
    if (len < 20 + 8 * n) return WC_ERR_INVALID;
    if (thresh)
        for (int l = 0; l < L; ++l)
            if (!(thresh[l] >= 0.0f)) return WC_ERR_INVALID;  // NaN or negative
    const uint64_t W = (uint64_t)h[0], H = (uint64_t)h[1], D = (uint64_t)h[2];
    // the pairs below N: position, value bits, key (budget) or kept flag (thresholds)
    std::vector<uint32_t> pos, bits, keys;
    uint64_t p = 0;  // the next pair's position if its run were 0
    bool live = true;  // positions only grow: after the first pair at or past N every pair is dropped
    for (uint64_t k = 0; k < n; ++k) {
        int32_t run;
        uint32_t b;
        std::memcpy(&run, payload + 20 + 8 * k, 4);
        std::memcpy(&b, payload + 24 + 8 * k, 4);
        if (run < 0) return WC_ERR_FORMAT;
        if (!live) continue;  // (still looking for a negative run)
        p += (uint64_t)run;
        if (p >= N) {
            live = false;
            continue;
        }
        const uint64_t row = p / D, K = p - row * D, I = row / H, J = row - I * H;
        uint32_t lv = 0;  // level - 1: the corner boxes (W, H, D) >> s that hold the position
        for (int s = 1; s < L; ++s) lv += (I < (W >> s) && J < (H >> s) && K < (D >> s)) ? 1u : 0u;
        const uint32_t m = b & 0x7fffffffu;
        uint32_t kk;
        if (max_pairs) {
            kk = (m >= 1u && m <= 0x7f800000u) ? m + ((uint32_t)(WC_LTOL_SHIFT * lv) << WC_HIST_SHIFT) : 0u;
        } else {
            float a;
            std::memcpy(&a, &m, 4);
            kk = a > thresh[lv] ? 1u : 0u;  // strict: false for NaN
        }
        pos.push_back((uint32_t)p);
        bits.push_back(b);
        keys.push_back(kk);
        ++p;
    }
    uint32_t T = 0u;
    if (max_pairs) {
        std::vector<uint32_t> cand;
        cand.reserve(keys.size());
        for (uint32_t kk : keys)
            if (kk) cand.push_back(kk);
        if (cand.size() > *max_pairs) {  // the (K + 1)-th largest, with multiplicity
            std::nth_element(cand.begin(), cand.begin() + *max_pairs, cand.end(), std::greater<uint32_t>());
            T = cand[*max_pairs];
        }
    }
    size_t kept = 0;
    for (uint32_t kk : keys) kept += kk > T ? 1 : 0;
    if (cap < 20 + 8 * kept) return WC_ERR_INVALID;
    h[4] = (int32_t)kept;
    std::memcpy(out, h, sizeof h);
    uint8_t* o = out + 20;
    int64_t last = -1;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (!(keys[i] > T)) continue;
        const int32_t run = (int32_t)((int64_t)pos[i] - last - 1);
        std::memcpy(o, &run, 4);
        std::memcpy(o + 4, &bits[i], 4);
        o += 8;
        last = (int64_t)pos[i];
    }
    *written = 20 + 8 * kept;
    if (key) *key = T;
    if (thresh_out) {
        if (max_pairs)
            (void)wc_budget_thresholds(T, L, thresh_out);
        else
            std::memcpy(thresh_out, thresh, sizeof(float) * L);
    }
    return WC_OK;
}
