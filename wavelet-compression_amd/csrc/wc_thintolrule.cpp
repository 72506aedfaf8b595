// wc_thintolrule.cpp — the tolerance rule of the compressed-domain thinning and
// split on one standard payload (wc_thin_tol_unit and wc_split_tol_unit in
// include/wavelet_amd.h): the host restatement of wc_thin.hip's tolerance form.
// The per-level bin counts of A(P) from the parsed pairs and the box, the
// thresholds from wc_tol_levels_threshold (wc_leveltolrule.cpp), then
// wc_thin_unit / wc_split_unit (wc_thinrule.cpp, wc_layersrule.cpp) at those
// thresholds.
//
// Plain C++ without the HIP runtime, so that tests/cpp/test_thin_tol.cpp links
// it under a sanitizer.
#include "wavelet_amd.h"

#include <cstring>
#include <vector>

namespace {

// thresh_1..L and bound of thin_tol(P, tol); L: the payload's levels
int tol_thresholds(const uint8_t* payload, size_t len, double tol, float* thresh, double* bound, int* levels) {
    if (!payload || len < 20 || !(tol >= 0.0)) return WC_ERR_INVALID;
    int L = 0;
    const int rc = wc_payload_levels(payload, 20, &L);  // a packed unit's tag is no level count: WC_ERR_FORMAT
    if (rc != WC_OK) return rc;
    int32_t h[5];
    std::memcpy(h, payload, sizeof h);
    if (h[4] < 0) return WC_ERR_FORMAT;
    const uint64_t W = (uint64_t)h[0], H = (uint64_t)h[1], D = (uint64_t)h[2], N = W * H * D, n = (uint64_t)h[4];
    if (N > 0x7fffffffull) return WC_ERR_FORMAT;
    if (len < 20 + 8 * n) return WC_ERR_INVALID;
    // the boxes wc_forward_levels_tol accepts: 2^L divides every dimension (L = 1: even dimensions)
    if (N && ((W | H | D) & ((1ull << L) - 1))) return WC_ERR_INVALID;
    std::vector<uint64_t> cnt((size_t)L * WC_HIST_BINS, 0);
    std::vector<uint64_t> pairs(L, 0);  // pairs of each level below N, NaN and +-0 included
    uint64_t p = 0;
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
        uint32_t lv = 0;  // level - 1
        for (int s = 1; s < L; ++s) lv += (I < (W >> s) && J < (H >> s) && K < (D >> s)) ? 1u : 0u;
        const uint32_t m = b & 0x7fffffffu;
        ++pairs[lv];
        if (m <= 0x7f800000u) ++cnt[(size_t)lv * WC_HIST_BINS + (m >> WC_HIST_SHIFT)];  // NaN counts nowhere
        ++p;
    }
    for (int l = 0; l < L; ++l) {  // the zeros of A(P)
        const uint64_t a = (W >> l) * (H >> l) * (D >> l);
        const uint64_t Nl = l + 1 < L ? a - (W >> (l + 1)) * (H >> (l + 1)) * (D >> (l + 1)) : a;
        cnt[(size_t)l * WC_HIST_BINS] += Nl - pairs[l];
    }
    *levels = L;
    return wc_tol_levels_threshold(cnt.data(), L, N, tol, thresh, bound);
}

}  // namespace

extern "C" int wc_thin_tol_unit(const uint8_t* payload, size_t len, double tol, uint8_t* out, size_t cap,
                                size_t* written, float* thresh_out, double* bound) {
    if (!out || !written) return WC_ERR_INVALID;
    float th[WC_MAX_LEVELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    double b = 0.0;
    int L = 0, rc;
    if ((rc = tol_thresholds(payload, len, tol, th, &b, &L)) != WC_OK) return rc;
    if ((rc = wc_thin_unit(payload, len, nullptr, th, out, cap, written, nullptr, nullptr)) != WC_OK) return rc;
    if (thresh_out) std::memcpy(thresh_out, th, sizeof(float) * (size_t)L);
    if (bound) *bound = b;
    return WC_OK;
}

extern "C" int wc_split_tol_unit(const uint8_t* payload, size_t len, double tol, uint8_t* base, size_t base_cap,
                                 size_t* base_len, uint8_t* rest, size_t rest_cap, size_t* rest_len,
                                 float* thresh_out, double* bound) {
    if (!base || !base_len || !rest || !rest_len) return WC_ERR_INVALID;
    float th[WC_MAX_LEVELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    double b = 0.0;
    int L = 0, rc;
    if ((rc = tol_thresholds(payload, len, tol, th, &b, &L)) != WC_OK) return rc;
    if ((rc = wc_split_unit(payload, len, nullptr, th, base, base_cap, base_len, rest, rest_cap, rest_len, nullptr,
                            nullptr)) != WC_OK)
        return rc;
    if (thresh_out) std::memcpy(thresh_out, th, sizeof(float) * (size_t)L);
    if (bound) *bound = b;
    return WC_OK;
}
