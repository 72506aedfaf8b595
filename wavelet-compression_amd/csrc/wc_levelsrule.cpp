// wc_levelsrule.cpp — what the multi-level mode (include/wavelet_amd.h) decides
// without a device: wc_levels_for, wc_payload_levels and the mode's argument
// checks.  It calls no device entry point (tests/cpp/test_thin.cpp links it so).
#include "wc_ctx.h"

#include <cstring>
#include <string>

using namespace wc;

namespace wc {

// The mode's preconditions, before anything is launched: a level per unit in
// 1..WC_MAX_LEVELS, and 2^L dividing every dimension of a unit with cells.
int validate_levels(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels) {
    if (n > 0 && !levels) return fail(c, WC_ERR_INVALID, "levels is NULL");
    for (int i = 0; i < n; ++i) {
        const int L = levels[i];
        if (L < 1 || L > WC_MAX_LEVELS)
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + ": levels " + std::to_string(L) + " outside 1.." +
                            std::to_string(WC_MAX_LEVELS));
        const wc_unit& u = units[i];
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        if (cells && L >= 2 && ((u.nx | u.ny | u.nz) & ((1 << L) - 1)))
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + " (" + std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" +
                            std::to_string(u.nz) + "): " + std::to_string(L) + " levels need W, H and D divisible by " +
                            std::to_string(1 << L) + " (wc_levels_for gives the levels a box admits)");
    }
    return WC_OK;
}

}  // namespace wc

extern "C" {

int wc_levels_for(int nx, int ny, int nz, int want) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return 1;
    int L = 1;
    while (L < want && L < WC_MAX_LEVELS && ((nx | ny | nz) & ((1 << (L + 1)) - 1)) == 0) ++L;
    return L;
}

int wc_payload_levels(const uint8_t* header, size_t len, int* levels) {
    if (!header || !levels || len < 20) return WC_ERR_INVALID;
    int32_t h[4];
    std::memcpy(h, header, sizeof h);
    if (h[0] < 0 || h[1] < 0 || h[2] < 0) return WC_ERR_FORMAT;
    const uint64_t cells = (uint64_t)h[0] * (uint64_t)h[1] * (uint64_t)h[2];
    if (h[3] >= 0) {
        if ((uint64_t)h[3] != cells) return WC_ERR_FORMAT;
        *levels = 1;
        return WC_OK;
    }
    if (h[3] > -2 || h[3] < -WC_MAX_LEVELS) return WC_ERR_FORMAT;
    const int L = -h[3];
    if (cells > 0x7fffffffull || (cells && ((h[0] | h[1] | h[2]) & ((1 << L) - 1)))) return WC_ERR_FORMAT;
    *levels = L;
    return WC_OK;
}

}  // extern "C"
