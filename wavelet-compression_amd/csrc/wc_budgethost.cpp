// wc_budgethost.cpp — host side of the size-budget mode (include/wavelet_amd.h):
// the mode's argument checks and wc_forward_levels_budget_host.  The selection
// rule on one unit's final array (wc_budget_select) is in wc_budgetrule.cpp, a
// translation unit without the HIP runtime.
//
// The entry point is its argument checks and a call of forward_serial
// (wc_hostserial.cpp) with wc_forward_levels_budget as the device step and
// wc_inverse_levels + wc_rmse as the round trip.
#include "wc_ctx.h"

#include <string>
#include <vector>

using namespace wc;

namespace wc {

// The mode's preconditions, before anything is launched: what validate_levels
// demands, and even dimensions of an L = 1 unit with cells (the 16-B loads of
// the select; 2^L covers it for L >= 2).
int validate_budget(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels) {
    int rc;
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    for (int i = 0; i < n; ++i) {
        const wc_unit& u = units[i];
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        if (cells && ((u.nx | u.ny | u.nz) & 1))
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + " (" + std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" +
                            std::to_string(u.nz) + "): the size-budget mode needs even W, H and D");
    }
    return WC_OK;
}

}  // namespace wc

extern "C" int wc_forward_levels_budget_host(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n,
                                             const int32_t* levels, const uint32_t* max_pairs, uint8_t* payload,
                                             uint64_t cap, uint64_t* offsets, uint32_t* kept, float* thresh,
                                             uint32_t* key, double* rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!cells || !payload || !offsets || !kept || !max_pairs) return fail(c, WC_ERR_INVALID, "null buffer");
    std::vector<int32_t> ones;
    levels = levels_or_ones(levels, n, ones);
    if ((rc = validate_budget(c, units, n, levels))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) ||
        (rc = ensure(c, c->h_bound, sizeof(uint32_t) * n)))  // the units' keys
        return rc;
    return forward_serial(
        c, cells, dtype, units, n, payload, cap, offsets, kept, rmse,
        [&](int a, int m, const void* d_cells, uint8_t* pay, uint64_t run_bound, uint64_t* doff, uint32_t* dkept) {
            return wc_forward_levels_budget(c, d_cells, dtype, units + a, m, levels + a, max_pairs + a, pay, run_bound,
                                            doff, dkept, (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a,
                                            (uint32_t*)c->h_bound.p + a);
        },
        levels_round_trip(c, dtype, units, levels),
        {{c->h_thresh.p, thresh, sizeof(float) * WC_MAX_LEVELS}, {c->h_bound.p, key, sizeof(uint32_t)}});
}
