// wc_leveltolhost.cpp — host form of the RMSE tolerance on the multi-level
// transform (include/wavelet_amd.h): wc_forward_levels_tol_host.  The selection
// rule on one unit's counts (wc_tol_levels_threshold) is in wc_leveltolrule.cpp,
// a translation unit without the HIP runtime.
//
// The entry point is its argument checks and a call of forward_serial
// (wc_hostserial.cpp) with wc_forward_levels_tol as the device step and
// wc_inverse_levels + wc_rmse as the round trip.
#include "wc_ctx.h"

using namespace wc;

extern "C" int wc_forward_levels_tol_host(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n,
                                          const int32_t* levels, const double* tol, uint8_t* payload, uint64_t cap,
                                          uint64_t* offsets, uint32_t* kept, float* thresh, double* bound,
                                          double* rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!cells || !payload || !offsets || !kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_levels(c, units, n, levels)) || (rc = validate_tol(c, units, n, tol))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) ||
        (rc = ensure(c, c->h_bound, sizeof(double) * n)))
        return rc;
    return forward_serial(
        c, cells, dtype, units, n, payload, cap, offsets, kept, rmse,
        [&](int a, int m, const void* d_cells, uint8_t* pay, uint64_t run_bound, uint64_t* doff, uint32_t* dkept) {
            return wc_forward_levels_tol(c, d_cells, dtype, units + a, m, levels + a, tol + a, pay, run_bound, doff,
                                         dkept, (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a,
                                         (double*)c->h_bound.p + a);
        },
        levels_round_trip(c, dtype, units, levels),
        {{c->h_thresh.p, thresh, sizeof(float) * WC_MAX_LEVELS}, {c->h_bound.p, bound, sizeof(double)}});
}
