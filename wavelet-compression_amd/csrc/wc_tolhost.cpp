// wc_tolhost.cpp — host side of the opt-in RMSE-tolerance mode
// (include/wavelet_amd.h): the selection rule on one unit's bin counts
// (wc_tol_threshold, the restatement of wc_tol.hip's tol_pick), the argument
// checks of the mode, and wc_forward_tol_host.
//
// wc_forward_tol_host is its argument checks and a call of forward_serial
// (wc_hostserial.cpp) with wc_forward_tol as the device step and
// wc_inverse_rmse as the round trip.
#include "wc_ctx.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace wc;

namespace wc {

// The mode's preconditions, before anything is launched: a tolerance per unit,
// each >= 0 (not NaN), and no unit with cells and an odd dimension.
int validate_tol(wc_ctx* c, const wc_unit* units, int n, const double* tol) {
    if (n > 0 && !tol) return fail(c, WC_ERR_INVALID, "tol is NULL");
    for (int i = 0; i < n; ++i) {
        if (!(tol[i] >= 0.0))
            return fail(c, WC_ERR_INVALID, "unit " + std::to_string(i) + ": tolerance is negative or NaN");
        const wc_unit& u = units[i];
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        if (cells && ((u.nx | u.ny | u.nz) & 1))
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + " (" + std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" +
                            std::to_string(u.nz) +
                            "): the RMSE-tolerance mode needs even W, H and D (the inverse transform does not "
                            "restore the trailing plane of an odd axis, so no error can be promised)");
    }
    return WC_OK;
}

}  // namespace wc

extern "C" {

int wc_tol_threshold(const uint64_t* counts, uint64_t ncoeff, double tol, float* thresh, double* bound) {
    if (!counts || !thresh || !(tol >= 0.0)) return WC_ERR_INVALID;
    const double budget = (tol * tol) * (double)ncoeff;
    double S = 0.0;
    int bstar = WC_HIST_BINS;
    for (int b = 0; b < WC_HIST_BINS; ++b) {
        if (!counts[b]) continue;
        double hi = (double)__builtin_inff();
        if (b < 0xFEF) {
            const uint32_t bits = (uint32_t)(b + 1) << WC_HIST_SHIFT;
            float f;
            std::memcpy(&f, &bits, 4);
            hi = (double)f;
        }
        const double t = S + (double)counts[b] * (8.0 * (hi * hi));
        if (!(t <= budget)) {
            bstar = b;
            break;
        }
        S = t;
    }
    float t;
    if (bstar == 0) {
        t = 0.0f;
    } else if (bstar >= 0xFF0) {
        const uint32_t bits = 0x7f7fffffu;  // FLT_MAX
        std::memcpy(&t, &bits, 4);
    } else {
        const uint32_t bits = ((uint32_t)bstar << WC_HIST_SHIFT) - 1u;
        std::memcpy(&t, &bits, 4);
    }
    *thresh = t;
    if (bound) *bound = ncoeff ? std::sqrt(S / (double)ncoeff) : 0.0;
    return WC_OK;
}

int wc_forward_tol_host(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n, const double* tol,
                        uint8_t* payload, uint64_t cap, uint64_t* offsets, uint32_t* kept, float* thresh,
                        double* bound, double* rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!cells || !payload || !offsets || !kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_tol(c, units, n, tol))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->h_thresh, sizeof(float) * n)) || (rc = ensure(c, c->h_bound, sizeof(double) * n))) return rc;
    return forward_serial(
        c, cells, dtype, units, n, payload, cap, offsets, kept, rmse,
        [&](int a, int m, const void* d_cells, uint8_t* pay, uint64_t run_bound, uint64_t* doff, uint32_t* dkept) {
            return wc_forward_tol(c, d_cells, dtype, units + a, m, tol + a, pay, run_bound, doff, dkept,
                                  (float*)c->h_thresh.p + a, (double*)c->h_bound.p + a);
        },
        [&](int a, int m, const uint8_t* pay, const uint64_t* doff) {
            return wc_inverse_rmse(c, pay, doff, units + a, m, c->h_cells.p, dtype, (float*)c->h_out.p,
                                   (double*)c->h_rmse.p + a);
        },
        {{c->h_thresh.p, thresh, sizeof(float)}, {c->h_bound.p, bound, sizeof(double)}});
}

}  // extern "C"
