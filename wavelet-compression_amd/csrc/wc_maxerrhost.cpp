// wc_maxerrhost.cpp — host side of the pointwise (max-abs) error bound
// (include/wavelet_amd.h): the mode's argument checks,
// wc_forward_levels_maxerr_host and wc_maxerr_host.  The rule on one unit
// (wc_maxerr_select) is in wc_maxerrrule.cpp, a translation unit without the
// HIP runtime.
//
// wc_forward_levels_maxerr_host is its argument checks and a call of
// forward_serial (wc_hostserial.cpp) with wc_forward_levels_maxerr as the
// device step and wc_inverse_levels + wc_rmse as the round trip.
#include "wc_ctx.h"

#include <string>
#include <vector>

using namespace wc;

namespace wc {

// The mode's preconditions, before anything is launched: what validate_levels
// demands, a bound per unit, each >= 0 (not NaN), and even dimensions of an
// L = 1 unit with cells (2^L covers it for L >= 2).
int validate_maxerr(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const double* maxerr) {
    int rc;
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    for (int i = 0; i < n; ++i) {
        if (!(maxerr[i] >= 0.0))
            return fail(c, WC_ERR_INVALID, "unit " + std::to_string(i) + ": the error bound is negative or NaN");
        const wc_unit& u = units[i];
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        if (cells && ((u.nx | u.ny | u.nz) & 1))
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + " (" + std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" +
                            std::to_string(u.nz) +
                            "): the max-error mode needs even W, H and D (the inverse transform does not restore "
                            "the trailing plane of an odd axis, so no error can be promised)");
    }
    return WC_OK;
}

}  // namespace wc

extern "C" {

int wc_forward_levels_maxerr_host(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n,
                                  const int32_t* levels, const double* maxerr, uint8_t* payload, uint64_t cap,
                                  uint64_t* offsets, uint32_t* kept, float* thresh, double* err, double* rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!cells || !payload || !offsets || !kept || !maxerr) return fail(c, WC_ERR_INVALID, "null buffer");
    std::vector<int32_t> ones;
    levels = levels_or_ones(levels, n, ones);
    if ((rc = validate_maxerr(c, units, n, levels, maxerr))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->h_thresh, sizeof(float) * n)) || (rc = ensure(c, c->h_bound, sizeof(double) * n))) return rc;
    return forward_serial(
        c, cells, dtype, units, n, payload, cap, offsets, kept, rmse,
        [&](int a, int m, const void* d_cells, uint8_t* pay, uint64_t run_bound, uint64_t* doff, uint32_t* dkept) {
            return wc_forward_levels_maxerr(c, d_cells, dtype, units + a, m, levels + a, maxerr + a, pay, run_bound,
                                            doff, dkept, (float*)c->h_thresh.p + a, (double*)c->h_bound.p + a);
        },
        levels_round_trip(c, dtype, units, levels), {{c->h_thresh.p, thresh, sizeof(float)}, {c->h_bound.p, err, sizeof(double)}});
}

int wc_maxerr_host(wc_ctx* c, const void* orig, int dtype, const float* regen, const wc_unit* units, int n,
                   double* err) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!orig || !regen || !err) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = set_device(c))) return rc;
    const size_t esz = dtype == WC_F64 ? 8 : 4;
    const uint64_t ext = cells_extent(units, n);
    if ((rc = ensure(c, c->h_cells, esz * ext)) || (rc = ensure(c, c->h_out, sizeof(float) * ext)) ||
        (rc = ensure(c, c->h_offsets, sizeof(double) * n)))
        return rc;
    hipError_t e;
    if ((e = hipMemcpyAsync(c->h_cells.p, orig, esz * ext, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->h_out.p, regen, sizeof(float) * ext, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return hip_fail(c, e, "maxerr upload");
    if ((rc = wc_maxerr(c, c->h_cells.p, dtype, (const float*)c->h_out.p, units, n, (double*)c->h_offsets.p))) return rc;
    if ((e = hipMemcpyAsync(err, c->h_offsets.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return hip_fail(c, e, "maxerr readback");
    return WC_OK;
}

}  // extern "C"
