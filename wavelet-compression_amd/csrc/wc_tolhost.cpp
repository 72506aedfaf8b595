// wc_tolhost.cpp — host side of the opt-in RMSE-tolerance mode
// (include/wavelet_amd.h): the selection rule on one unit's bin counts
// (wc_tol_threshold, the restatement of wc_tol.hip's tol_pick), the argument
// checks of the mode, and wc_forward_tol_host.
//
// wc_forward_tol_host runs its unit runs (WC_OPT_HOST_CHUNK) one after another
// on the context's stream: upload the run's cells, wc_forward_tol, pack, the
// round trip's RMSE when asked for, download.  It is not pipelined over the
// copy streams as wc_forward_host is (wc_hostpipe.cpp).
#include "wc_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

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
    const size_t esz = dtype == WC_F64 ? 8 : 4;
    const uint64_t ext = cells_extent(units, n);

    // contiguous unit runs of at least opt_host_chunk cells (0: one run)
    std::vector<int> rb{0};
    if (c->opt_host_chunk > 0) {
        uint64_t acc = 0;
        for (int i = 0; i < n; ++i) {
            acc += (uint64_t)units[i].nx * units[i].ny * units[i].nz;
            if (acc >= (uint64_t)c->opt_host_chunk && i + 1 < n) {
                rb.push_back(i + 1);
                acc = 0;
            }
        }
    }
    rb.push_back(n);
    const int nr = (int)rb.size() - 1;
    uint64_t run_bound = 0;
    int run_units = 0;
    for (int r = 0; r < nr; ++r) {
        run_bound = std::max(run_bound, wc_payload_bound(units + rb[r], rb[r + 1] - rb[r]));
        run_units = std::max(run_units, rb[r + 1] - rb[r]);
    }
    if ((rc = ensure(c, c->h_cells, esz * ext)) || (rc = ensure(c, c->h_payload, run_bound)) ||
        (rc = ensure(c, c->h_packed, run_bound)) || (rc = ensure(c, c->h_offsets, sizeof(uint64_t) * (run_units + 1))) ||
        (rc = ensure(c, c->h_poff, sizeof(uint64_t) * (run_units + 1))) || (rc = ensure(c, c->h_kept, 4ull * run_units)) ||
        (rc = ensure(c, c->h_thresh, sizeof(float) * n)) || (rc = ensure(c, c->h_bound, sizeof(double) * n)))
        return rc;
    if (rmse && ((rc = ensure(c, c->h_out, sizeof(float) * ext)) || (rc = ensure(c, c->h_rmse, sizeof(double) * n))))
        return rc;

    std::vector<uint64_t> po(run_units + 1);
    uint64_t R = 4;  // run r's packed bytes [4, end) land at R (== 4 mod 8)
    auto run = [&](int r) -> int {
        const int a = rb[r], m = rb[r + 1] - rb[r];
        uint64_t lo = UINT64_MAX, hi = 0;
        for (int i = a; i < a + m; ++i) {
            const uint64_t cnt = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
            if (!cnt) continue;
            lo = std::min(lo, units[i].cell_offset);
            hi = std::max(hi, units[i].cell_offset + cnt);
        }
        hipError_t e;
        if (hi > lo && (e = hipMemcpyAsync((uint8_t*)c->h_cells.p + esz * lo, (const uint8_t*)cells + esz * lo,
                                           esz * (hi - lo), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return hip_fail(c, e, "cells upload");
        uint8_t* pay = (uint8_t*)c->h_payload.p;
        uint64_t* doff = (uint64_t*)c->h_offsets.p;
        uint64_t* dpoff = (uint64_t*)c->h_poff.p;
        uint32_t* dkept = (uint32_t*)c->h_kept.p;
        int rc2;
        if ((rc2 = wc_forward_tol(c, c->h_cells.p, dtype, units + a, m, tol + a, pay, run_bound, doff, dkept,
                                  (float*)c->h_thresh.p + a, (double*)c->h_bound.p + a)))
            return rc2;
        // pack the slots densely (offsets stay == 4 mod 8), as wc_forward_host does
        e = launch_pack(c->stream, (const UnitDev*)c->plan.d_units.p, m, dkept, pay, dpoff, (uint8_t*)c->h_packed.p);
        if (e != hipSuccess) return hip_fail(c, e, "pack launch");
        // the round trip: the run's payloads back to cells, compared with the cells on the device
        if (rmse && (rc2 = wc_inverse_rmse(c, pay, doff, units + a, m, c->h_cells.p, dtype, (float*)c->h_out.p,
                                           (double*)c->h_rmse.p + a)))
            return rc2;
        if ((e = hipMemcpyAsync(po.data(), dpoff, sizeof(uint64_t) * (m + 1), hipMemcpyDeviceToHost, c->stream)) !=
                hipSuccess ||
            (e = hipMemcpyAsync(kept + a, dkept, 4ull * m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return hip_fail(c, e, "sizes readback");
        for (int i = 0; i < m; ++i) offsets[a + i] = R - 4 + po[i];
        const uint64_t span = po[m] - 4;
        if (R - 4 + po[m] > cap) return fail(c, WC_ERR_INVALID, "payload_capacity");
        if (span && (e = hipMemcpyAsync(payload + R, (const uint8_t*)c->h_packed.p + 4, span, hipMemcpyDeviceToHost,
                                        c->stream)) != hipSuccess)
            return hip_fail(c, e, "payload readback");
        R += po[m];
        return WC_OK;
    };
    for (int r = 0; r < nr && rc == WC_OK; ++r) rc = run(r);
    hipError_t e = hipSuccess;
    if (rc == WC_OK) {
        offsets[n] = R - 4;
        if (thresh) e = hipMemcpyAsync(thresh, c->h_thresh.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && bound)
            e = hipMemcpyAsync(bound, c->h_bound.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && rmse)
            e = hipMemcpyAsync(rmse, c->h_rmse.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
    }
    // no copy that reads or writes the caller's buffers may outlive the call
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc != WC_OK) return rc;
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "results readback");
    return check_kernel_errors(c);
}

}  // extern "C"
