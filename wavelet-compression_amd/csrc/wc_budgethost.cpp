// wc_budgethost.cpp — host side of the size-budget mode (include/wavelet_amd.h):
// the mode's argument checks and wc_forward_levels_budget_host.  The selection
// rule on one unit's final array (wc_budget_select) is in wc_budgetrule.cpp, a
// translation unit without the HIP runtime.
//
// As wc_forward_levels_tol_host, the unit runs (WC_OPT_HOST_CHUNK) go one after
// another on the context's stream: upload the run's cells,
// wc_forward_levels_budget, pack, the round trip's RMSE when asked for
// (wc_inverse_levels + wc_rmse), download.
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
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
    if (!levels) {
        ones.assign(n, 1);
        levels = ones.data();
    }
    if ((rc = validate_budget(c, units, n, levels))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = set_device(c))) return rc;
    const size_t esz = dtype == WC_F64 ? 8 : 4;
    const uint64_t ext = cells_extent(units, n);
    const std::vector<int> rb = level_runs(c, units, n);
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
        (rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) ||
        (rc = ensure(c, c->h_bound, sizeof(uint32_t) * n)))  // the units' keys
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
        if ((rc2 = wc_forward_levels_budget(c, c->h_cells.p, dtype, units + a, m, levels + a, max_pairs + a, pay,
                                            run_bound, doff, dkept, (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a,
                                            (uint32_t*)c->h_bound.p + a)))
            return rc2;
        // pack the slots densely (offsets stay == 4 mod 8), as wc_forward_host does
        e = launch_pack(c->stream, (const UnitDev*)c->plan.d_units.p, m, dkept, pay, dpoff, (uint8_t*)c->h_packed.p);
        if (e != hipSuccess) return hip_fail(c, e, "pack launch");
        // the round trip: the run's payloads back to cells, compared with the cells on the device
        if (rmse && ((rc2 = wc_inverse_levels(c, pay, doff, units + a, m, levels + a, (float*)c->h_out.p)) ||
                     (rc2 = wc_rmse(c, c->h_cells.p, dtype, (const float*)c->h_out.p, units + a, m,
                                    (double*)c->h_rmse.p + a)))) {
            (void)hipStreamSynchronize(c->stream);
            return rc2;
        }
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
        if (thresh)
            e = hipMemcpyAsync(thresh, c->h_thresh.p, sizeof(float) * WC_MAX_LEVELS * n, hipMemcpyDeviceToHost,
                               c->stream);
        if (e == hipSuccess && key)
            e = hipMemcpyAsync(key, c->h_bound.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && rmse)
            e = hipMemcpyAsync(rmse, c->h_rmse.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
    }
    // no copy that reads or writes the caller's buffers may outlive the call
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc != WC_OK) return rc;
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "results readback");
    return check_kernel_errors(c);
}
