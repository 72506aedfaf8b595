// wc_levelshost.cpp — host side of the opt-in multi-level mode
// (include/wavelet_amd.h): the level a box admits (wc_levels_for), the level a
// payload header carries (wc_payload_levels), the argument checks of the mode,
// and the _levels_host entry points.
//
// The host entry points run their unit runs (WC_OPT_HOST_CHUNK) one after
// another on the context's stream, as wc_forward_tol_host does: they are not
// pipelined over the copy streams (wc_hostpipe.cpp).
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

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

// contiguous unit runs of at least opt_host_chunk cells (0: one run)
std::vector<int> level_runs(const wc_ctx* c, const wc_unit* units, int n) {
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
    return rb;
}

}  // namespace wc

namespace {

// the span of cells the units [a, a + m) own
void cell_span(const wc_unit* units, int a, int m, uint64_t& lo, uint64_t& hi) {
    lo = UINT64_MAX;
    hi = 0;
    for (int i = a; i < a + m; ++i) {
        const uint64_t cnt = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        if (!cnt) continue;
        lo = std::min(lo, units[i].cell_offset);
        hi = std::max(hi, units[i].cell_offset + cnt);
    }
}

}  // namespace

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

int wc_forward_levels_host(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n,
                           const int32_t* levels, double keep, const float* thresh, uint8_t* payload, uint64_t cap,
                           uint64_t* offsets, uint32_t* kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!cells || !payload || !offsets || !kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_levels(c, units, n, levels))) return rc;
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
        (rc = ensure(c, c->h_poff, sizeof(uint64_t) * (run_units + 1))) || (rc = ensure(c, c->h_kept, 4ull * run_units)))
        return rc;

    std::vector<uint64_t> po(run_units + 1);
    uint64_t R = 4;  // run r's packed bytes [4, end) land at R (== 4 mod 8)
    auto run = [&](int r) -> int {
        const int a = rb[r], m = rb[r + 1] - rb[r];
        uint64_t lo, hi;
        cell_span(units, a, m, lo, hi);
        hipError_t e;
        if (hi > lo && (e = hipMemcpyAsync((uint8_t*)c->h_cells.p + esz * lo, (const uint8_t*)cells + esz * lo,
                                           esz * (hi - lo), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return hip_fail(c, e, "cells upload");
        uint8_t* pay = (uint8_t*)c->h_payload.p;
        uint64_t* doff = (uint64_t*)c->h_offsets.p;
        uint64_t* dpoff = (uint64_t*)c->h_poff.p;
        uint32_t* dkept = (uint32_t*)c->h_kept.p;
        int rc2;
        if ((rc2 = wc_forward_levels(c, c->h_cells.p, dtype, units + a, m, levels + a, keep, thresh, pay, run_bound,
                                     doff, dkept)))
            return rc2;
        // pack the slots densely (offsets stay == 4 mod 8), as wc_forward_host does
        e = launch_pack(c->stream, (const UnitDev*)c->plan.d_units.p, m, dkept, pay, dpoff, (uint8_t*)c->h_packed.p);
        if (e != hipSuccess) return hip_fail(c, e, "pack launch");
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
    if (rc == WC_OK) offsets[n] = R - 4;
    // no copy that reads or writes the caller's buffers may outlive the call
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc != WC_OK) return rc;
    if (es != hipSuccess) return hip_fail(c, es, "results readback");
    return check_kernel_errors(c);
}

int wc_inverse_levels_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    // unit u's bytes: its header and the nrle pairs the header announces (wc_inverse_host
    // sizes its copies the same way; offsets has n entries, in any order)
    std::vector<uint64_t> end(n);
    std::vector<int32_t> from_headers;
    if (!levels) from_headers.resize(n);
    for (int i = 0; i < n; ++i) {
        if (offsets[i] & 3) return fail(c, WC_ERR_INVALID, "offsets must be multiples of 4");
        int32_t nrle;
        std::memcpy(&nrle, payload + offsets[i] + 16, 4);
        end[i] = offsets[i] + 20 + 8ull * (uint64_t)std::max(nrle, 0);
        if (!levels) {  // each unit's L from its header
            int L = 0;
            if (wc_payload_levels(payload + offsets[i], 20, &L) != WC_OK)
                return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": malformed payload header");
            from_headers[i] = L;
        }
    }
    if (!levels) levels = from_headers.data();
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if ((rc = set_device(c))) return rc;
    const uint64_t ext = cells_extent(units, n);
    const std::vector<int> rb = level_runs(c, units, n);
    const int nr = (int)rb.size() - 1;
    // a run's payload bytes [lo, hi) upload to the same distance from an 8-B
    // boundary (pairs stay 8-B aligned); its offsets are rebased to that copy
    auto span = [&](int r, uint64_t& lo, uint64_t& hi) {
        lo = UINT64_MAX;
        hi = 0;
        for (int i = rb[r]; i < rb[r + 1]; ++i) {
            lo = std::min(lo, offsets[i]);
            hi = std::max(hi, end[i]);
        }
    };
    uint64_t run_bytes = 0;
    int run_units = 0;
    for (int r = 0; r < nr; ++r) {
        uint64_t lo, hi;
        span(r, lo, hi);
        run_bytes = std::max(run_bytes, hi - lo);
        run_units = std::max(run_units, rb[r + 1] - rb[r]);
    }
    if ((rc = ensure(c, c->h_payload, run_bytes + 16)) || (rc = ensure(c, c->h_out, sizeof(float) * ext)) ||
        (rc = ensure(c, c->h_offsets, sizeof(uint64_t) * run_units)))
        return rc;
    std::vector<uint64_t> ro(run_units);
    for (int r = 0; r < nr; ++r) {
        const int a = rb[r], m = rb[r + 1] - rb[r];
        uint64_t p0, p1;
        span(r, p0, p1);
        const uint64_t shift = p0 & 7;
        for (int i = 0; i < m; ++i) ro[i] = offsets[a + i] - p0 + shift;
        hipError_t e;
        if ((e = hipMemcpyAsync((uint8_t*)c->h_payload.p + shift, payload + p0, p1 - p0, hipMemcpyHostToDevice,
                                c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(c->h_offsets.p, ro.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice, c->stream)) !=
                hipSuccess)
            return hip_fail(c, e, "payload upload");
        if ((rc = wc_inverse_levels(c, (const uint8_t*)c->h_payload.p, (const uint64_t*)c->h_offsets.p, units + a, m,
                                    levels + a, (float*)c->h_out.p))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        // the units' boxes, back-to-back ones in one copy (cells no unit owns stay as they were)
        e = hipSuccess;
        for (int i = a; i < a + m && e == hipSuccess;) {
            uint64_t lo = units[i].cell_offset, hi = lo + (uint64_t)units[i].nx * units[i].ny * units[i].nz;
            for (++i; i < a + m && units[i].cell_offset == hi; ++i)
                hi += (uint64_t)units[i].nx * units[i].ny * units[i].nz;
            if (hi > lo)
                e = hipMemcpyAsync(out + lo, (const float*)c->h_out.p + lo, sizeof(float) * (hi - lo),
                                   hipMemcpyDeviceToHost, c->stream);
        }
        // ro is rewritten by the next run: the uploads have finished after this synchronize
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "box readback");
    }
    return check_kernel_errors(c);
}

}  // extern "C"
