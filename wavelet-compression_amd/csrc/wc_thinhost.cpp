// wc_thinhost.cpp — host side of the compressed-domain thinning
// (include/wavelet_amd.h): wc_thin_budget_host and wc_thin_thresh_host.  (The
// rule on one payload, wc_thin_unit, is in wc_thinrule.cpp, plain C++; the device
// entry points are in wc_capi.cpp.)
//
// As wc_inverse_region_host, the unit runs (WC_OPT_HOST_CHUNK, by the cells of the
// units) go one after another on the context's stream: upload the run's payload
// bytes, the device call into wc_forward's slot layout, pack the slots densely
// (wc_compact.hip, as wc_forward_host does), download.  Only payload bytes cross
// the bus.  A unit whose header disagrees fails the call before anything runs.
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace {

int thin_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
              const int32_t* levels, const uint32_t* max_pairs, const float* thresh, uint8_t* out, uint64_t cap,
              uint64_t* out_offsets, uint32_t* kept, float* thresh_out, uint32_t* key) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !out || !out_offsets || !kept || (!max_pairs && !thresh))
        return fail(c, WC_ERR_INVALID, "null buffer");
    // unit u's bytes: its header and the nrle pairs the header announces; its L from the header
    std::vector<uint64_t> end(n);
    std::vector<int32_t> lv(n);
    for (int i = 0; i < n; ++i) {
        if (offsets[i] & 3) return fail(c, WC_ERR_INVALID, "offsets must be multiples of 4");
        int32_t h[5];
        std::memcpy(h, payload + offsets[i], sizeof h);
        int L = 0;
        if (wc_payload_levels(payload + offsets[i], 20, &L) != WC_OK || h[0] != units[i].nx || h[1] != units[i].ny ||
            h[2] != units[i].nz || h[4] < 0 || (levels && levels[i] != L))
            return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": the payload header disagrees with the unit");
        lv[i] = L;
        end[i] = offsets[i] + 20 + 8ull * (uint64_t)h[4];
    }
    if ((rc = validate_levels(c, units, n, lv.data()))) return rc;
    if (thresh)
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < lv[i]; ++l)
                if (!(thresh[(size_t)i * WC_MAX_LEVELS + l] >= 0.0f))
                    return fail(c, WC_ERR_INVALID, "unit " + std::to_string(i) + ": a threshold is NaN or negative");
    if (cap < wc_thin_bound(units, n, max_pairs)) return fail(c, WC_ERR_INVALID, "out_capacity < wc_thin_bound");
    if ((rc = set_device(c))) return rc;
    const std::vector<int> rb = level_runs(c, units, n);
    const int nr = (int)rb.size() - 1;
    auto span = [&](int r, uint64_t& lo, uint64_t& hi) {
        lo = UINT64_MAX;
        hi = 0;
        for (int i = rb[r]; i < rb[r + 1]; ++i) {
            lo = std::min(lo, offsets[i]);
            hi = std::max(hi, end[i]);
        }
    };
    uint64_t run_bytes = 0, run_bound = 0;
    int run_units = 0;
    for (int r = 0; r < nr; ++r) {
        uint64_t lo, hi;
        span(r, lo, hi);
        run_bytes = std::max(run_bytes, hi - lo);
        run_bound = std::max(run_bound, wc_payload_bound(units + rb[r], rb[r + 1] - rb[r]));
        run_units = std::max(run_units, rb[r + 1] - rb[r]);
    }
    if ((rc = ensure(c, c->h_payload, run_bytes + 32)) || (rc = ensure(c, c->h_out, run_bound)) ||
        (rc = ensure(c, c->h_packed, run_bound)) || (rc = ensure(c, c->h_offsets, sizeof(uint64_t) * (run_units + 1))) ||
        (rc = ensure(c, c->pk_off, sizeof(uint64_t) * (run_units + 1))) ||
        (rc = ensure(c, c->h_poff, sizeof(uint64_t) * (run_units + 1))) || (rc = ensure(c, c->h_kept, 4ull * run_units)) ||
        (rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) || (rc = ensure(c, c->h_bound, sizeof(uint32_t) * n)))
        return rc;
    std::vector<uint64_t> ro(run_units), po(run_units + 1);
    uint64_t R = 4;  // run r's packed bytes [4, end) land at R (== 4 mod 8)
    for (int r = 0; r < nr; ++r) {
        const int a = rb[r], m = rb[r + 1] - rb[r];
        uint64_t p0, p1;
        span(r, p0, p1);
        const uint64_t shift = 16 + (p0 & 7);  // the copy keeps the bytes' distance from an 8-B boundary
        for (int i = 0; i < m; ++i) ro[i] = offsets[a + i] - p0 + shift;
        hipError_t e;
        if ((e = hipMemcpyAsync((uint8_t*)c->h_payload.p + shift, payload + p0, p1 - p0, hipMemcpyHostToDevice,
                                c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(c->h_offsets.p, ro.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice, c->stream)) !=
                hipSuccess)
            return hip_fail(c, e, "payload upload");
        uint32_t* dkept = (uint32_t*)c->h_kept.p;
        uint64_t* dpoff = (uint64_t*)c->h_poff.p;
        rc = thin_device(c, (const uint8_t*)c->h_payload.p, (const uint64_t*)c->h_offsets.p, units + a, m, lv.data() + a,
                         max_pairs ? max_pairs + a : nullptr, thresh ? thresh + (size_t)WC_MAX_LEVELS * a : nullptr, true,
                         (uint8_t*)c->h_out.p, run_bound, (uint64_t*)c->pk_off.p, dkept,
                         max_pairs ? (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a : nullptr,
                         max_pairs ? (uint32_t*)c->h_bound.p + a : nullptr);
        if (rc == WC_OK) {
            // the plan thin_device left is the run's units': its slots are wc_forward's
            e = launch_pack(c->stream, (const UnitDev*)c->plan.d_units.p, m, dkept, (const uint8_t*)c->h_out.p, dpoff,
                            (uint8_t*)c->h_packed.p);
            if (e != hipSuccess) rc = hip_fail(c, e, "pack launch");
        }
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        if ((e = hipMemcpyAsync(po.data(), dpoff, sizeof(uint64_t) * (m + 1), hipMemcpyDeviceToHost, c->stream)) !=
                hipSuccess ||
            (e = hipMemcpyAsync(kept + a, dkept, 4ull * m, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(c->stream)) != hipSuccess)
            return hip_fail(c, e, "sizes readback");
        if (R - 4 + po[m] > cap) return fail(c, WC_ERR_INVALID, "out_capacity");
        for (int i = 0; i < m; ++i) out_offsets[a + i] = R - 4 + po[i];
        const uint64_t bytes = po[m] - 4;
        if (bytes && (e = hipMemcpyAsync(out + R, (const uint8_t*)c->h_packed.p + 4, bytes, hipMemcpyDeviceToHost,
                                         c->stream)) != hipSuccess)
            return hip_fail(c, e, "payload readback");
        // ro and the staging are rewritten by the next run
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(c, e, "payload readback");
        R += po[m];
    }
    out_offsets[n] = R - 4;
    hipError_t e = hipSuccess;
    if (max_pairs && thresh_out)
        e = hipMemcpyAsync(thresh_out, c->h_thresh.p, sizeof(float) * WC_MAX_LEVELS * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && max_pairs && key)
        e = hipMemcpyAsync(key, c->h_bound.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "results readback");
    return check_kernel_errors(c);
}

}  // namespace

extern "C" {

int wc_thin_budget_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                        const int32_t* levels, const uint32_t* max_pairs, uint8_t* out, uint64_t out_capacity,
                        uint64_t* out_offsets, uint32_t* kept, float* thresh, uint32_t* key) {
    if (c && n > 0 && !max_pairs) return fail(c, WC_ERR_INVALID, "null buffer");
    return thin_host(c, payload, offsets, units, n, levels, max_pairs, nullptr, out, out_capacity, out_offsets, kept,
                     thresh, key);
}

int wc_thin_thresh_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                        const int32_t* levels, const float* thresh, uint8_t* out, uint64_t out_capacity,
                        uint64_t* out_offsets, uint32_t* kept) {
    if (c && n > 0 && !thresh) return fail(c, WC_ERR_INVALID, "null buffer");
    return thin_host(c, payload, offsets, units, n, levels, nullptr, thresh, out, out_capacity, out_offsets, kept,
                     nullptr, nullptr);
}

}  // extern "C"
