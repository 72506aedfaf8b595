// wc_regionhost.cpp — host side of the sub-box inverse (include/wavelet_amd.h
// wc_inverse_region): the mode's argument checks, wc_inverse_region_host and
// the driver it shares with wc_inverse_coarse_host.  (wc_region_align and
// wc_region_units are in wc_regionrule.cpp, plain C++.)
//
// The driver runs its unit runs (WC_OPT_HOST_CHUNK, by the cells of the
// full-size units) one after another on the context's stream, as
// wc_inverse_levels_host does; only the derived units' cells cross back.
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace wc {

// The mode's preconditions beyond validate_levels, before anything is launched:
// a reduce per unit in 0..levels[u]; on a unit with cells 2^L dividing every
// dimension and every origin and extent of a region inside the box; an all-zero
// region on a unit without cells; out_units[u] carrying exactly the extents >> r.
int validate_region(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                    const wc_region* regions, const wc_unit* out_units) {
    for (int i = 0; i < n; ++i) {
        const int r = reduce ? reduce[i] : 0, L = levels[i];
        const wc_unit& u = units[i];
        const wc_region& g = regions[i];
        // the messages' parts, put together only for a refusal (the checks run on every call)
        auto who = [&] { return "unit " + std::to_string(i); };
        auto gs = [&] {
            return "region (" + std::to_string(g.x0) + ", " + std::to_string(g.y0) + ", " + std::to_string(g.z0) +
                   ") + " + std::to_string(g.nx) + "x" + std::to_string(g.ny) + "x" + std::to_string(g.nz);
        };
        auto us = [&] { return std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" + std::to_string(u.nz); };
        if (r < 0 || r > L)
            return fail(c, WC_ERR_INVALID, who() + ": reduce " + std::to_string(r) + " outside 0.." + std::to_string(L));
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        const int32_t m = (1 << L) - 1;
        if (!cells) {
            if (g.x0 | g.y0 | g.z0 | g.nx | g.ny | g.nz)
                return fail(c, WC_ERR_INVALID,
                            who() + " (" + us() + "): a unit without cells needs an all-zero region, not " + gs());
        } else {
            if ((u.nx | u.ny | u.nz) & m)
                return fail(c, WC_ERR_INVALID,
                            who() + " (" + us() + "): a region decode of " + std::to_string(L) +
                                " level(s) needs W, H and D divisible by " + std::to_string(1 << L));
            if (g.x0 < 0 || g.y0 < 0 || g.z0 < 0 || g.nx < 0 || g.ny < 0 || g.nz < 0 ||
                (int64_t)g.x0 + g.nx > u.nx || (int64_t)g.y0 + g.ny > u.ny || (int64_t)g.z0 + g.nz > u.nz)
                return fail(c, WC_ERR_INVALID, who() + " (" + us() + "): " + gs() + " is not inside the box");
            if ((g.x0 | g.y0 | g.z0 | g.nx | g.ny | g.nz) & m)
                return fail(c, WC_ERR_INVALID,
                            who() + ": " + gs() + " is not aligned to " + std::to_string(1 << L) + " (wc_region_align)");
        }
        const wc_unit& o = out_units[i];
        if (o.nx != g.nx >> r || o.ny != g.ny >> r || o.nz != g.nz >> r || o.reserved != 0)
            return fail(c, WC_ERR_INVALID,
                        who() + ": out_units must carry " + std::to_string(g.nx >> r) + "x" + std::to_string(g.ny >> r) +
                            "x" + std::to_string(g.nz >> r) + " and reserved = 0 (wc_region_units)");
    }
    return WC_OK;
}

// wc_inverse_coarse_host (regions NULL) and wc_inverse_region_host after their
// null checks: the levels (from the headers where the caller passes none), the
// mode's checks, then run by run the upload, the device call and the readback.
int inverse_compact_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                         const wc_unit* out_units, float* out) {
    int rc;
    // unit u's bytes: its header and the nrle pairs the header announces, as wc_inverse_levels_host
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
    if ((rc = validate_levels(c, units, n, levels)) ||
        (rc = regions ? validate_region(c, units, n, levels, reduce, regions, out_units)
                      : validate_coarse(c, units, n, levels, reduce, out_units)))
        return rc;
    if (!regions && std::all_of(reduce, reduce + n, [](int32_t r) { return r == 0; }))
        return wc_inverse_levels_host(c, payload, offsets, out_units, n, levels, out);
    if ((rc = set_device(c))) return rc;
    const uint64_t ext = cells_extent(out_units, n);
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
    if ((rc = ensure(c, c->h_payload, run_bytes + 16)) || (rc = ensure(c, c->h_out, sizeof(float) * ext + 16)) ||
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
        const uint8_t* d_payload = (const uint8_t*)c->h_payload.p;
        const uint64_t* d_offsets = (const uint64_t*)c->h_offsets.p;
        float* d_out = (float*)c->h_out.p;
        rc = regions ? wc_inverse_region(c, d_payload, d_offsets, units + a, m, levels + a,
                                         reduce ? reduce + a : nullptr, regions + a, out_units + a, d_out)
                     : wc_inverse_coarse(c, d_payload, d_offsets, units + a, m, levels + a, reduce + a, out_units + a,
                                         d_out);
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        // the units' boxes, back-to-back ones in one copy (cells no unit owns stay as they were)
        e = hipSuccess;
        for (int i = a; i < a + m && e == hipSuccess;) {
            uint64_t lo = out_units[i].cell_offset,
                     hi = lo + (uint64_t)out_units[i].nx * out_units[i].ny * out_units[i].nz;
            for (++i; i < a + m && out_units[i].cell_offset == hi; ++i)
                hi += (uint64_t)out_units[i].nx * out_units[i].ny * out_units[i].nz;
            if (hi > lo)
                e = hipMemcpyAsync(out + lo, (const float*)d_out + lo, sizeof(float) * (hi - lo),
                                   hipMemcpyDeviceToHost, c->stream);
        }
        // ro is rewritten by the next run: the uploads have finished after this synchronize
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "box readback");
    }
    return check_kernel_errors(c);
}

}  // namespace wc

extern "C" {

int wc_inverse_region_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                           const wc_unit* out_units, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !regions || !out_units || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    return inverse_compact_host(c, payload, offsets, units, n, levels, reduce, regions, out_units, out);
}

}  // extern "C"
