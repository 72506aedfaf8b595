// wc_regionhost.cpp — host side of the sub-box inverse (include/wavelet_amd.h
// wc_inverse_region): the mode's argument checks, wc_inverse_region_host and
// inverse_compact_host, which it shares with wc_inverse_coarse_host.
// (wc_region_align and wc_region_units are in wc_regionrule.cpp, plain C++.)
//
// inverse_compact_host is the two modes' checks and a call of payload_serial
// (wc_hostserial.cpp): runs by the cells of the full-size units, only the
// derived units' cells cross back.
#include "wc_ctx.h"

#include <algorithm>
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
// mode's checks, then payload_serial with the mode's device call.
int inverse_compact_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                         const wc_unit* out_units, float* out) {
    int rc;
    std::vector<uint64_t> end;
    std::vector<int32_t> from_headers;
    if ((rc = payload_ends(c, payload, offsets, n, end, levels ? nullptr : &from_headers))) return rc;
    if (!levels) levels = from_headers.data();
    if ((rc = validate_levels(c, units, n, levels)) ||
        (rc = regions ? validate_region(c, units, n, levels, reduce, regions, out_units)
                      : validate_coarse(c, units, n, levels, reduce, out_units)))
        return rc;
    if (!regions && std::all_of(reduce, reduce + n, [](int32_t r) { return r == 0; }))
        return wc_inverse_levels_host(c, payload, offsets, out_units, n, levels, out);
    if ((rc = set_device(c))) return rc;
    SerialOut o;
    o.out_units = out_units;
    o.out = out;
    o.out_bytes = sizeof(float) * cells_extent(out_units, n) + 16;
    return payload_serial(
        c, payload, offsets, end.data(), units, n,
        [&](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets, uint64_t) {
            float* d_out = (float*)c->h_out.p;
            return regions ? wc_inverse_region(c, d_payload, d_offsets, units + a, m, levels + a,
                                               reduce ? reduce + a : nullptr, regions + a, out_units + a, d_out)
                           : wc_inverse_coarse(c, d_payload, d_offsets, units + a, m, levels + a, reduce + a,
                                               out_units + a, d_out);
        },
        o);
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
