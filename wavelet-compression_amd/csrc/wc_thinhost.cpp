// wc_thinhost.cpp — host side of the compressed-domain thinning
// (include/wavelet_amd.h): wc_thin_budget_host and wc_thin_thresh_host.  (The
// rule on one payload, wc_thin_unit, is in wc_thinrule.cpp, plain C++; the device
// entry points are in wc_capi.cpp.)
//
// thin_host is the checks of both forms and a call of payload_serial
// (wc_hostserial.cpp) with the packed-run tail: per run the payload bytes up, the
// device call into wc_forward's slot layout, the slots packed densely
// (wc_compact.hip, as wc_forward_host does), download.  Only payload bytes cross
// the bus.  A unit whose header disagrees fails the call before anything runs.
#include "wc_ctx.h"

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
    // thin_device's own outputs: the slot offsets of a run, the thresholds and keys of the budget form
    if ((rc = ensure(c, c->pk_off, sizeof(uint64_t) * ((size_t)n + 1))) ||
        (rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) || (rc = ensure(c, c->h_bound, sizeof(uint32_t) * n)))
        return rc;
    SerialOut o;
    o.shift = 16;
    o.slack = 32;
    o.payload = out;
    o.cap = cap;
    o.out_offsets = out_offsets;
    o.kept = kept;
    if (max_pairs)
        o.results = {{c->h_thresh.p, thresh_out, sizeof(float) * WC_MAX_LEVELS}, {c->h_bound.p, key, sizeof(uint32_t)}};
    return payload_serial(
        c, payload, offsets, end.data(), units, n,
        [&](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets, uint64_t) {
            return thin_device(c, d_payload, d_offsets, units + a, m, lv.data() + a, max_pairs ? max_pairs + a : nullptr,
                               thresh ? thresh + (size_t)WC_MAX_LEVELS * a : nullptr, true, (uint8_t*)c->h_out.p,
                               wc_payload_bound(units + a, m), (uint64_t*)c->pk_off.p, (uint32_t*)c->h_kept.p,
                               max_pairs ? (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a : nullptr,
                               max_pairs ? (uint32_t*)c->h_bound.p + a : nullptr);
        },
        o);
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
