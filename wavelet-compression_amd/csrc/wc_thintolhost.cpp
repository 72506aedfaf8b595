// wc_thintolhost.cpp — host side of the tolerance forms of the compressed-domain
// thinning and split (include/wavelet_amd.h): wc_thin_tol_host and
// wc_split_tol_host.  (The rule on one payload, wc_thin_tol_unit /
// wc_split_tol_unit, is in wc_thintolrule.cpp, plain C++; the device entry points
// are in wc_capi.cpp.)
//
// Both are their checks and a call of payload_serial (wc_hostserial.cpp) with the
// packed-run tail, exactly as wc_thinhost.cpp and wc_layershost.cpp: per run the
// payload bytes up, the device call into wc_forward's slot layout, the slots
// packed densely, download; the thresholds and bounds come back at the call's end.
// A unit whose header disagrees fails the call before anything runs.
#include "wc_ctx.h"

#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace {

// the thinning, or (split) the split with the rest's outputs
int tol_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
             const int32_t* levels, const double* tol, uint8_t* out, uint64_t cap, uint64_t* out_offsets, uint32_t* kept,
             bool split, uint8_t* rest, uint64_t rest_cap, uint64_t* rest_offsets, uint32_t* rest_pairs, float* thresh,
             double* bound) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !tol || !out || !out_offsets || !kept || (split && (!rest || !rest_offsets || !rest_pairs)))
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
    if ((rc = validate_levels(c, units, n, lv.data())) || (rc = validate_tol(c, units, n, tol))) return rc;
    uint64_t bb = 0, rb = 0;
    (void)wc_split_bound(units, n, nullptr, &bb, &rb);
    if (cap < bb) return fail(c, WC_ERR_INVALID, split ? "capacity < wc_split_bound" : "out_capacity < wc_thin_bound");
    if (split && rest_cap < rb) return fail(c, WC_ERR_INVALID, "capacity < wc_split_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->pk_off, sizeof(uint64_t) * ((size_t)n + 1))) ||
        (rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) || (rc = ensure(c, c->h_bound, sizeof(double) * n)))
        return rc;
    SerialOut o;
    o.shift = 16;
    o.slack = 32;
    o.payload = out;
    o.cap = cap;
    o.out_offsets = out_offsets;
    o.kept = kept;
    if (split) {
        o.payload2 = rest;
        o.cap2 = rest_cap;
        o.out_offsets2 = rest_offsets;
        o.kept2 = rest_pairs;
    }
    o.results = {{c->h_thresh.p, thresh, sizeof(float) * WC_MAX_LEVELS}, {c->h_bound.p, bound, sizeof(double)}};
    return payload_serial(
        c, payload, offsets, end.data(), units, n,
        [&](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets, uint64_t) {
            const uint64_t run_bound = wc_payload_bound(units + a, m);
            float* d_thresh = (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a;
            double* d_bound = (double*)c->h_bound.p + a;
            if (!split)
                return thin_tol_device(c, d_payload, d_offsets, units + a, m, lv.data() + a, tol + a, (uint8_t*)c->h_out.p,
                                       run_bound, (uint64_t*)c->pk_off.p, (uint32_t*)c->h_kept.p, d_thresh, d_bound);
            return split_tol_device(c, d_payload, d_offsets, units + a, m, lv.data() + a, tol + a, (uint8_t*)c->h_out.p,
                                    run_bound, (uint64_t*)c->pk_off.p, (uint32_t*)c->h_kept.p,
                                    SplitOut{(uint8_t*)c->h_second.p, run_bound, (uint64_t*)c->h_second_off.p,
                                             (uint32_t*)c->h_second_cnt.p},
                                    d_thresh, d_bound);
        },
        o);
}

}  // namespace

extern "C" {

int wc_thin_tol_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                     const int32_t* levels, const double* tol, uint8_t* out, uint64_t out_capacity,
                     uint64_t* out_offsets, uint32_t* kept, float* thresh, double* bound) {
    return tol_host(c, payload, offsets, units, n, levels, tol, out, out_capacity, out_offsets, kept, false, nullptr, 0,
                    nullptr, nullptr, thresh, bound);
}

int wc_split_tol_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                      const int32_t* levels, const double* tol, uint8_t* base, uint64_t base_capacity,
                      uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                      uint64_t* rest_offsets, uint32_t* rest_pairs, float* thresh, double* bound) {
    return tol_host(c, payload, offsets, units, n, levels, tol, base, base_capacity, base_offsets, kept, true, rest,
                    rest_capacity, rest_offsets, rest_pairs, thresh, bound);
}

}  // extern "C"
