// wc_layershost.cpp — host side of the progressive layers (include/wavelet_amd.h):
// wc_split_budget_host, wc_split_thresh_host and wc_merge_host.  (The rule on one
// unit, wc_split_unit / wc_merge_unit, and the bounds are in wc_layersrule.cpp,
// plain C++; the device entry points are in wc_capi.cpp.)
//
// Each is its checks and a call of payload_serial (wc_hostserial.cpp) with the
// packed-run tail, as wc_thinhost.cpp: per run the payload bytes up, the device call
// into wc_forward's slot layout, the slots packed densely, download.  The split
// hands the driver a second packed output (the rest), the merge a second input
// (b): SerialOut's second stream.  A unit whose header disagrees (for the merge:
// either header, or the two with each other) fails the call before anything runs.
#include "wc_ctx.h"

#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace {

// unit i's header at p against the unit and, when given, its level count: its L and the end of its bytes
int open_header(wc_ctx* c, const uint8_t* p, uint64_t off, const wc_unit& f, int i, const int32_t* levels, int32_t& L,
                uint64_t& end) {
    if (off & 3) return fail(c, WC_ERR_INVALID, "offsets must be multiples of 4");
    int32_t h[5];
    std::memcpy(h, p + off, sizeof h);
    int l = 0;
    if (wc_payload_levels(p + off, 20, &l) != WC_OK || h[0] != f.nx || h[1] != f.ny || h[2] != f.nz || h[4] < 0 ||
        (levels && levels[i] != l))
        return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": the payload header disagrees with the unit");
    L = l;
    end = off + 20 + 8ull * (uint64_t)h[4];
    return WC_OK;
}

int split_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
               const int32_t* levels, const uint32_t* max_pairs, const float* thresh, uint8_t* base, uint64_t base_cap,
               uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_cap, uint64_t* rest_offsets,
               uint32_t* rest_pairs, float* thresh_out, uint32_t* key) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !base || !base_offsets || !kept || !rest || !rest_offsets || !rest_pairs ||
        (!max_pairs && !thresh))
        return fail(c, WC_ERR_INVALID, "null buffer");
    std::vector<uint64_t> end(n);
    std::vector<int32_t> lv(n);
    for (int i = 0; i < n; ++i)
        if ((rc = open_header(c, payload, offsets[i], units[i], i, levels, lv[i], end[i]))) return rc;
    if ((rc = validate_levels(c, units, n, lv.data()))) return rc;
    if (thresh)
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < lv[i]; ++l)
                if (!(thresh[(size_t)i * WC_MAX_LEVELS + l] >= 0.0f))
                    return fail(c, WC_ERR_INVALID, "unit " + std::to_string(i) + ": a threshold is NaN or negative");
    uint64_t bb = 0, rb = 0;
    (void)wc_split_bound(units, n, max_pairs, &bb, &rb);
    if (base_cap < bb || rest_cap < rb) return fail(c, WC_ERR_INVALID, "capacity < wc_split_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->pk_off, sizeof(uint64_t) * ((size_t)n + 1))) ||
        (rc = ensure(c, c->h_thresh, sizeof(float) * WC_MAX_LEVELS * n)) || (rc = ensure(c, c->h_bound, sizeof(uint32_t) * n)))
        return rc;
    SerialOut o;
    o.shift = 16;
    o.slack = 32;
    o.payload = base;
    o.cap = base_cap;
    o.out_offsets = base_offsets;
    o.kept = kept;
    o.payload2 = rest;
    o.cap2 = rest_cap;
    o.out_offsets2 = rest_offsets;
    o.kept2 = rest_pairs;
    if (max_pairs)
        o.results = {{c->h_thresh.p, thresh_out, sizeof(float) * WC_MAX_LEVELS}, {c->h_bound.p, key, sizeof(uint32_t)}};
    return payload_serial(
        c, payload, offsets, end.data(), units, n,
        [&](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets, uint64_t) {
            const uint64_t bound = wc_payload_bound(units + a, m);
            return split_device(c, d_payload, d_offsets, units + a, m, lv.data() + a, max_pairs ? max_pairs + a : nullptr,
                                thresh ? thresh + (size_t)WC_MAX_LEVELS * a : nullptr, true, (uint8_t*)c->h_out.p, bound,
                                (uint64_t*)c->pk_off.p, (uint32_t*)c->h_kept.p,
                                SplitOut{(uint8_t*)c->h_second.p, bound, (uint64_t*)c->h_second_off.p,
                                         (uint32_t*)c->h_second_cnt.p},
                                max_pairs ? (float*)c->h_thresh.p + (size_t)WC_MAX_LEVELS * a : nullptr,
                                max_pairs ? (uint32_t*)c->h_bound.p + a : nullptr);
        },
        o);
}

}  // namespace

extern "C" {

int wc_split_budget_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const uint32_t* max_pairs, uint8_t* base, uint64_t base_capacity,
                         uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                         uint64_t* rest_offsets, uint32_t* rest_pairs, float* thresh, uint32_t* key) {
    if (c && n > 0 && !max_pairs) return fail(c, WC_ERR_INVALID, "null buffer");
    return split_host(c, payload, offsets, units, n, levels, max_pairs, nullptr, base, base_capacity, base_offsets, kept,
                      rest, rest_capacity, rest_offsets, rest_pairs, thresh, key);
}

int wc_split_thresh_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const float* thresh, uint8_t* base, uint64_t base_capacity,
                         uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                         uint64_t* rest_offsets, uint32_t* rest_pairs) {
    if (c && n > 0 && !thresh) return fail(c, WC_ERR_INVALID, "null buffer");
    return split_host(c, payload, offsets, units, n, levels, nullptr, thresh, base, base_capacity, base_offsets, kept,
                      rest, rest_capacity, rest_offsets, rest_pairs, nullptr, nullptr);
}

int wc_merge_host(wc_ctx* c, const uint8_t* a, const uint64_t* a_offsets, const uint8_t* b, const uint64_t* b_offsets,
                  const wc_unit* units, int n, const int32_t* levels, uint8_t* out, uint64_t out_capacity,
                  uint64_t* out_offsets, uint32_t* pairs) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!a || !a_offsets || !b || !b_offsets || !out || !out_offsets || !pairs) return fail(c, WC_ERR_INVALID, "null buffer");
    std::vector<uint64_t> ea(n), eb(n);
    std::vector<int32_t> lv(n);
    for (int i = 0; i < n; ++i) {
        int32_t lb = 0;
        if ((rc = open_header(c, a, a_offsets[i], units[i], i, levels, lv[i], ea[i])) ||
            (rc = open_header(c, b, b_offsets[i], units[i], i, levels, lb, eb[i])))
            return rc;
        if (lb != lv[i])
            return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": the headers of a and b disagree");
    }
    if ((rc = validate_levels(c, units, n, lv.data()))) return rc;
    if (out_capacity < wc_merge_bound(units, n)) return fail(c, WC_ERR_INVALID, "out_capacity < wc_merge_bound");
    if ((rc = set_device(c))) return rc;
    if ((rc = ensure(c, c->pk_off, sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
    SerialOut o;
    o.shift = 16;
    o.slack = 32;
    o.payload = out;
    o.cap = out_capacity;
    o.out_offsets = out_offsets;
    o.kept = pairs;
    o.bytes2 = b;
    o.offsets2 = b_offsets;
    o.end2 = eb.data();
    return payload_serial(
        c, a, a_offsets, ea.data(), units, n,
        [&](int r0, int m, const uint8_t* d_a, const uint64_t* d_a_offsets, uint64_t) {
            return merge_device(c, d_a, d_a_offsets, (const uint8_t*)c->h_second.p, (const uint64_t*)c->h_second_off.p,
                                units + r0, m, lv.data() + r0, (uint8_t*)c->h_out.p, wc_payload_bound(units + r0, m),
                                (uint64_t*)c->pk_off.p, (uint32_t*)c->h_kept.p);
        },
        o);
}

}  // extern "C"
