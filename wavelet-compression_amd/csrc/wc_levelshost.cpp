// wc_levelshost.cpp — the _levels_host entry points of the opt-in multi-level
// mode (include/wavelet_amd.h).  (wc_levels_for, wc_payload_levels and the
// argument checks of the mode are in wc_levelsrule.cpp, which calls no device
// entry point.)
//
// The host entry points are their argument checks and a call of one of the two
// serial drivers (wc_hostserial.cpp): forward_serial with wc_forward_levels as
// the device step, payload_serial with wc_inverse_levels and the box readback.
#include "wc_ctx.h"

#include <vector>

using namespace wc;

namespace wc {

// the round trip of the level modes' forward_serial calls: wc_inverse_levels + wc_rmse
RoundTrip levels_round_trip(wc_ctx* c, int dtype, const wc_unit* units, const int32_t* levels) {
    return [=](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets) {
        const int rc = wc_inverse_levels(c, d_payload, d_offsets, units + a, m, levels + a, (float*)c->h_out.p);
        return rc ? rc
                  : wc_rmse(c, c->h_cells.p, dtype, (const float*)c->h_out.p, units + a, m, (double*)c->h_rmse.p + a);
    };
}

}  // namespace wc

extern "C" {

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
    return forward_serial(
        c, cells, dtype, units, n, payload, cap, offsets, kept, nullptr,
        [&](int a, int m, const void* d_cells, uint8_t* pay, uint64_t run_bound, uint64_t* doff, uint32_t* dkept) {
            return wc_forward_levels(c, d_cells, dtype, units + a, m, levels + a, keep, thresh, pay, run_bound, doff,
                                     dkept);
        },
        nullptr, {});
}

int wc_inverse_levels_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    std::vector<uint64_t> end;
    std::vector<int32_t> from_headers;
    if ((rc = payload_ends(c, payload, offsets, n, end, levels ? nullptr : &from_headers))) return rc;
    if (!levels) levels = from_headers.data();
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if ((rc = set_device(c))) return rc;
    SerialOut o;
    o.out_units = units;
    o.out = out;
    o.out_bytes = sizeof(float) * cells_extent(units, n);
    return payload_serial(c, payload, offsets, end.data(), units, n,
                          [&](int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets, uint64_t) {
                              return wc_inverse_levels(c, d_payload, d_offsets, units + a, m, levels + a,
                                                       (float*)c->h_out.p);
                          },
                          o);
}

}  // extern "C"
