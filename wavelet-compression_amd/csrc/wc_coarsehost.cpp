// wc_coarsehost.cpp — host side of the reduced-resolution inverse
// (include/wavelet_amd.h wc_inverse_coarse): the output units of a reduction
// (wc_coarse_units), the mode's argument checks and wc_inverse_coarse_host.
//
// The host entry point is wc_regionhost.cpp's inverse_compact_host without regions.
#include "wc_ctx.h"

#include <string>
#include <vector>

using namespace wc;

namespace wc {

// dmagic of wc_device.h div_rows for any divisor d >= 1 (positions < 2^31)
uint64_t rows_magic(int32_t d) {
    const int lg = ceil_log2(d);
    if ((d & (d - 1)) == 0) return (uint64_t)lg << 32;
    return ((uint64_t(1) << (31 + lg)) / (uint64_t)d + 1) | ((uint64_t)(31 + lg) << 32);
}

// The mode's preconditions beyond validate_levels, before anything is launched:
// a reduce per unit in 0..levels[u], 2^r dividing every dimension of a unit with
// cells, and out_units[u] carrying exactly the dims >> r.
int validate_coarse(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                    const wc_unit* out_units) {
    for (int i = 0; i < n; ++i) {
        const int r = reduce[i], L = levels[i];
        const std::string who = "unit " + std::to_string(i);
        if (r < 0 || r > L)
            return fail(c, WC_ERR_INVALID, who + ": reduce " + std::to_string(r) + " outside 0.." + std::to_string(L));
        const wc_unit& u = units[i];
        const uint64_t cells = (uint64_t)u.nx * u.ny * u.nz;
        if (cells && r >= 1 && ((u.nx | u.ny | u.nz) & ((1 << r) - 1)))
            return fail(c, WC_ERR_INVALID,
                        who + " (" + std::to_string(u.nx) + "x" + std::to_string(u.ny) + "x" + std::to_string(u.nz) +
                            "): reduce " + std::to_string(r) + " needs W, H and D divisible by " +
                            std::to_string(1 << r));
        const wc_unit& o = out_units[i];
        if (o.nx != u.nx >> r || o.ny != u.ny >> r || o.nz != u.nz >> r || o.reserved != 0)
            return fail(c, WC_ERR_INVALID,
                        who + ": out_units must carry " + std::to_string(u.nx >> r) + "x" + std::to_string(u.ny >> r) +
                            "x" + std::to_string(u.nz >> r) + " and reserved = 0 (wc_coarse_units)");
    }
    return WC_OK;
}

}  // namespace wc

extern "C" {

int wc_coarse_units(const wc_unit* units, const int32_t* reduce, int n, wc_unit* out, uint64_t* extent) {
    if (n < 0 || (n > 0 && (!units || !reduce || !out)) || !extent) return WC_ERR_INVALID;
    uint64_t cur = 0, ext = 0;
    for (int i = 0; i < n; ++i) {
        const wc_unit& u = units[i];
        const int r = reduce[i];
        if (u.nx < 0 || u.ny < 0 || u.nz < 0 || r < 0 || r > WC_MAX_LEVELS) return WC_ERR_INVALID;
        cur = (cur + 3) & ~uint64_t(3);
        out[i] = wc_unit{cur, u.nx >> r, u.ny >> r, u.nz >> r, 0};
        cur += (uint64_t)out[i].nx * out[i].ny * out[i].nz;
        ext = cur;
    }
    *extent = ext;
    return WC_OK;
}

int wc_inverse_coarse_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !reduce || !out_units || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    return inverse_compact_host(c, payload, offsets, units, n, levels, reduce, nullptr, out_units, out);
}

}  // extern "C"
