// wc_packdecodehost.cpp — host forms of the decoders over packed units
// (include/wavelet_amd.h "Decoding packed units directly"): wc_inverse_packed_host,
// wc_inverse_packed_coarse_host and wc_inverse_packed_region_host.
//
// One function behind the three.  It checks every unit on the host first, with
// the format's host rule (what the device would refuse fails the call here,
// before anything is uploaded, so the outputs stay untouched), then calls
// payload_serial (wc_hostserial.cpp) in its checked form: per run (by the cells
// of the full-size units) the packed bytes up (the smaller form), the device
// call, the device's verdict, and only then the result cells back.
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace {

enum class Mode { Full, Coarse, Region };

int inverse_packed_host(wc_ctx* c, Mode mode, const uint8_t* packed, const uint64_t* packed_offsets,
                        const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                        const wc_region* regions, const wc_unit* out_units, float* out) {
    int rc;
    if ((rc = validate_pack(c, units, n)) || (levels && (rc = validate_levels(c, units, n, levels)))) return rc;
    // unit u's bytes, from its header and width table; its L from its tag
    std::vector<uint64_t> end(n);
    std::vector<int32_t> from_tags(n);
    for (int i = 0; i < n; ++i) {
        if ((packed_offsets[i] & 7) != 4) return fail(c, WC_ERR_INVALID, "packed offsets must be 4 (mod 8)");
        const uint8_t* p = packed + packed_offsets[i];
        int32_t h[5];
        std::memcpy(h, p, 20);
        const uint64_t cells = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        uint64_t len = 0;
        int L = 0, V = 0;
        // the table is read only where the header stands for the unit (its length is then at most the unit's)
        if (h[0] != units[i].nx || h[1] != units[i].ny || h[2] != units[i].nz || h[4] < 0 || (uint64_t)h[4] > cells ||
            wc_payload_packed(p, 20, &L, &V) != WC_OK || V < 2 || (levels && levels[i] != L) ||
            wc_packed_size(p, 20 + (((uint64_t)h[4] + 63) / 64 + 7) / 8 * 8, &len) != WC_OK)
            return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": malformed packed unit");
        from_tags[i] = L;
        end[i] = packed_offsets[i] + len;
    }
    if (!levels) levels = from_tags.data();
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if (mode == Mode::Coarse && (rc = validate_coarse(c, units, n, levels, reduce, out_units))) return rc;
    if (mode == Mode::Region && (rc = validate_region(c, units, n, levels, reduce, regions, out_units))) return rc;
    if ((rc = set_device(c))) return rc;
    SerialOut o;
    o.out_units = out_units;
    o.out = out;
    o.out_bytes = sizeof(float) * cells_extent(out_units, n) + 16;
    o.checked = true;  // a refused unit fails the call with its run's output untouched
    return payload_serial(
        c, packed, packed_offsets, end.data(), units, n,
        [&](int a, int m, const uint8_t* d_packed, const uint64_t* d_off, uint64_t cap) {
            float* d_out = (float*)c->h_out.p;
            switch (mode) {
                case Mode::Full:
                    return wc_inverse_packed(c, d_packed, d_off, cap, units + a, m, levels + a, d_out);
                case Mode::Coarse:
                    return wc_inverse_packed_coarse(c, d_packed, d_off, cap, units + a, m, levels + a, reduce + a,
                                                    out_units + a, d_out);
                default:
                    return wc_inverse_packed_region(c, d_packed, d_off, cap, units + a, m, levels + a,
                                                    reduce ? reduce + a : nullptr, regions + a, out_units + a, d_out);
            }
        },
        o);
}

}  // namespace

extern "C" {

int wc_inverse_packed_host(wc_ctx* c, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units, int n,
                           const int32_t* levels, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!packed || !packed_offsets || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    return inverse_packed_host(c, Mode::Full, packed, packed_offsets, units, n, levels, nullptr, nullptr, units, out);
}

int wc_inverse_packed_coarse_host(wc_ctx* c, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units,
                                  int n, const int32_t* levels, const int32_t* reduce, const wc_unit* out_units,
                                  float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!packed || !packed_offsets || !reduce || !out_units || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    return inverse_packed_host(c, Mode::Coarse, packed, packed_offsets, units, n, levels, reduce, nullptr, out_units,
                               out);
}

int wc_inverse_packed_region_host(wc_ctx* c, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units,
                                  int n, const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                                  const wc_unit* out_units, float* out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!packed || !packed_offsets || !regions || !out_units || !out) return fail(c, WC_ERR_INVALID, "null buffer");
    return inverse_packed_host(c, Mode::Region, packed, packed_offsets, units, n, levels, reduce, regions, out_units,
                               out);
}

}  // extern "C"
