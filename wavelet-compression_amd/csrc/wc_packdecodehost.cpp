// wc_packdecodehost.cpp — host forms of the decoders over packed units
// (include/wavelet_amd.h "Decoding packed units directly"): wc_inverse_packed_host,
// wc_inverse_packed_coarse_host and wc_inverse_packed_region_host.
//
// One driver.  It checks every unit on the host first, with the format's host
// rule (what the device would refuse fails the call here, before anything is
// uploaded, so the outputs stay untouched), then runs its unit runs
// (WC_OPT_HOST_CHUNK, by the cells of the full-size units) one after another on
// the context's stream, as wc_inverse_levels_host and the region host driver do:
// the run's packed bytes up (the smaller form), the device call, only the
// result cells back.  Nothing here is sized by wc_payload_bound.
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
    const uint64_t ext = cells_extent(out_units, n);
    const std::vector<int> rb = level_runs(c, units, n);
    const int nr = (int)rb.size() - 1;
    // a run's packed bytes [lo, hi) upload to the same distance from an 8-B boundary
    // (units stay 4 mod 8); its offsets are rebased to that copy
    auto span = [&](int r, uint64_t& lo, uint64_t& hi) {
        lo = UINT64_MAX;
        hi = 0;
        for (int i = rb[r]; i < rb[r + 1]; ++i) {
            lo = std::min(lo, packed_offsets[i]);
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
        const uint64_t shift = p0 & 7;  // 4
        for (int i = 0; i < m; ++i) ro[i] = packed_offsets[a + i] - p0 + shift;
        hipError_t e;
        if ((e = hipMemcpyAsync((uint8_t*)c->h_payload.p + shift, packed + p0, p1 - p0, hipMemcpyHostToDevice,
                                c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(c->h_offsets.p, ro.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice, c->stream)) !=
                hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return hip_fail(c, e, "packed upload");
        }
        const uint8_t* d_packed = (const uint8_t*)c->h_payload.p;
        const uint64_t* d_off = (const uint64_t*)c->h_offsets.p;
        const uint64_t cap = shift + (p1 - p0);
        float* d_out = (float*)c->h_out.p;
        switch (mode) {
            case Mode::Full:
                rc = wc_inverse_packed(c, d_packed, d_off, cap, units + a, m, levels + a, d_out);
                break;
            case Mode::Coarse:
                rc = wc_inverse_packed_coarse(c, d_packed, d_off, cap, units + a, m, levels + a, reduce + a,
                                              out_units + a, d_out);
                break;
            case Mode::Region:
                rc = wc_inverse_packed_region(c, d_packed, d_off, cap, units + a, m, levels + a,
                                              reduce ? reduce + a : nullptr, regions + a, out_units + a, d_out);
                break;
        }
        // ro is rewritten by the next run: the uploads have finished after this synchronize.  A unit the
        // device refused after all fails the call before this run's cells cross back.
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (rc) return rc;
        if (es != hipSuccess) return hip_fail(c, es, "packed decode");
        if ((rc = check_kernel_errors(c))) return rc;
        // the units' boxes, back-to-back ones in one copy (cells no unit owns stay as they were)
        e = hipSuccess;
        for (int i = a; i < a + m && e == hipSuccess;) {
            uint64_t lo = out_units[i].cell_offset,
                     hi = lo + (uint64_t)out_units[i].nx * out_units[i].ny * out_units[i].nz;
            for (++i; i < a + m && out_units[i].cell_offset == hi; ++i)
                hi += (uint64_t)out_units[i].nx * out_units[i].ny * out_units[i].nz;
            if (hi > lo)
                e = hipMemcpyAsync(out + lo, (const float*)d_out + lo, sizeof(float) * (hi - lo), hipMemcpyDeviceToHost,
                                   c->stream);
        }
        const hipError_t eb = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || eb != hipSuccess) return hip_fail(c, e != hipSuccess ? e : eb, "box readback");
    }
    return WC_OK;
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
