// wc_hostserial.cpp — the two serial host drivers behind the opt-in modes' _host
// entry points (include/wavelet_amd.h), and the helpers they share.  Plain C++
// over the HIP runtime API and launch_pack: no kernels of its own, also built
// against the CPU fake of that API (tests/cpp/test_hostserial.cpp).
//
// Both split the batch into unit runs (WC_OPT_HOST_CHUNK, by the cells of the
// full-size units) and take them one after another on the context's stream; they
// are not pipelined over the copy streams as wc_forward_host is (wc_hostpipe.cpp).
// forward_serial: cells in, packed payloads out.  payload_serial: payload bytes
// in; the units' boxes or (thinning, layers) packed payloads out.  The layers add a
// second stream to it: a second packed output (a split) or a second input (a merge).
//
// One rule on errors: after a driver's first enqueue every return goes through
// serial_finish, which drains the stream first.  No copy that reads or writes
// the caller's buffers, or a host vector of the call, outlives the call.
#include "wc_ctx.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace wc {

// Unit u's bytes of a standard payload: its header and the nrle pairs the header
// announces (wc_inverse_host sizes its copies the same way; offsets has n entries,
// in any order).  With from_headers, each unit's L from its header as well.
int payload_ends(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, int n, std::vector<uint64_t>& end,
                 std::vector<int32_t>* from_headers) {
    end.resize(n);
    if (from_headers) from_headers->resize(n);
    for (int i = 0; i < n; ++i) {
        if (offsets[i] & 3) return fail(c, WC_ERR_INVALID, "offsets must be multiples of 4");
        int32_t nrle;
        std::memcpy(&nrle, payload + offsets[i] + 16, 4);
        end[i] = offsets[i] + 20 + 8ull * (uint64_t)std::max(nrle, 0);
        if (from_headers) {
            int L = 0;
            if (wc_payload_levels(payload + offsets[i], 20, &L) != WC_OK)
                return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": malformed payload header");
            (*from_headers)[i] = L;
        }
    }
    return WC_OK;
}

namespace {

// contiguous unit runs of at least opt_host_chunk cells (0: one run)
std::vector<int> serial_runs(const wc_ctx* c, const wc_unit* units, int n) {
    std::vector<int> rb{0};
    if (c->opt_host_chunk > 0) {
        uint64_t acc = 0;
        for (int i = 0; i < n; ++i) {
            acc += (uint64_t)units[i].nx * units[i].ny * units[i].nz;
            if (acc >= (uint64_t)c->opt_host_chunk && i + 1 < n) {
                rb.push_back(i + 1);
                acc = 0;
            }
        }
    }
    rb.push_back(n);
    return rb;
}

// the span of cells the units [a, a + m) own (hi <= lo: none)
void cell_span(const wc_unit* units, int a, int m, uint64_t& lo, uint64_t& hi) {
    lo = UINT64_MAX;
    hi = 0;
    for (int i = a; i < a + m; ++i) {
        const uint64_t cnt = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        if (!cnt) continue;
        lo = std::min(lo, units[i].cell_offset);
        hi = std::max(hi, units[i].cell_offset + cnt);
    }
}

// the span of bytes the units [a, a + m) read: unit u's are [offsets[u], end[u])
void byte_span(const uint64_t* offsets, const uint64_t* end, int a, int m, uint64_t& lo, uint64_t& hi) {
    lo = UINT64_MAX;
    hi = 0;
    for (int i = a; i < a + m; ++i) {
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, end[i]);
    }
}

// the largest run's unit count and wc_payload_bound
void run_sizes(const std::vector<int>& rb, const wc_unit* units, int& run_units, uint64_t& run_bound) {
    run_units = 0;
    run_bound = 0;
    for (size_t r = 0; r + 1 < rb.size(); ++r) {
        run_units = std::max(run_units, rb[r + 1] - rb[r]);
        run_bound = std::max(run_bound, wc_payload_bound(units + rb[r], rb[r + 1] - rb[r]));
    }
}

// the staging of a run's dense packing: launch_pack's output and the per-unit metadata
int ensure_pack_staging(wc_ctx* c, int run_units, uint64_t run_bound) {
    int rc;
    if ((rc = ensure(c, c->h_packed, run_bound)) || (rc = ensure(c, c->h_offsets, sizeof(uint64_t) * (run_units + 1))) ||
        (rc = ensure(c, c->h_poff, sizeof(uint64_t) * (run_units + 1))) || (rc = ensure(c, c->h_kept, 4ull * run_units)))
        return rc;
    return WC_OK;
}

// Run [a, a + m), whose slots (wc_forward's layout, the plan's units) are at d_slots: pack them
// densely (offsets stay == 4 mod 8, as wc_forward_host does); then the tail: the sizes and kept
// counts back, the run's offsets rebased to R, its bytes to payload + R.
// (d_kept: the slots' pair counts; NULL: c->h_kept)
hipError_t pack_run(wc_ctx* c, int m, const uint8_t* d_slots, const void* d_kept = nullptr) {
    return launch_pack(c->stream, (const UnitDev*)c->plan.d_units.p, m, (const uint32_t*)(d_kept ? d_kept : c->h_kept.p),
                       d_slots, (uint64_t*)c->h_poff.p, (uint8_t*)c->h_packed.p);
}

int packed_run_tail(wc_ctx* c, int a, int m, std::vector<uint64_t>& po, uint8_t* payload, uint64_t cap, uint64_t* offsets,
                    uint32_t* kept, uint64_t& R, const void* d_kept = nullptr) {
    hipError_t e;
    if ((e = hipMemcpyAsync(po.data(), c->h_poff.p, sizeof(uint64_t) * (m + 1), hipMemcpyDeviceToHost, c->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(kept + a, d_kept ? d_kept : c->h_kept.p, 4ull * m, hipMemcpyDeviceToHost, c->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return hip_fail(c, e, "sizes readback");
    for (int i = 0; i < m; ++i) offsets[a + i] = R - 4 + po[i];
    const uint64_t span = po[m] - 4;
    if (R - 4 + po[m] > cap) return fail(c, WC_ERR_INVALID, "payload_capacity");
    if (span && (e = hipMemcpyAsync(payload + R, (const uint8_t*)c->h_packed.p + 4, span, hipMemcpyDeviceToHost,
                                    c->stream)) != hipSuccess)
        return hip_fail(c, e, "payload readback");
    R += po[m];
    return WC_OK;
}

// the boxes of units [a, a + m) from d_out, back-to-back ones in one copy (cells no unit owns stay as they were)
hipError_t boxes_back(wc_ctx* c, const wc_unit* units, int a, int m, const float* d_out, float* out) {
    hipError_t e = hipSuccess;
    for (int i = a; i < a + m && e == hipSuccess;) {
        uint64_t lo = units[i].cell_offset, hi = lo + (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        for (++i; i < a + m && units[i].cell_offset == hi; ++i) hi += (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        if (hi > lo)
            e = hipMemcpyAsync(out + lo, d_out + lo, sizeof(float) * (hi - lo), hipMemcpyDeviceToHost, c->stream);
    }
    return e;
}

// The single exit of both drivers.  After a clean run of every unit run: the end of the packed
// bytes and the per-unit results (packed output only: offsets set); then, whatever happened, the
// drain.  (A clean box readback has nothing in flight: each of its runs ended with a synchronize.)
int serial_finish(wc_ctx* c, int rc, int n, uint64_t* offsets, uint64_t R, const std::vector<UnitResult>& results) {
    hipError_t e = hipSuccess;
    if (rc == WC_OK && offsets) {
        offsets[n] = R - 4;
        for (const UnitResult& u : results)
            if (u.host && e == hipSuccess)
                e = hipMemcpyAsync(u.host, u.dev, u.stride * n, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = rc == WC_OK && !offsets ? hipSuccess : hipStreamSynchronize(c->stream);
    if (rc != WC_OK) return rc;
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "results readback");
    return check_kernel_errors(c);
}

}  // namespace

int forward_serial(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n, uint8_t* payload, uint64_t cap,
                   uint64_t* offsets, uint32_t* kept, double* rmse, const ForwardStep& step, const RoundTrip& trip,
                   std::vector<UnitResult> results) {
    int rc;
    const size_t esz = dtype == WC_F64 ? 8 : 4;
    const uint64_t ext = cells_extent(units, n);
    const std::vector<int> rb = serial_runs(c, units, n);
    const int nr = (int)rb.size() - 1;
    int run_units;
    uint64_t run_bound;
    run_sizes(rb, units, run_units, run_bound);
    if ((rc = ensure(c, c->h_cells, esz * ext)) || (rc = ensure(c, c->h_payload, run_bound)) ||
        (rc = ensure_pack_staging(c, run_units, run_bound)))
        return rc;
    if (rmse) {
        if ((rc = ensure(c, c->h_out, sizeof(float) * ext)) || (rc = ensure(c, c->h_rmse, sizeof(double) * n))) return rc;
        results.push_back({c->h_rmse.p, rmse, sizeof(double)});
    }
    std::vector<uint64_t> po(run_units + 1);
    uint64_t R = 4;  // run r's packed bytes [4, end) land at R (== 4 mod 8)
    auto run = [&](int a, int m) -> int {
        uint64_t lo, hi;
        cell_span(units, a, m, lo, hi);
        hipError_t e;
        if (hi > lo && (e = hipMemcpyAsync((uint8_t*)c->h_cells.p + esz * lo, (const uint8_t*)cells + esz * lo,
                                           esz * (hi - lo), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return hip_fail(c, e, "cells upload");
        uint8_t* pay = (uint8_t*)c->h_payload.p;
        uint64_t* doff = (uint64_t*)c->h_offsets.p;
        int rc2;
        if ((rc2 = step(a, m, c->h_cells.p, pay, run_bound, doff, (uint32_t*)c->h_kept.p))) return rc2;
        if ((e = pack_run(c, m, pay)) != hipSuccess) return hip_fail(c, e, "pack launch");
        // the round trip: the run's payloads back to cells, compared with the cells on the device
        if (rmse && (rc2 = trip(a, m, pay, doff))) return rc2;
        return packed_run_tail(c, a, m, po, payload, cap, offsets, kept, R);
    };
    rc = WC_OK;
    for (int r = 0; r < nr && rc == WC_OK; ++r) rc = run(rb[r], rb[r + 1] - rb[r]);
    return serial_finish(c, rc, n, offsets, R, results);
}

int payload_serial(wc_ctx* c, const uint8_t* bytes, const uint64_t* offsets, const uint64_t* end, const wc_unit* units,
                   int n, const PayloadStep& step, const SerialOut& o) {
    int rc;
    const bool packs = o.payload != nullptr;
    const std::vector<int> rb = serial_runs(c, units, n);
    const int nr = (int)rb.size() - 1;
    int run_units;
    uint64_t run_bound, run_bytes = 0, run_bytes2 = 0;
    run_sizes(rb, units, run_units, run_bound);
    for (int r = 0; r < nr; ++r) {
        uint64_t lo, hi;
        byte_span(offsets, end, rb[r], rb[r + 1] - rb[r], lo, hi);
        run_bytes = std::max(run_bytes, hi - lo);
        if (o.bytes2) {
            byte_span(o.offsets2, o.end2, rb[r], rb[r + 1] - rb[r], lo, hi);
            run_bytes2 = std::max(run_bytes2, hi - lo);
        }
    }
    if ((o.bytes2 || o.payload2) &&
        ((rc = ensure(c, c->h_second, o.bytes2 ? run_bytes2 + o.slack : run_bound)) ||
         (rc = ensure(c, c->h_second_off, sizeof(uint64_t) * (run_units + 1))) ||
         (rc = ensure(c, c->h_second_cnt, 4ull * run_units))))
        return rc;
    if ((rc = ensure(c, c->h_payload, run_bytes + o.slack)) || (rc = ensure(c, c->h_out, packs ? run_bound : o.out_bytes)) ||
        (rc = packs ? ensure_pack_staging(c, run_units, run_bound)
                    : ensure(c, c->h_offsets, sizeof(uint64_t) * run_units)))
        return rc;
    std::vector<uint64_t> ro(run_units), ro2(o.bytes2 ? run_units : 0), po(packs ? run_units + 1 : 0);
    uint64_t R = 4, R2 = 4;  // run r's packed bytes [4, end) land at R (== 4 mod 8); R2: the second output's
    auto run = [&](int a, int m) -> int {
        // the run's bytes [p0, p1) upload to the same distance from an 8-B boundary (pairs stay 8-B
        // aligned, packed units 4 mod 8); its offsets are rebased to that copy
        uint64_t p0, p1;
        byte_span(offsets, end, a, m, p0, p1);
        const uint64_t shift = o.shift + (p0 & 7);
        for (int i = 0; i < m; ++i) ro[i] = offsets[a + i] - p0 + shift;
        hipError_t e;
        if ((e = hipMemcpyAsync((uint8_t*)c->h_payload.p + shift, bytes + p0, p1 - p0, hipMemcpyHostToDevice,
                                c->stream)) != hipSuccess ||
            (e = hipMemcpyAsync(c->h_offsets.p, ro.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice, c->stream)) !=
                hipSuccess)
            return hip_fail(c, e, "payload upload");
        if (o.bytes2) {  // the second input of the run, by the same rule
            uint64_t q0, q1;
            byte_span(o.offsets2, o.end2, a, m, q0, q1);
            const uint64_t shift2 = o.shift + (q0 & 7);
            for (int i = 0; i < m; ++i) ro2[i] = o.offsets2[a + i] - q0 + shift2;
            if ((e = hipMemcpyAsync((uint8_t*)c->h_second.p + shift2, o.bytes2 + q0, q1 - q0, hipMemcpyHostToDevice,
                                    c->stream)) != hipSuccess ||
                (e = hipMemcpyAsync(c->h_second_off.p, ro2.data(), sizeof(uint64_t) * m, hipMemcpyHostToDevice,
                                    c->stream)) != hipSuccess)
                return hip_fail(c, e, "payload upload");
        }
        int rc2;
        if ((rc2 = step(a, m, (const uint8_t*)c->h_payload.p, (const uint64_t*)c->h_offsets.p, shift + (p1 - p0))))
            return rc2;
        if (packs) {
            // the plan the step left is the run's units': its slots are wc_forward's.  ro is rewritten by
            // the next run: the uploads have finished after the tail's synchronize.
            if ((e = pack_run(c, m, (const uint8_t*)c->h_out.p)) != hipSuccess) return hip_fail(c, e, "pack launch");
            if ((rc2 = packed_run_tail(c, a, m, po, o.payload, o.cap, o.out_offsets, o.kept, R)) || !o.payload2) return rc2;
            // the second output through the same staging (the first tail has synchronized; its last copy, out of
            // the staging, is ahead of this packing on the stream)
            if ((e = pack_run(c, m, (const uint8_t*)c->h_second.p, c->h_second_cnt.p)) != hipSuccess)
                return hip_fail(c, e, "pack launch");
            return packed_run_tail(c, a, m, po, o.payload2, o.cap2, o.out_offsets2, o.kept2, R2, c->h_second_cnt.p);
        }
        if (o.checked) {  // a unit the device refused after all fails the call before this run's cells cross back
            if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(c, e, "packed decode");
            if ((rc2 = check_kernel_errors(c))) return rc2;
        }
        e = boxes_back(c, o.out_units, a, m, (const float*)c->h_out.p, o.out);
        // ro is rewritten by the next run: the uploads have finished after this synchronize
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "box readback");
        return WC_OK;
    };
    rc = WC_OK;
    for (int r = 0; r < nr && rc == WC_OK; ++r) rc = run(rb[r], rb[r + 1] - rb[r]);
    if (rc == WC_OK && o.payload2) o.out_offsets2[n] = R2 - 4;
    return serial_finish(c, rc, n, packs ? o.out_offsets : nullptr, R, o.results);
}

}  // namespace wc
