// wc_packhost.cpp — host side of the packed payloads (include/wavelet_amd.h
// "Opt-in packed payloads"): the argument checks, the per-batch descriptors and
// the entry points wc_pack, wc_unpack, wc_pack_host and wc_unpack_host.  (The
// format's host rule is in wc_packrule.cpp, plain C++; the kernels in
// wc_pack.hip.)
//
// The descriptors (slot offsets in both layouts, one tile per kPackTile cells)
// depend on the units' dimensions and the value bytes only.  They stay on the
// device while a batch recurs, so a repeated call uploads nothing; a new batch
// uploads them and waits for that copy once, as a new plan does.
//
// The host forms are one upload, the device call, the dense packing of the
// slots and one download.  They are not pipelined over WC_OPT_HOST_CHUNK runs.
#include "wc_ctx.h"
#include "wc_packfmt.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace wc {
hipError_t launch_dense(hipStream_t, bool standard, int n, const uint64_t* bytes, const uint32_t* kept,
                        const uint64_t* src_off, const uint8_t* src, uint64_t* dense, uint8_t* dst);
}

namespace wc {

int validate_pack(wc_ctx* c, const wc_unit* units, int n) {
    for (int i = 0; i < n; ++i)
        if ((uint64_t)units[i].nx * units[i].ny * units[i].nz > kPackMaxCells)
            return fail(c, WC_ERR_INVALID,
                        "unit " + std::to_string(i) + ": more than WC_PACK_MAX_CELLS cells (the device transcoders sum a "
                        "unit's width table per tile)");
    return WC_OK;
}

}  // namespace wc

namespace {

// The batch's descriptors on the device (c->pk_desc: PackDesc[n] | FTile[pk_ntiles]).
int pack_plan(wc_ctx* c, const wc_unit* units, int n, int vbytes) {
    bool same = c->pk_vbytes == vbytes && (int)c->pk_key.size() == n && c->pk_desc.p;
    for (int i = 0; same && i < n; ++i)
        same = c->pk_key[i].nx == units[i].nx && c->pk_key[i].ny == units[i].ny && c->pk_key[i].nz == units[i].nz;
    if (same) return WC_OK;
    c->pk_key.clear();
    std::vector<PackDesc> desc(n);
    std::vector<FTile> tiles;
    uint64_t pk = 4, pay = 4;
    for (int i = 0; i < n; ++i) {
        const uint64_t cells = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        desc[i] = PackDesc{pk, pay, units[i].nx, units[i].ny, units[i].nz, (uint32_t)cells};
        pk += pack_slot(cells, vbytes);
        pay += 24 + 8 * cells;
        const uint32_t nt = std::max<uint32_t>(1u, (uint32_t)((cells + kPackTile - 1) / kPackTile));
        for (uint32_t t = 0; t < nt; ++t) tiles.push_back(FTile{(uint32_t)i, t});
    }
    const size_t db = sizeof(PackDesc) * n, tb = sizeof(FTile) * tiles.size();
    int rc;
    if ((rc = ensure(c, c->pk_desc, db + tb))) return rc;
    hipError_t e;
    if ((e = hipMemcpyAsync(c->pk_desc.p, desc.data(), db, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync((uint8_t*)c->pk_desc.p + db, tiles.data(), tb, hipMemcpyHostToDevice, c->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)  // the host vectors back the copies
        return hip_fail(c, e, "pack descriptors upload");
    c->pk_key.assign(units, units + n);
    c->pk_vbytes = vbytes;
    c->pk_ntiles = (uint32_t)tiles.size();
    return WC_OK;
}

const FTile* pack_tiles(const wc_ctx* c, int n) {
    return (const FTile*)((const uint8_t*)c->pk_desc.p + sizeof(PackDesc) * n);
}

}  // namespace

extern "C" {

int wc_pack(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n, int vbytes,
            uint8_t* d_packed, uint64_t cap, uint64_t* d_packed_offsets, uint64_t* d_packed_bytes) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (vbytes < 2 || vbytes > 4) return fail(c, WC_ERR_INVALID, "vbytes outside 2..4");
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !d_packed || !d_packed_offsets || !d_packed_bytes)
        return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_pack(c, units, n))) return rc;
    uint64_t bound = 0;
    (void)wc_packed_bound(units, n, vbytes, &bound);
    if (cap < bound) return fail(c, WC_ERR_INVALID, "packed_capacity < wc_packed_bound");
    if ((rc = check_aligned(c, d_payload, "payload", 4)) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_packed, "packed")) || (rc = check_aligned(c, d_packed_offsets, "packed offsets", 8)) ||
        (rc = check_aligned(c, d_packed_bytes, "packed bytes", 8)))
        return rc;
    if ((rc = set_device(c)) || (rc = pack_plan(c, units, n, vbytes))) return rc;
    StageTimer t(c, WC_STAGE_PACK);
    const hipError_t e = launch_pack_units(c->stream, (const PackDesc*)c->pk_desc.p, pack_tiles(c, n), c->pk_ntiles,
                                           d_payload, d_offsets, vbytes, n, d_packed, d_packed_offsets, d_packed_bytes,
                                           (uint32_t*)c->errflag.p);
    if (e != hipSuccess) return hip_fail(c, e, "pack launch");
    c->err_check_pending = true;  // refused source units surface at the next wc_synchronize
    return WC_OK;
}

int wc_unpack(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_packed_offsets, uint64_t packed_capacity,
              const wc_unit* units, int n, uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_packed || !d_packed_offsets || !d_payload || !d_offsets || !d_kept)
        return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_pack(c, units, n))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_packed, "packed", 8)) || (rc = check_aligned(c, d_packed_offsets, "packed offsets", 8)) ||
        (rc = check_aligned(c, d_payload, "payload")) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_kept, "kept", 4)))
        return rc;
    // the descriptors' packed slots are not read here: any value bytes give the same forward slots
    if ((rc = set_device(c)) || (rc = pack_plan(c, units, n, c->pk_vbytes ? c->pk_vbytes : 4))) return rc;
    StageTimer t(c, WC_STAGE_PACK);
    const hipError_t e = launch_unpack_units(c->stream, (const PackDesc*)c->pk_desc.p, pack_tiles(c, n), c->pk_ntiles,
                                             d_packed, d_packed_offsets, packed_capacity, n, d_payload, d_offsets,
                                             d_kept, (uint32_t*)c->errflag.p);
    if (e != hipSuccess) return hip_fail(c, e, "unpack launch");
    c->err_check_pending = true;  // refused packed units surface at the next wc_synchronize
    return WC_OK;
}

int wc_pack_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n, int vbytes,
                 uint8_t* packed, uint64_t cap, uint64_t* packed_offsets, uint64_t* packed_bytes) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (vbytes < 2 || vbytes > 4) return fail(c, WC_ERR_INVALID, "vbytes outside 2..4");
    if (n == 0) return WC_OK;
    if (!payload || !offsets || !packed || !packed_offsets || !packed_bytes) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_pack(c, units, n))) return rc;
    // unit u's source bytes: its header and the pairs the header announces (at most its cells: more is refused
    // on the device, and the bytes past them are not needed for that)
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int i = 0; i < n; ++i) {
        if (offsets[i] & 3) return fail(c, WC_ERR_INVALID, "offsets must be multiples of 4");
        int32_t nrle;
        std::memcpy(&nrle, payload + offsets[i] + 16, 4);
        const uint64_t cells = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + 20 + 8 * std::min<uint64_t>((uint64_t)std::max(nrle, 0), cells));
    }
    uint64_t bound = 0;
    (void)wc_packed_bound(units, n, vbytes, &bound);
    if ((rc = set_device(c))) return rc;
    const uint64_t shift = lo & 7;
    if ((rc = ensure(c, c->pk_in, hi - lo + 16)) || (rc = ensure(c, c->pk_out, bound)) ||
        (rc = ensure(c, c->h_packed, bound)) || (rc = ensure(c, c->pk_off, sizeof(uint64_t) * (3 * (size_t)n + 2))) ||
        (rc = ensure(c, c->pk_bytes, sizeof(uint64_t) * n)))
        return rc;
    uint64_t* d_src = (uint64_t*)c->pk_off.p;  // source offsets [n] | slot offsets [n + 1] | dense offsets [n + 1]
    uint64_t* d_slot = d_src + n;
    uint64_t* d_dense = d_slot + n + 1;
    std::vector<uint64_t> ro(n), meta(2 * (size_t)n + 1);
    for (int i = 0; i < n; ++i) ro[i] = offsets[i] - lo + shift;
    hipError_t e;
    if ((e = hipMemcpyAsync((uint8_t*)c->pk_in.p + shift, payload + lo, hi - lo, hipMemcpyHostToDevice, c->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(d_src, ro.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return hip_fail(c, e, "payload upload");
    }
    if ((rc = wc_pack(c, (const uint8_t*)c->pk_in.p, d_src, units, n, vbytes, (uint8_t*)c->pk_out.p, bound, d_slot,
                      (uint64_t*)c->pk_bytes.p))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    e = launch_dense(c->stream, false, n, (const uint64_t*)c->pk_bytes.p, nullptr, d_slot, (const uint8_t*)c->pk_out.p,
                     d_dense, (uint8_t*)c->h_packed.p);
    if (e == hipSuccess)
        e = hipMemcpyAsync(meta.data(), d_dense, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(meta.data() + n + 1, c->pk_bytes.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);  // ro and the caller's payload are consumed
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "sizes readback");
    if ((rc = check_kernel_errors(c))) return rc;  // outputs untouched
    if (meta[n] > cap) return fail(c, WC_ERR_INVALID, "packed_capacity below the packed units' bytes");
    if ((e = hipMemcpy(packed + 4, (const uint8_t*)c->h_packed.p + 4, meta[n] - 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(c, e, "packed readback");
    std::memcpy(packed_offsets, meta.data(), sizeof(uint64_t) * (n + 1));
    std::memcpy(packed_bytes, meta.data() + n + 1, sizeof(uint64_t) * n);
    return WC_OK;
}

int wc_unpack_host(wc_ctx* c, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units, int n,
                   uint8_t* payload, uint64_t cap, uint64_t* offsets, uint32_t* kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!packed || !packed_offsets || !payload || !offsets || !kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_pack(c, units, n))) return rc;
    // unit u's packed bytes, from its header and width table (the host rule refuses what the device would)
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int i = 0; i < n; ++i) {
        if ((packed_offsets[i] & 7) != 4)
            return fail(c, WC_ERR_INVALID, "packed offsets must be 4 (mod 8)");
        const uint8_t* p = packed + packed_offsets[i];
        int32_t h[5];
        std::memcpy(h, p, 20);
        const uint64_t cells = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        uint64_t len = 0;
        // the table is read only where the header stands for the unit (its length is then at most the unit's)
        if (h[0] != units[i].nx || h[1] != units[i].ny || h[2] != units[i].nz || h[4] < 0 || (uint64_t)h[4] > cells ||
            wc_packed_size(p, 20 + (((uint64_t)h[4] + 63) / 64 + 7) / 8 * 8, &len) != WC_OK)
            return fail(c, WC_ERR_FORMAT, "unit " + std::to_string(i) + ": malformed packed unit");
        lo = std::min(lo, packed_offsets[i]);
        hi = std::max(hi, packed_offsets[i] + len);
    }
    const uint64_t bound = wc_payload_bound(units, n);
    if ((rc = set_device(c))) return rc;
    const uint64_t shift = lo & 7;  // 4
    if ((rc = ensure(c, c->pk_in, hi - lo + 16)) || (rc = ensure(c, c->h_payload, bound)) ||
        (rc = ensure(c, c->h_packed, bound)) || (rc = ensure(c, c->pk_off, sizeof(uint64_t) * (3 * (size_t)n + 2))) ||
        (rc = ensure(c, c->h_kept, 4ull * n)))
        return rc;
    uint64_t* d_src = (uint64_t*)c->pk_off.p;  // packed offsets [n] | slot offsets [n + 1] | dense offsets [n + 1]
    uint64_t* d_slot = d_src + n;
    uint64_t* d_dense = d_slot + n + 1;
    std::vector<uint64_t> ro(n), po(n + 1);
    std::vector<uint32_t> hk(n);
    for (int i = 0; i < n; ++i) ro[i] = packed_offsets[i] - lo + shift;
    hipError_t e;
    if ((e = hipMemcpyAsync((uint8_t*)c->pk_in.p + shift, packed + lo, hi - lo, hipMemcpyHostToDevice, c->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(d_src, ro.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return hip_fail(c, e, "packed upload");
    }
    if ((rc = wc_unpack(c, (const uint8_t*)c->pk_in.p, d_src, shift + (hi - lo), units, n, (uint8_t*)c->h_payload.p,
                        bound, d_slot, (uint32_t*)c->h_kept.p))) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    e = launch_dense(c->stream, true, n, nullptr, (const uint32_t*)c->h_kept.p, d_slot, (const uint8_t*)c->h_payload.p,
                     d_dense, (uint8_t*)c->h_packed.p);
    if (e == hipSuccess) e = hipMemcpyAsync(po.data(), d_dense, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hk.data(), c->h_kept.p, 4ull * n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || es != hipSuccess) return hip_fail(c, e != hipSuccess ? e : es, "sizes readback");
    if ((rc = check_kernel_errors(c))) return rc;  // outputs untouched
    if (po[n] > cap) return fail(c, WC_ERR_INVALID, "payload_capacity below the payloads' bytes");
    if ((e = hipMemcpy(payload + 4, (const uint8_t*)c->h_packed.p + 4, po[n] - 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(c, e, "payload readback");
    std::memcpy(offsets, po.data(), sizeof(uint64_t) * (n + 1));
    std::memcpy(kept, hk.data(), 4ull * n);
    return WC_OK;
}

}  // extern "C"
