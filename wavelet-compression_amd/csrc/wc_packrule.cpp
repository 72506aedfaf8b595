// wc_packrule.cpp — the packed payload format on the host (include/wavelet_amd.h
// "Opt-in packed payloads"): the value rule q, the tag, the length of a packed
// unit from its header and width table, and the transcoder of one unit in each
// direction.  Plain C++ with no HIP includes: tests/cpp/test_pack.cpp links it
// alone under ASan + UBSan, and wc_pack.hip restates the same rule on the device
// (wc_packfmt.h holds what the two share).
#include "wavelet_amd.h"
#include "wc_packfmt.h"

#include <cstring>

namespace {

struct Hdr {
    int32_t W, H, D, tag, n;
};

inline uint64_t pad8(uint64_t v) { return (v + 7) & ~uint64_t(7); }

inline int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

}  // namespace

extern "C" {

uint32_t wc_pack_value(uint32_t bits, int vbytes) { return wc::pack_value(bits, vbytes); }

int32_t wc_packed_tag(int levels, int vbytes) {
    if (levels < 1 || levels > WC_MAX_LEVELS || vbytes < 2 || vbytes > 4) return 0;
    return -(16 * vbytes + levels);
}

int wc_payload_packed(const uint8_t* header, size_t len, int* levels, int* vbytes) {
    if (!header || !levels || !vbytes || len < 20) return WC_ERR_INVALID;
    Hdr h;
    std::memcpy(&h, header, sizeof h);
    int L = 0, V = 0;
    if (!wc::pack_header(h.W, h.H, h.D, h.tag, L, V)) return WC_ERR_FORMAT;
    *levels = L;
    *vbytes = V;
    return WC_OK;
}

int wc_packed_size(const uint8_t* unit, size_t avail, uint64_t* bytes) {
    if (!unit || !bytes || avail < 20) return WC_ERR_INVALID;
    Hdr h;
    std::memcpy(&h, unit, sizeof h);
    int L = 0, V = 0;
    if (!wc::pack_header(h.W, h.H, h.D, h.tag, L, V) || V == 0) return WC_ERR_FORMAT;
    const uint64_t cells = (uint64_t)h.W * (uint64_t)h.H * (uint64_t)h.D;
    if (h.n < 0 || (uint64_t)h.n > cells) return WC_ERR_FORMAT;
    const uint64_t n = (uint64_t)h.n, nch = (n + 63) / 64;
    if (avail < 20 + pad8(nch)) return WC_ERR_INVALID;
    uint64_t total = 20 + pad8(nch);
    for (uint64_t c = 0; c < nch; ++c) {
        const uint32_t w = unit[20 + c];
        if (w > 31) return WC_ERR_FORMAT;
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * (nch - 1);
        total += w * ((m + 7) / 8) + (uint64_t)V * m;
    }
    *bytes = total;
    return WC_OK;
}

int wc_packed_bound(const wc_unit* units, int n, int vbytes, uint64_t* bytes) {
    if (n < 0 || (n > 0 && !units) || !bytes || vbytes < 2 || vbytes > 4) return WC_ERR_INVALID;
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) {
        if (units[i].nx < 0 || units[i].ny < 0 || units[i].nz < 0) return WC_ERR_INVALID;
        b += wc::pack_slot((uint64_t)units[i].nx * (uint64_t)units[i].ny * (uint64_t)units[i].nz, vbytes);
    }
    *bytes = b;
    return WC_OK;
}

int wc_pack_unit(const uint8_t* payload, size_t len, int vbytes, uint8_t* out, size_t cap, size_t* written) {
    if (!payload || !out || !written || len < 20 || vbytes < 2 || vbytes > 4) return WC_ERR_INVALID;
    Hdr h;
    std::memcpy(&h, payload, sizeof h);
    int L = 0, V = 0;
    if (!wc::pack_header(h.W, h.H, h.D, h.tag, L, V) || V != 0) return WC_ERR_FORMAT;
    const uint64_t cells = (uint64_t)h.W * (uint64_t)h.H * (uint64_t)h.D;
    if (h.n < 0 || (uint64_t)h.n > cells) return WC_ERR_FORMAT;
    const uint64_t n = (uint64_t)h.n, nch = (n + 63) / 64;
    if (len < 20 + 8 * n) return WC_ERR_INVALID;
    const uint8_t* pairs = payload + 20;
    // the widths first: they give the length, so nothing is written into a short buffer
    uint64_t total = 20 + pad8(nch);
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * (nch - 1);
        uint32_t acc = 0;
        for (uint64_t j = 0; j < m; ++j) {
            uint32_t run;
            std::memcpy(&run, pairs + 8 * (64 * c + j), 4);
            acc |= run;
        }
        if (acc & 0x80000000u) return WC_ERR_FORMAT;  // a negative run
        total += (uint64_t)bit_length(acc) * ((m + 7) / 8) + (uint64_t)vbytes * m;
    }
    if (cap < total) return WC_ERR_INVALID;
    const int32_t head[5] = {h.W, h.H, h.D, wc_packed_tag(L, vbytes), h.n};
    std::memcpy(out, head, 20);
    std::memset(out + 20, 0, pad8(nch));
    uint8_t* p = out + 20 + pad8(nch);
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * (nch - 1), pl = (m + 7) / 8;
        uint32_t run[64], val[64], acc = 0;
        for (uint64_t j = 0; j < m; ++j) {
            std::memcpy(&run[j], pairs + 8 * (64 * c + j), 4);
            std::memcpy(&val[j], pairs + 8 * (64 * c + j) + 4, 4);
            val[j] = wc::pack_value(val[j], vbytes);
            acc |= run[j];
        }
        const int w = bit_length(acc);
        out[20 + c] = (uint8_t)w;
        std::memset(p, 0, (size_t)w * pl);
        for (int b = 0; b < w; ++b, p += pl)
            for (uint64_t j = 0; j < m; ++j) p[j / 8] |= (uint8_t)(((run[j] >> b) & 1u) << (j % 8));
        for (int q = 0; q < vbytes; ++q, p += m)
            for (uint64_t j = 0; j < m; ++j) p[j] = (uint8_t)(val[j] >> (8 * (3 - q)));
    }
    *written = (size_t)total;
    return WC_OK;
}

int wc_unpack_unit(const uint8_t* packed, size_t len, uint8_t* out, size_t cap, size_t* written) {
    if (!packed || !out || !written || len < 20) return WC_ERR_INVALID;
    uint64_t total = 0;
    const int rc = wc_packed_size(packed, len, &total);
    if (rc != WC_OK) return rc;
    if (len < total) return WC_ERR_INVALID;
    Hdr h;
    std::memcpy(&h, packed, sizeof h);
    int L = 0, V = 0;
    (void)wc::pack_header(h.W, h.H, h.D, h.tag, L, V);  // wc_packed_size has accepted it
    const uint64_t n = (uint64_t)h.n, nch = (n + 63) / 64;
    if (cap < 20 + 8 * n) return WC_ERR_INVALID;
    const int32_t head[5] = {h.W, h.H, h.D, L >= 2 ? -L : (int32_t)((int64_t)h.W * h.H * h.D), h.n};
    std::memcpy(out, head, 20);
    const uint8_t* p = packed + 20 + pad8(nch);
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * (nch - 1), pl = (m + 7) / 8;
        const int w = packed[20 + c];
        uint32_t run[64] = {}, val[64] = {};
        for (int b = 0; b < w; ++b, p += pl)
            for (uint64_t j = 0; j < m; ++j) run[j] |= (uint32_t)((p[j / 8] >> (j % 8)) & 1u) << b;
        for (int q = 0; q < V; ++q, p += m)
            for (uint64_t j = 0; j < m; ++j) val[j] |= (uint32_t)p[j] << (8 * (3 - q));
        for (uint64_t j = 0; j < m; ++j) {
            std::memcpy(out + 20 + 8 * (64 * c + j), &run[j], 4);
            std::memcpy(out + 20 + 8 * (64 * c + j) + 4, &val[j], 4);
        }
    }
    *written = (size_t)(20 + 8 * n);
    return WC_OK;
}

}  // extern "C"
