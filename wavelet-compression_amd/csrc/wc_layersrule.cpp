// wc_layersrule.cpp — the rule of the progressive layers on one standard payload
// (wc_split_unit and wc_merge_unit in include/wavelet_amd.h): the host restatement
// of wc_thin.hip's split and wc_layers.hip's merge.  A split is a thinning (wc_thinrule.cpp's wc_thin_unit, called
// as it stands) and its complement inside the canonical form; a merge is the union
// of two position-sorted pair lists.  Both write the reference's run rule on what
// they keep.
//
// Plain C++ without the HIP runtime, so that a test program links it under a
// sanitizer.
#include "wavelet_amd.h"

#include <cstring>
#include <vector>

namespace {

struct Pairs {
    int32_t h[5];
    uint64_t N;
    std::vector<uint32_t> pos, bits;  // the pairs below N, in position order
};

// The pairs of a standard payload at positions below N.  WC_ERR_FORMAT: no standard
// header, a negative count or run; WC_ERR_INVALID: fewer than 20 + 8 n bytes.
int open_pairs(const uint8_t* p, size_t len, Pairs& P) {
    if (len < 20) return WC_ERR_INVALID;
    int L = 0;
    const int rc = wc_payload_levels(p, 20, &L);  // a packed unit's tag is no level count
    if (rc != WC_OK) return rc;
    std::memcpy(P.h, p, sizeof P.h);
    if (P.h[4] < 0) return WC_ERR_FORMAT;
    P.N = (uint64_t)P.h[0] * (uint64_t)P.h[1] * (uint64_t)P.h[2];
    const uint64_t n = (uint64_t)P.h[4];
    if (P.N > 0x7fffffffull) return WC_ERR_FORMAT;
    if (len < 20 + 8 * n) return WC_ERR_INVALID;
    uint64_t q = 0;  // the next pair's position if its run were 0
    bool live = true;
    for (uint64_t k = 0; k < n; ++k) {
        int32_t run;
        uint32_t b;
        std::memcpy(&run, p + 20 + 8 * k, 4);
        std::memcpy(&b, p + 24 + 8 * k, 4);
        if (run < 0) return WC_ERR_FORMAT;
        if (!live) continue;  // (still looking for a negative run)
        q += (uint64_t)run;
        if (q >= P.N) {
            live = false;
            continue;
        }
        P.pos.push_back((uint32_t)q);
        P.bits.push_back(b);
        ++q;
    }
    return WC_OK;
}

// header h with pos.size() pairs, runs by the reference's rule
void emit(const int32_t* h, const std::vector<uint32_t>& pos, const std::vector<uint32_t>& bits, uint8_t* out) {
    int32_t hd[5] = {h[0], h[1], h[2], h[3], (int32_t)pos.size()};
    std::memcpy(out, hd, sizeof hd);
    int64_t last = -1;
    for (size_t i = 0; i < pos.size(); ++i) {
        const int32_t run = (int32_t)((int64_t)pos[i] - last - 1);
        std::memcpy(out + 20 + 8 * i, &run, 4);
        std::memcpy(out + 24 + 8 * i, &bits[i], 4);
        last = (int64_t)pos[i];
    }
}

}  // namespace

extern "C" int wc_split_unit(const uint8_t* payload, size_t len, const uint32_t* max_pairs, const float* thresh,
                             uint8_t* base, size_t base_cap, size_t* base_len, uint8_t* rest, size_t rest_cap,
                             size_t* rest_len, uint32_t* key, float* thresh_out) {
    if (!payload || !base || !base_len || !rest || !rest_len || (max_pairs != nullptr) == (thresh != nullptr))
        return WC_ERR_INVALID;
    Pairs P;
    int rc = open_pairs(payload, len, P);
    if (rc != WC_OK) return rc;
    // the base: the thinning itself, into a block of its own (nothing is written on a refusal)
    std::vector<uint8_t> b(20 + 8 * P.pos.size());
    size_t blen = 0;
    uint32_t T = 0;
    float th[WC_MAX_LEVELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if ((rc = wc_thin_unit(payload, len, max_pairs, thresh, b.data(), b.size(), &blen, &T, th)) != WC_OK) return rc;
    Pairs B;
    if ((rc = open_pairs(b.data(), blen, B)) != WC_OK) return rc;
    // the rest: the pairs of canon(P) that the base does not hold; both lists are in position order
    std::vector<uint32_t> rpos, rbits;
    size_t j = 0;
    for (size_t i = 0; i < P.pos.size(); ++i) {
        if (j < B.pos.size() && B.pos[j] == P.pos[i]) {
            ++j;
            continue;
        }
        const uint32_t m = P.bits[i] & 0x7fffffffu;
        if (m < 1u || m > 0x7f800000u) continue;  // +-0 or NaN: not in the canonical form
        rpos.push_back(P.pos[i]);
        rbits.push_back(P.bits[i]);
    }
    const size_t rlen = 20 + 8 * rpos.size();
    if (base_cap < blen || rest_cap < rlen) return WC_ERR_INVALID;
    std::memcpy(base, b.data(), blen);
    emit(P.h, rpos, rbits, rest);
    *base_len = blen;
    *rest_len = rlen;
    if (key) *key = T;
    if (thresh_out) {
        int L = 0;
        (void)wc_payload_levels(payload, 20, &L);
        std::memcpy(thresh_out, th, sizeof(float) * (size_t)L);
    }
    return WC_OK;
}

extern "C" int wc_merge_unit(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint8_t* out, size_t cap,
                             size_t* written) {
    if (!a || !b || !out || !written) return WC_ERR_INVALID;
    Pairs A, B;
    int rc;
    if ((rc = open_pairs(a, a_len, A)) != WC_OK || (rc = open_pairs(b, b_len, B)) != WC_OK) return rc;
    if (std::memcmp(A.h, B.h, 4 * sizeof(int32_t)) != 0) return WC_ERR_FORMAT;  // another unit, or another L
    std::vector<uint32_t> pos, bits;
    pos.reserve(A.pos.size() + B.pos.size());
    bits.reserve(A.pos.size() + B.pos.size());
    size_t i = 0, j = 0;
    while (i < A.pos.size() || j < B.pos.size()) {
        const bool ta = j == B.pos.size() || (i < A.pos.size() && A.pos[i] < B.pos[j]);
        if (i < A.pos.size() && j < B.pos.size() && A.pos[i] == B.pos[j]) return WC_ERR_FORMAT;  // an overlap
        pos.push_back(ta ? A.pos[i] : B.pos[j]);
        bits.push_back(ta ? A.bits[i] : B.bits[j]);
        ta ? ++i : ++j;
    }
    const size_t len = 20 + 8 * pos.size();
    if (cap < len) return WC_ERR_INVALID;
    emit(A.h, pos, bits, out);
    *written = len;
    return WC_OK;
}

// The extents of the device forms.  The base's slots are wc_thin_bound's; a rest slot and a merged slot
// hold every coefficient of the unit (the pair count of a payload is not known to the host).
extern "C" int wc_split_bound(const wc_unit* units, int n, const uint32_t* max_pairs, uint64_t* base_bytes,
                              uint64_t* rest_bytes) {
    if (n < 0 || (n > 0 && !units) || !base_bytes || !rest_bytes) return WC_ERR_INVALID;
    uint64_t b = 4, r = 4;
    for (int i = 0; i < n; ++i) {
        const uint64_t N = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        b += 24 + 8 * (max_pairs && max_pairs[i] < N ? (uint64_t)max_pairs[i] : N);
        r += 24 + 8 * N;
    }
    *base_bytes = b;
    *rest_bytes = r;
    return WC_OK;
}

extern "C" uint64_t wc_merge_bound(const wc_unit* units, int n) {
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) b += 24 + 8 * (uint64_t)units[i].nx * units[i].ny * units[i].nz;
    return b;
}
