// wc_packfmt.h — what the host rule (wc_packrule.cpp, plain C++) and the device
// transcoders (wc_pack.hip) share of the packed payload format
// (include/wavelet_amd.h "Opt-in packed payloads"): the value rule q, the
// header check and the slot size.  Integers only, so both sides give the same
// bits.  No HIP include: the host rule is built without one.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define WC_PACK_HD __host__ __device__ inline
#else
#define WC_PACK_HD inline
#endif

namespace wc {

constexpr int kPackMaxLevels = 4;  // WC_MAX_LEVELS (checked in wc_packrule.cpp's users by the tag range -33..-68)

// q: the value's bits rounded to nearest even at vbytes bytes.  A carry into the
// exponent is wanted; a finite value stays finite (the truncation where the
// rounding would reach inf), a NaN stays a NaN (quiet bit set), inf is unchanged.
WC_PACK_HD uint32_t pack_value(uint32_t b, int vbytes) {
    if (vbytes < 2 || vbytes > 3) return b;
    const int s = 8 * (4 - vbytes);
    const uint32_t low = (1u << s) - 1u, m = b & 0x7FFFFFFFu, sign = b & 0x80000000u;
    if (m > 0x7F800000u) return (b | 0x00400000u) & ~low;
    if (m == 0x7F800000u) return b;
    uint32_t r = (m + (1u << (s - 1)) - 1u + ((m >> s) & 1u)) & ~low;
    if (r >= 0x7F800000u) r = m & ~low;
    return sign | r;
}

// The header's fourth field against the box: the standard header (W*H*D: L = 1,
// V = 0), the multi-level header (-L, L = 2..4: V = 0) or a packed tag
// (-(16 V + L), V = 2..4, L = 1..4).  For L >= 2 on a box with cells 2^L divides
// every dimension, as wc_payload_levels asks.
WC_PACK_HD bool pack_header(int32_t W, int32_t H, int32_t D, int32_t tag, int& L, int& V) {
    if (W < 0 || H < 0 || D < 0) return false;
    const uint64_t wh = (uint64_t)W * (uint64_t)H;  // below 2^62; three factors could wrap (2^30 * 2^30 * 16 = 2^64)
    if (D && wh > 0x7FFFFFFFull) return false;
    const uint64_t cells = wh * (uint64_t)D;
    if (cells > 0x7FFFFFFFull) return false;
    if (tag >= 0) {
        L = 1;
        V = 0;
        return (uint64_t)tag == cells;
    }
    if (tag < -(16 * 4 + kPackMaxLevels)) return false;
    const int t = -(int)tag;
    if (tag >= -kPackMaxLevels) {
        if (tag > -2) return false;
        L = t;
        V = 0;
    } else {
        if (tag > -(16 * 2 + 1)) return false;
        L = t & 15;
        V = t >> 4;
        if (L < 1 || L > kPackMaxLevels) return false;
    }
    return L < 2 || !cells || ((W | H | D) & ((1 << L) - 1)) == 0;
}

// The worst-case packed unit of N cells, S(N), and its slot stride pad8(S + 4).
WC_PACK_HD uint64_t pack_worst(uint64_t N, int vbytes) {
    return 20 + (((N + 63) / 64 + 7) & ~uint64_t(7)) + 31 * ((N + 7) / 8) + (uint64_t)vbytes * N;
}
WC_PACK_HD uint64_t pack_slot(uint64_t N, int vbytes) { return (pack_worst(N, vbytes) + 4 + 7) & ~uint64_t(7); }

}  // namespace wc
