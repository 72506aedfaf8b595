// wc_regionmap.h — the index map of the sub-box decode (include/wavelet_amd.h
// "Opt-in sub-box decode"), one statement for the kernel (wc_region.hip), the
// host (wc_capi.cpp) and the stand-alone sanitizer program
// (tests/cpp/test_regionrule.cpp).  Plain C++: no HIP header is needed.
//
// All quantities are "primed": the unit after the corner filter of a reduction
// r, n = (W, H, D) >> r with L' = L - r levels, and the region's origin o and
// extent s in cells of that resolution (2^L' divides every n, o and s).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define WC_RMAP_FN __host__ __device__ __forceinline__
#else
#define WC_RMAP_FN inline
#endif

namespace wc {

constexpr uint32_t kRegionOut = 0xffffffffu;  // region_axis: the coordinate is not needed

// lvl of the pair at (I, J, K) inside the primed box (w, h, d): 0 for L' = 0,
// else j* + 1 with j* the largest j < L' whose box (w, h, d) >> j holds the
// pair.  The boxes are nested, so j* is the count of the j >= 1 that hold.
WC_RMAP_FN uint32_t region_level(uint32_t I, uint32_t J, uint32_t K, uint32_t w, uint32_t h, uint32_t d, uint32_t L) {
    if (L == 0u) return 0u;
    uint32_t lvl = 1u;  // j = 1..3: WC_MAX_LEVELS is 4
    lvl += (1u < L && I < (w >> 1) && J < (h >> 1) && K < (d >> 1)) ? 1u : 0u;
    lvl += (2u < L && I < (w >> 2) && J < (h >> 2) && K < (d >> 2)) ? 1u : 0u;
    lvl += (3u < L && I < (w >> 3) && J < (h >> 3) && K < (d >> 3)) ? 1u : 0u;
    return lvl;
}

// One axis: coordinate c (< n) of a pair of level lvl -> its index in the
// compact s-unit, or kRegionOut.  The low half of level lvl keeps the cells
// [o >> lvl, (o + s) >> lvl), the high half the same range behind n >> lvl;
// in the compact unit the high half starts at s >> lvl.  The difference wraps
// to >= 2^31 below the range, which the one unsigned compare rejects.  A kept
// index is < 2 * (s >> lvl) <= s for lvl >= 1 and < s for lvl = 0.
WC_RMAP_FN uint32_t region_axis(uint32_t c, uint32_t n, uint32_t o, uint32_t s, uint32_t lvl) {
    const uint32_t nl = n >> lvl, sl = s >> lvl;
    const bool high = lvl >= 1u && c >= nl;
    const uint32_t q = c - (high ? nl : 0u) - (o >> lvl);
    return q < sl ? q + (high ? sl : 0u) : kRegionOut;
}

// The largest needed coordinate of one axis (s >= 1): the last high coefficient
// of level 1, or the last cell for L' = 0.
WC_RMAP_FN uint32_t region_last(uint32_t n, uint32_t o, uint32_t s, uint32_t L) {
    return L >= 1u ? (n >> 1) + (o >> 1) + (s >> 1) - 1u : o + s - 1u;
}

// end: one past the flat position (I*H + J)*D + K of the largest needed
// (I, J, K); 0 for a region without cells.  H, D: the payload's full box.
WC_RMAP_FN uint64_t region_end(uint32_t w, uint32_t h, uint32_t d, uint32_t L, uint32_t ox, uint32_t oy, uint32_t oz,
                               uint32_t sx, uint32_t sy, uint32_t sz, uint32_t H, uint32_t D) {
    if (sx == 0u || sy == 0u || sz == 0u) return 0u;
    return ((uint64_t)region_last(w, ox, sx, L) * H + region_last(h, oy, sy, L)) * D + region_last(d, oz, sz, L) + 1u;
}

}  // namespace wc
