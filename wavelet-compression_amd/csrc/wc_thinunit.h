// wc_thinunit.h — a unit's standard payload as the passes over its pairs see it
// (wc_thin.hip, wc_layers.hip): the pairs, their count and the pair tiles that run,
// from the header alone.  The code is wc_thin.hip's, moved here unchanged.
// Internal: not installed.
#pragma once

#include "wc_pairscan.h"

namespace wc {

// A unit's payload as every pass sees it, from the header alone.
struct ThinUnit {
    const uint32_t* __restrict__ runs;  // the pairs
    uint32_t n;                         // pairs the header announces
    uint32_t T;                         // pair tiles that run
    uint32_t np;                        // pairs with a scratch entry: min(n, T * kFlatTile)
    bool ok;                            // the header agrees with the unit
};
__device__ __forceinline__ ThinUnit thin_open(const ThinDesc& C, const uint8_t* __restrict__ payload, uint64_t off) {
    ThinUnit U{nullptr, 0u, 0u, 0u, false};
    if (off & 3u) return U;
    const uint8_t* ph = payload + off;
    int32_t nrle;
    U.ok = header_ok(C.W, C.H, C.D, C.want, ph, nrle);
    if (!U.ok) return U;
    U.runs = reinterpret_cast<const uint32_t*>(ph + 20);
    U.n = (uint32_t)nrle;
    const uint32_t ptiles = U.n ? (U.n - 1u) / (uint32_t)kFlatTile + 1u : 1u;
    U.T = C.N ? min(ptiles, (C.N - 1u) / (uint32_t)kFlatTile + 1u) : 0u;
    U.np = (uint32_t)min((uint64_t)U.n, (uint64_t)U.T * kFlatTile);
    return U;
}

using ThinScan = PairScan<Sat32, Granule62, kFlatTile, LoadPairs>;

}  // namespace wc
