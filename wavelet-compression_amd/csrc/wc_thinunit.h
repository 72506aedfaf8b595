// wc_thinunit.h — a unit's standard payload as the passes over its pairs see it
// (wc_thin.hip's pair selection, wc_layers.hip's merge): the pairs, their count
// and the pair tiles that run, from the header alone (thin_open); the positions
// of one pair tile's pairs (tile_positions); the 20-byte header of an output
// (write_header).  Internal: not installed.
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

// The positions of one pair tile: the lane's pairs, the in-wave sums and the tile's
// prefix; pair k = kw + r * 64 + l of round r sits at base + incl[r] - 1.
struct TilePos {
    uint32_t kw;
    uint64_t base;
    uint2 q[ThinScan::kRounds];
    uint32_t incl[ThinScan::kRounds];
};
__device__ __forceinline__ void tile_positions(const ThinUnit& U, uint32_t t, unsigned long long* st,
                                               uint32_t* __restrict__ err, ThinScan::T* s_w, ThinScan::V* s_x, int w,
                                               int l, TilePos& o) {
    using Scan = ThinScan;
    PayloadRuns src;
    src.runs = U.runs;
    o.kw = Scan::wave_first(t, w);
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) o.q[r] = Scan::load(U.runs, o.kw + r * 64 + l, U.n);
    Scan::WaveSums ws;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) o.incl[r] = ws.round(o.q[r], o.kw + r * 64 + l, U.n);
    const Scan::Prefix P = Scan::prefix(ws.finish(err), t, U.n, src, st, Granule62{}, err, s_w, s_x, w, l);
    o.base = (uint64_t)P.excl + P.wexcl;
}

// The header of an output payload of the unit with `pairs` pairs.
__device__ __forceinline__ void write_header(uint8_t* __restrict__ slot, const ThinDesc& C, uint32_t pairs) {
    int32_t* h = reinterpret_cast<int32_t*>(slot);
    h[0] = C.W;
    h[1] = C.H;
    h[2] = C.D;
    h[3] = C.want;
    h[4] = (int32_t)pairs;
}

}  // namespace wc
