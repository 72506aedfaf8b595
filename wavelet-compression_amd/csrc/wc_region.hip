// wc_region.hip — region decode of the sub-box inverse (wc_inverse_region in
// include/wavelet_amd.h).
//
// Not part of the reference's codec.  The transform is Haar on every level: a
// synthesis step writes cells 2m and 2m + 1 of a line from the low and the high
// coefficient m of that line alone.  A region aligned to 2^L therefore needs,
// on every level lvl, the coefficients m in [o >> lvl, (o + s) >> lvl) of the
// low and of the high half of each axis and nothing else, and those, put side
// by side, are the flat array of an s_x x s_y x s_z unit with the same levels
// (wc_regionmap.h states the map; the reduction r of wc_inverse_coarse comes
// first, as its corner filter).  k_decode_region turns a payload's pairs into
// that compact unit in the coefficient scratch, at the place the plan of the
// derived units gives it; k_level<false>, k_level_copy, k_inverse{,_fast} and
// k_corner_box (wc_coarse.hip, for L' = 0) then run unchanged on the derived
// units.  Nothing of size W*H*D is written or read.
//
// The kernel is k_decode_corner (wc_coarse.hip) through its step 2: the shared
// pair-tile scan (wc_pairscan.h PairScan, which owns the rule for which tiles
// run and why no look-back waits on a tile that has left) over zeroed 62-bit
// granules, Sat32 sums (every position acted on is below end <= W*H*D < 2^31;
// a negative run counts as run 0 and raises kErrNegativeRun, so pair k lands at
// a position >= k).  The unit's tiles are [0, T), T = min(pair tiles of the
// payload, ceil(end / kFlatTile)): a tile t >= T holds only pairs at or past
// end and leaves before any atomic, so a tile t < T reads only granules of
// tiles below t, all of which run.  A tile t < T whose exclusive prefix turns
// out >= end has published its inclusive sum by then and skips the scatter.
// A unit whose region has no cells (end = 0) reads nothing, its header included.
//
// The scatter's 4-B stores stay side by side along K inside a band, as the
// corner decode's do (DESIGN.md "r = L" records what Box3D order cost there).
//
// Bounds: a pair is stored only if its position p < end <= W*H*D, its
// (I, J, K) from p lies inside the primed box and region_axis keeps it on all
// three axes; a kept axis index is < s of that axis (wc_regionmap.h), so every
// store is inside the unit's s_x*s_y*s_z elements at dst_off, whatever the
// payload holds.  Pair loads are bounded by the header's pair count, as in
// k_decode.
#include "wc_pairscan.h"
#include "wc_regionmap.h"

namespace wc {

// tiles: the decode tiles of the plan of the FULL units, the prefix below the
// batch's largest ceil(end / kFlatTile).  bad[u] (written by the first tile of
// a unit whose region has cells, read by the later launches, which have tiles
// only for such units): kUnitRefused = the header disagrees (kErrHeader;
// nothing past the header is read, no cell is written); kUnitBox = L' = 0
// (k_corner_box writes the cells); kUnitRun otherwise.
__global__ __launch_bounds__(kThreads) void k_decode_region(const RegionDesc* __restrict__ desc,
                                                          const FTile* __restrict__ tiles,
                                                          const uint8_t* __restrict__ payload,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ ticket,
                                                          unsigned long long* __restrict__ status,
                                                          float* __restrict__ compact,
                                                          uint32_t* __restrict__ err, int ordered,
                                                          uint32_t* __restrict__ bad) {
    using Scan = PairScan<Sat32, Granule62, kFlatTile, LoadPairs>;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const RegionDesc C = desc[u];
    if (C.end == 0u) return;  // uniform: nothing of the unit is needed
    const uint8_t* ph = payload + offsets[u];
    int32_t nrle;
    const bool hok = header_ok(C.W, C.H, C.D, C.want, ph, nrle);
    if (ft.index == 0 && tid == 0) {
        bad[u] = !hok ? kUnitRefused : C.direct ? kUnitBox : kUnitRun;
        if (!hok) atomicOr(err, kErrHeader);
    }
    if (!hok) return;  // uniform
    const uint32_t n = (uint32_t)nrle;
    const uint32_t ptiles = n ? (n - 1u) / (uint32_t)kFlatTile + 1u : 1u;
    const uint32_t T = min(ptiles, (C.end - 1u) / (uint32_t)kFlatTile + 1u);
    if (ft.index >= T) return;  // uniform; before any atomic
    const uint32_t t = Scan::tile_index(ft.index, T, ordered, ticket + u, s_x);

    // 1. this lane's pairs and the saturating in-wave inclusive sums of (run + 1);
    // 2. the sum over the unit's earlier tiles
    const uint32_t* __restrict__ runs = reinterpret_cast<const uint32_t*>(ph + 20);
    const uint32_t kw = Scan::wave_first(t, w);
    uint2 q[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) q[r] = Scan::load(runs, kw + r * 64 + l, n);
    uint32_t incl[Scan::kRounds];
    Scan::WaveSums ws;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) incl[r] = ws.round(q[r], kw + r * 64 + l, n);
    const Scan::Prefix P = Scan::prefix(ws.finish(err), t, n, runs, status + C.dt_begin, Granule62{}, err, s_w, s_x, w, l);
    const uint64_t A = P.excl;  // positions before this tile's first pair
    if (A >= (uint64_t)C.end) return;  // uniform: the whole tile is past the last needed pair (its sum is published)

    // 3. the pairs the region needs, to their places in the compact unit
    float* __restrict__ dst = compact + C.dst_off;
    const uint64_t base = A + P.wexcl;  // + incl[r] - 1: position of the lane's pair in round r
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        const uint64_t p64 = base + incl[r] - 1u;  // incl >= 1 where k < n
        if (k >= n || p64 >= (uint64_t)C.end) continue;
        const uint32_t p = (uint32_t)p64;  // < end <= W*H*D < 2^31
        const uint32_t row = div_rows(p, C.dmagic), K = p - row * (uint32_t)C.D;
        const uint32_t I = div_rows(row, C.hmagic), J = row - I * (uint32_t)C.H;
        if (I >= C.w || J >= C.h || K >= C.d) continue;  // the corner filter of the reduction
        const uint32_t lvl = region_level(I, J, K, C.w, C.h, C.d, C.L);
        const uint32_t ix = region_axis(I, C.w, C.ox, C.sx, lvl), iy = region_axis(J, C.h, C.oy, C.sy, lvl),
                       iz = region_axis(K, C.d, C.oz, C.sz, lvl);
        if ((int32_t)(ix | iy | iz) < 0) continue;  // kRegionOut on an axis (kept indices are < 2^31)
        dst[(ix * C.sy + iy) * C.sz + iz] = __uint_as_float(q[r].y);
    }
}

hipError_t launch_decode_region(hipStream_t st, const RegionDesc* desc, const FTile* dtiles, uint32_t ndt,
                                const uint8_t* payload, const uint64_t* offsets, uint32_t* ticket,
                                unsigned long long* status, float* compact, uint32_t* err, int ordered, uint32_t* bad) {
    if (ndt)
        k_decode_region<<<ndt, kThreads, 0, st>>>(desc, dtiles, payload, offsets, ticket, status, compact, err, ordered,
                                                  bad);
    return hipGetLastError();
}

}  // namespace wc
