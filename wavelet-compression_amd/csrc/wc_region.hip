// wc_region.hip — the decode of the reduced-resolution inverse and of the
// sub-box inverse (wc_inverse_coarse and wc_inverse_region in
// include/wavelet_amd.h).
//
// Not part of the reference's codec.  A unit W x H x D with L levels and a
// reduction r needs only the low-pass corner (w, h, d) = (W, H, D) >> r of its
// flat array A (x-slowest order (I*H + J)*D + K): the synthesis of level l
// touches only the corner (W, H, D) >> (l - 1), so levels L..r+1 act on that
// corner exactly as levels L' = L-r..1 act on a w x h x d unit (the primed
// unit).  And the transform is Haar on every level: a synthesis step writes
// cells 2m and 2m + 1 of a line from the low and the high coefficient m of that
// line alone.  A region of the primed unit aligned to 2^L' therefore needs, on
// every level lvl, the coefficients m in [o >> lvl, (o + s) >> lvl) of the low
// and of the high half of each axis and nothing else, and those, put side by
// side, are the flat array of an s_x x s_y x s_z unit with the same levels
// (wc_regionmap.h states the map).  k_decode_region turns a payload's pairs
// into that compact unit C[(ix*s_y + iy)*s_z + iz] in the coefficient scratch,
// at the place the plan of the derived units (s_x, s_y, s_z) gives it;
// k_level<false>, k_level_copy and k_inverse{,_fast} then run unchanged on the
// derived units.  A unit with r == L has nothing left to run: its compact unit
// IS the result, and k_corner_box copies it to its Box3D place
// out[I + s_x*(J + s_y*K)].  Nothing of size W*H*D is written or read.
//
//   k_decode_region<kWhole>  pair tiles -> the compact unit's coefficients
//                    (scattered 4-B stores, neighbours in K side by side inside
//                    a band; the zeros between them come from a memset of the
//                    compact scratch before).  kWhole (wc_inverse_coarse): the
//                    region is the whole primed box, the map is the identity and
//                    is not called: it is stated for even dimensions, and a
//                    coarse batch may hold an odd unit at L = 1, r = 0.
//   k_corner_box     units with r == L: compact unit -> Box3D cells, 32 x 32
//                    (I, K) tiles through LDS so that both sides move whole
//                    rows.  (Scattering the pairs straight into Box3D order
//                    was measured first: neighbouring K are w*h cells apart
//                    there, one store per cache line, and the decode of the
//                    one-level C2 payloads took 0.55 ms against 0.17 ms into
//                    the compact order; DESIGN.md "r = L".)
//
// k_decode_region runs the decoders' shared pair-tile scan (wc_pairscan.h
// PairScan, which also owns the rule for which tiles run and why no look-back
// waits on a tile that has left) over zeroed 62-bit granules.  Sums are Sat32,
// as in k_rowindex: every position this kernel acts on is below end <= W*H*D <
// 2^31, and a saturated sum is past it like the exact one; a negative run counts
// as run 0 (and raises kErrNegativeRun), so pair k lands at a position >= k.
// The unit's tiles are [0, T), T = min(pair tiles of the payload, ceil(end /
// kFlatTile)): a tile t >= T holds only pairs at or past end and leaves before
// any atomic, so a tile t < T reads only granules of tiles below t, all of which
// run.  A tile t < T whose exclusive prefix turns out >= end has published its
// inclusive sum by then and skips the scatter.  A unit whose region has no cells
// (end = 0) reads nothing, its header included.
//
// Bounds: a pair is stored only if its position p < end <= W*H*D and its
// (I, J, K) from p lies inside the primed box (w, h, d).  kWhole: s = (w, h, d),
// so the store is inside the unit's s_x*s_y*s_z elements at dst_off.  Otherwise
// region_axis must also keep the pair on all three axes, and a kept axis index
// is < s of that axis (wc_regionmap.h).  Either way every store is inside the
// compact unit, whatever the payload holds; pair loads are bounded by the
// header's pair count, as in k_decode.
#include "wc_packsrc.h"
#include "wc_pairscan.h"
#include "wc_regionmap.h"

namespace wc {

// tiles: the decode tiles of the plan of the FULL units (interleaved by tile
// index across units; a prefix of that list: every tile index below the
// batch's largest ceil(end / kFlatTile)).  bad[u] (written by the first tile of
// a unit whose region has cells, read by the later launches, which have tiles
// only for such units): kUnitRefused = the header disagrees (kErrHeader;
// nothing past the header is read, no cell is written, every later launch skips
// the unit); kUnitBox = r == L (k_corner_box writes the cells, the level passes
// and the inverse skip the unit); kUnitRun otherwise.
// Src: the pairs' source, a standard payload at payload + offsets[u]
// (PayloadPairs) or a packed unit there (PackedPairs, wc_packsrc.h: payload is
// then the packed buffer and its capacity; wc_inverse_packed_coarse / _region).
template <bool kWhole, class Src = PayloadPairs>
__global__ __launch_bounds__(kThreads) void k_decode_region(const RegionDesc* __restrict__ desc,
                                                          const FTile* __restrict__ tiles,
                                                          typename Src::Arg payload,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ ticket,
                                                          unsigned long long* __restrict__ status,
                                                          float* __restrict__ compact,
                                                          uint32_t* __restrict__ err, int ordered,
                                                          uint32_t* __restrict__ bad) {
    using Scan = PairScan<Sat32, Granule62, kFlatTile, LoadPairs>;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    typename Src::Lds* s_src = nullptr;
    if constexpr (Src::kLds) {
        __shared__ typename Src::Lds s_own;
        s_src = &s_own;
    }
    Src src(payload, err);
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const RegionDesc C = desc[u];
    // uniform: nothing of the unit is needed.  kWhole: never taken (a unit with tiles has cells), and said so:
    // without the hint the compiler lays the whole scan out around this exit, 4 % more code
    const bool none = C.end == 0u;
    // What the header check needs is loaded before the exit (the empty asm keeps the compiler from sinking the
    // loads below it): the payload's offset beside the descriptor, not one memory round trip after it in every
    // block, most of which are here only to find their tile at or past T.
    const uint64_t poff = offsets[u];
    asm volatile("" ::"s"(poff), "s"(C.W));
    if (kWhole ? __builtin_expect(none, false) : none) return;
    int32_t nrle;
    const bool hok = src.open(poff, C.W, C.H, C.D, C.want, nrle);
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
    src.enter(t, s_src, w, l);
    const uint32_t kw = Scan::wave_first(t, w);
    uint2 q[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) q[r] = src.fetch(r, kw + r * 64 + l, n, w, l);
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) q[r] = src.unpack(r, q[r], w, l);
    uint32_t incl[Scan::kRounds];
    Scan::WaveSums ws;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) incl[r] = ws.round(q[r], kw + r * 64 + l, src.lim(r, n));
    const Scan::Prefix P = Scan::prefix(ws.finish(err), t, n, src, status + C.dt_begin,
                                        Granule62{}, err, s_w, s_x, w, l);
    const uint64_t A = P.excl;  // positions before this tile's first pair
    if (A >= (uint64_t)C.end) return;  // uniform: the whole tile is past the last needed pair (its sum is published)

    // 3. the pairs the region needs, to their places in the compact unit
    float* __restrict__ dst = compact + C.dst_off;
    const uint64_t base = A + P.wexcl;  // + incl[r] - 1: position of the lane's pair in round r
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        const uint64_t p64 = base + incl[r] - 1u;  // incl >= 1 where k < n
        if (k >= src.lim(r, n) || p64 >= (uint64_t)C.end) continue;
        const uint32_t p = (uint32_t)p64;  // < end <= W*H*D < 2^31
        const uint32_t row = div_rows(p, C.dmagic), K = p - row * (uint32_t)C.D;
        const uint32_t I = div_rows(row, C.hmagic), J = row - I * (uint32_t)C.H;
        if (I >= C.w || J >= C.h || K >= C.d) continue;  // the corner filter of the reduction
        uint32_t ix = I, iy = J, iz = K;
        if constexpr (!kWhole) {
            const uint32_t lvl = region_level(I, J, K, C.w, C.h, C.d, C.L);
            ix = region_axis(I, C.w, C.ox, C.sx, lvl);
            iy = region_axis(J, C.h, C.oy, C.sy, lvl);
            iz = region_axis(K, C.d, C.oz, C.sz, lvl);
            if ((int32_t)(ix | iy | iz) < 0) continue;  // kRegionOut on an axis (kept indices are < 2^31)
        }
        dst[(ix * C.sy + iy) * C.sz + iz] = __uint_as_float(q[r].y);
    }
}

// tiles: the flat tiles (kFlatTile cells) of the plan of the DERIVED units:
// block (u, i) of a unit with r == L whose header agreed takes the unit's
// transposition tiles i, i + nft, ... (nft = the unit's flat tiles), a tile
// being 32 I x 32 K at one J: rows of K are contiguous in the compact unit,
// rows of I in the Box3D.  Every cell of the unit is written (the zeros of the
// cleared scratch included); a refused unit keeps its cells.
constexpr int kBoxTile = 32;
__global__ __launch_bounds__(kThreads) void k_corner_box(const RegionDesc* __restrict__ desc,
                                                       const FTile* __restrict__ tiles,
                                                       const float* __restrict__ compact, float* __restrict__ out,
                                                       const uint32_t* __restrict__ bad) {
    __shared__ float tile[kBoxTile][kBoxTile + 1];
    const FTile ft = tiles[blockIdx.x];
    if (bad[ft.unit] != kUnitBox) return;  // uniform
    const RegionDesc C = desc[ft.unit];
    const uint32_t w = C.sx, h = C.sy, d = C.sz;
    const uint32_t ti = (w + kBoxTile - 1) / kBoxTile, tk = (d + kBoxTile - 1) / kBoxTile;
    const uint32_t ntiles = h * ti * tk;
    const uint32_t nft = (w * h * d + (uint32_t)kFlatTile - 1) / (uint32_t)kFlatTile;
    const float* __restrict__ src = compact + C.dst_off;
    float* __restrict__ dst = out + C.out_off;
    const uint32_t a = threadIdx.x & (kBoxTile - 1), b0 = threadIdx.x / kBoxTile;  // 32 x 8 threads
    for (uint32_t t = ft.index; t < ntiles; t += nft) {  // uniform
        const uint32_t kt = t % tk, it = (t / tk) % ti, J = t / (tk * ti);
        const uint32_t I0 = it * kBoxTile, K0 = kt * kBoxTile;
#pragma unroll
        for (uint32_t b = b0; b < (uint32_t)kBoxTile; b += kThreads / kBoxTile) {
            const uint32_t I = I0 + b, K = K0 + a;
            if (I < w && K < d) tile[b][a] = src[(I * h + J) * d + K];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t b = b0; b < (uint32_t)kBoxTile; b += kThreads / kBoxTile) {
            const uint32_t I = I0 + a, K = K0 + b;
            if (I < w && K < d) dst[I + w * (J + h * K)] = tile[a][b];
        }
        __syncthreads();
    }
}

hipError_t launch_decode_region(hipStream_t st, const RegionDesc* desc, const FTile* dtiles, uint32_t ndt,
                                const uint8_t* payload, const uint64_t* offsets, uint32_t* ticket,
                                unsigned long long* status, float* compact, uint32_t* err, int ordered, uint32_t* bad,
                                bool whole, const uint64_t* packed_cap) {
    if (ndt && packed_cap)  // the payload is packed units, read below *packed_cap
        (whole ? k_decode_region<true, PackedPairs> : k_decode_region<false, PackedPairs>)<<<ndt, kThreads, 0, st>>>(
            desc, dtiles, PackedPairs::Arg{payload, *packed_cap}, offsets, ticket, status, compact, err, ordered, bad);
    else if (ndt)
        (whole ? k_decode_region<true> : k_decode_region<false>)<<<ndt, kThreads, 0, st>>>(
            desc, dtiles, payload, offsets, ticket, status, compact, err, ordered, bad);
    return hipGetLastError();
}

hipError_t launch_corner_box(hipStream_t st, const RegionDesc* desc, const FTile* ftiles, uint32_t nft,
                             const float* compact, float* out, const uint32_t* bad) {
    if (nft) k_corner_box<<<nft, kThreads, 0, st>>>(desc, ftiles, compact, out, bad);
    return hipGetLastError();
}

}  // namespace wc
