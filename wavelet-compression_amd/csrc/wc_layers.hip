// wc_layers.hip — the merge of progressive layers in the compressed domain
// (wc_merge in include/wavelet_amd.h): two payloads of one unit with disjoint
// positions become their union.  The split that makes such layers
// (wc_split_budget, wc_split_thresh) is the pair selection of wc_thin.hip.  No
// cell and no dense coefficient exists anywhere: the work follows the pairs.
//
// Not part of the reference's codec.  Positions come from the decoders' pair-tile
// scan (wc_thinunit.h tile_positions); the unit view and the header writer are
// wc_thinunit.h's too.
//
// Passes (one stream, nothing read back; tiles = the plan's decode tiles):
//   k_merge_scan        grid y = side (a, b): the positions of a side's pairs below N
//                       into its position row, and their count (they are a prefix of
//                       the pairs: positions strictly increase).  A unit runs only if
//                       BOTH headers agree with it.
//   k_merge_place       grid y = side: pair k of this side at position p has rank
//                       r = #(positions of the other side below p), by a lower-bound
//                       search in the other row; output index k + r; run = p - 1 -
//                       max(own predecessor, other row's entry r - 1).  The search is
//                       bounded per tile: one search (the same in every lane) for the
//                       tile's first position gives lo, and since positions are distinct
//                       integers r <= lo + (p - first): each lane searches [lo, that].
//                       Side a raises the unit's overlap word where the other row holds p.
//   k_merge_units       per unit: header, pair count, offsets; kErrHeader / kErrOverlap
// Which tiles run: T = min(pair tiles of the payload, ceil(N / kFlatTile)), per
// input, as in wc_thin.hip: a tile t >= T holds only pairs at or past N, its blocks
// leave after the header, before any atomic.  A tile t < T always publishes.  The
// look-back is lookback_sum's with its derive path: no wait depends on which
// workgroups are resident.  k_merge_place waits for nothing.
//
// Scratch (wc_ctx::merge): two position rows, 8 B per coefficient in whole tiles.
//
// Bounds: a position entry is written for a pair k < n of a tile t < T whose
// position is below N (so k < N); an output pair is written at index
// < min(N, na' + nb') inside the slot of 24 + 8 N bytes; the searches read entries
// [0, count) of a row only.  A negative run counts as run 0 (Sat32;
// kErrNegativeRun), so positions still grow.
#include "wc_thinunit.h"

namespace wc {

// Side s = blockIdx.y of unit u: its positions below N and their count.
__global__ __launch_bounds__(kThreads) void k_merge_scan(MergeLaunch a) {
    using Scan = ThinScan;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = (int)blockIdx.y;
    const FTile ft = a.tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const ThinDesc C = a.desc[u];
    const ThinUnit U = thin_open(C, a.pay[s], a.off[s][u]);
    const ThinUnit O = thin_open(C, a.pay[1 - s], a.off[1 - s][u]);
    if (!U.ok || !O.ok || ft.index >= U.T) return;  // uniform; before any atomic
    const uint32_t t = Scan::tile_index(ft.index, U.T, a.ordered, a.ticket[s] + u, s_x);
    TilePos tp;
    tile_positions(U, t, a.status[s] + C.dt_begin, a.err, s_w, s_x, w, l, tp);

    uint32_t* __restrict__ row = a.pos[s] + (size_t)C.dt_begin * kFlatTile;
    uint32_t live = 0u;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = tp.kw + r * 64 + l;
        const uint64_t p64 = tp.base + tp.incl[r] - 1u;
        const bool in = k < U.n && p64 < (uint64_t)C.N;  // then k <= p64 < N: inside the unit's row
        if (in) row[k] = (uint32_t)p64;
        live += (uint32_t)__popcll(__ballot(in));
    }
    if (l == 0 && live) atomicAdd(a.live + (size_t)s * a.n + u, live);
}

// entries [lo, hi) of row are sorted: the first index in [lo, hi] whose entry is >= p (hi: none)
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ row, uint32_t lo, uint32_t hi, uint32_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (row[mid] < p)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// Tile ft.index of side s = blockIdx.y: its live pairs to their places in the output.
__global__ __launch_bounds__(kThreads) void k_merge_place(MergeLaunch a) {
    const int s = (int)blockIdx.y;
    const FTile ft = a.tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const uint32_t nm = a.live[(size_t)s * a.n + u], no = a.live[(size_t)(1 - s) * a.n + u];
    const uint32_t k0 = ft.index * (uint32_t)kFlatTile;
    if (k0 >= nm) return;  // uniform (a refused unit: both counts are 0)
    const ThinDesc C = a.desc[u];
    const uint32_t* __restrict__ mine = a.pos[s] + (size_t)C.dt_begin * kFlatTile;
    const uint32_t* __restrict__ other = a.pos[1 - s] + (size_t)C.dt_begin * kFlatTile;
    const uint32_t* __restrict__ runs = reinterpret_cast<const uint32_t*>(a.pay[s] + a.off[s][u] + 20);
    uint2* __restrict__ pairs = reinterpret_cast<uint2*>(a.out + C.out_off + 20);
    const uint32_t lim = (uint32_t)min((uint64_t)C.N, (uint64_t)nm + no);
    const uint32_t first = mine[k0];
    const uint32_t lo = lower_bound(other, 0u, no, first);  // the same in every lane
    for (int i = 0; i < kFlatPerThread; ++i) {
        const uint32_t k = k0 + i * kThreads + threadIdx.x;
        if (k >= nm) break;
        const uint32_t p = mine[k];
        const uint32_t r = lower_bound(other, lo, (uint32_t)min((uint64_t)no, (uint64_t)lo + (p - first)), p);
        if (s == 0 && r < no && other[r] == p) atomicOr(a.overlap + u, 1u);
        const uint32_t qm = k ? mine[k - 1] + 1u : 0u, qo = r ? other[r - 1] + 1u : 0u;  // predecessor + 1; none: 0
        const uint32_t idx = k + r;
        if (idx >= lim) continue;  // only with an overlap
        pairs[idx] = make_uint2(p - max(qm, qo), runs[2 * (size_t)k + 1]);
    }
}

// Thread u: unit u's header, pair count and offset.  A header that disagrees: slot untouched, kErrHeader;
// an overlap: a header with 0 pairs, kErrOverlap.
__global__ __launch_bounds__(kThreads) void k_merge_units(MergeLaunch a) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= a.n) return;
    const ThinDesc C = a.desc[u];
    const bool ok = thin_open(C, a.pay[0], a.off[0][u]).ok && thin_open(C, a.pay[1], a.off[1][u]).ok;
    const bool ov = ok && a.overlap[u] != 0u;
    const uint32_t k =
        ok && !ov ? (uint32_t)min((uint64_t)C.N, (uint64_t)a.live[u] + a.live[(size_t)a.n + u]) : 0u;
    if (ok) write_header(a.out + C.out_off, C, k);
    if (!ok) atomicOr(a.err, kErrHeader);
    if (ov) atomicOr(a.err, kErrOverlap);
    a.pairs[u] = k;
    a.out_offsets[u] = C.out_off;
    if (u == a.n - 1) a.out_offsets[a.n] = C.out_off + 20 + 8ull * k;
}

hipError_t launch_merge(hipStream_t st, const MergeLaunch& a) {
    if (a.n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.ntiles) {
        k_merge_scan<<<dim3(a.ntiles, 2), kThreads, 0, st>>>(a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_merge_place<<<dim3(a.ntiles, 2), kThreads, 0, st>>>(a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    k_merge_units<<<((uint32_t)a.n + kThreads - 1) / kThreads, kThreads, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace wc
