// wc_layers.hip — progressive layers in the compressed domain (wc_split_budget,
// wc_split_thresh and wc_merge in include/wavelet_amd.h): a standard payload P
// becomes (base, rest), base the thinning of P and rest its complement inside the
// canonical form of P; two payloads with disjoint positions become their union.
// No cell and no dense coefficient exists anywhere: the work follows the pairs.
//
// Not part of the reference's codec.  Positions come from the decoders' pair-tile
// scan (wc_pairscan.h PairScan<Sat32, Granule62, kFlatTile, LoadPairs>), the
// budget form's keys and select are the thinning's own launches
// (wc_thin.hip launch_thin_front), the unit view is wc_thinunit.h's.
//
// Split, passes (one stream, nothing read back; tiles = the plan's decode tiles):
//   launch_thin_front   budget form: {key, pos} per pair (key = bg_key of a
//                       candidate below N, else 0) and the radix select: T per unit.
//                       Base: key > T; rest: 0 < key <= T.
//   k_split_tscan       threshold form: key 2 where |c| > t_lvl, 1 for any other
//                       candidate below N, 0 otherwise; T = 1 for every unit
//   k_split_compact     per pair tile, both outputs at once: the look-back carries
//                       the pair (base count, rest count) as one 62-bit granule,
//                       base in bits 0-30 and rest in bits 31-61.  Both are sums of
//                       counts below 2^31, so neither field carries into the other and
//                       lookback_sum's algebra holds; the derive path counts both from
//                       the tile's own scratch row.  A kept pair's value goes to its
//                       slot, its position to the output's position row.
//   k_split_diff        grid y = output: run_k' = pos_k' - pos_{k'-1} - 1 (pos_{-1} = -1)
//   k_split_units       per unit: both headers, counts and offsets; the header check
// Merge, passes:
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
// leave after the header, before any atomic.  A tile t < T always publishes.  Both
// look-backs are lookback_sum's with its derive path: no wait depends on which
// workgroups are resident.  k_merge_place and the difference pass wait for nothing.
//
// Scratch: split = the thinning's 12 B per coefficient (wc_ctx::thin) plus 4 B for
// the rest's positions, 16 B x kFlatTile x ceil(N / kFlatTile) per unit; merge = two
// position rows, 8 B per coefficient in whole tiles.
//
// Bounds.  Split: a scratch entry is written for pair k < n of a tile t < T <= the
// unit's plan tiles; a base pair at k' < cap, a rest pair at k' < N, inside slots
// of 24 + 8 cap and 24 + 8 N bytes.  Merge: a position entry is written for a pair
// k < n of a tile t < T whose position is below N (so k < N); an output pair is
// written at index < min(N, na' + nb') inside the slot of 24 + 8 N bytes; the
// searches read entries [0, count) of a row only.  A negative run counts as run 0
// (Sat32; kErrNegativeRun), so positions still grow.
#include "wc_budget.h"
#include "wc_pairscan.h"
#include "wc_thinunit.h"

namespace wc {

hipError_t launch_thin_front(hipStream_t, const ThinLaunch&);  // wc_thin.hip

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

// ---- split ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_split_tscan(const ThinDesc* __restrict__ desc,
                                                        const FTile* __restrict__ tiles,
                                                        const uint8_t* __restrict__ payload,
                                                        const uint64_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ ticket,
                                                        unsigned long long* __restrict__ status,
                                                        uint2* __restrict__ s1, uint32_t* __restrict__ err,
                                                        int ordered) {
    using Scan = ThinScan;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    if (!U.ok || ft.index >= U.T) return;  // uniform; before any atomic
    const uint32_t t = Scan::tile_index(ft.index, U.T, ordered, ticket + u, s_x);
    TilePos tp;
    tile_positions(U, t, status + C.dt_begin, err, s_w, s_x, w, l, tp);

    const LtGeom G{C.dmagic, C.hmagic, (uint32_t)C.W, (uint32_t)C.H, (uint32_t)C.D, (int)C.L};
    uint2* __restrict__ row = s1 + (size_t)C.dt_begin * kFlatTile;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = tp.kw + r * 64 + l;
        if (k >= U.n) continue;
        const uint64_t p64 = tp.base + tp.incl[r] - 1u;  // incl >= 1 where k < n
        uint2 e = make_uint2(0u, 0xffffffffu);
        if (p64 < (uint64_t)C.N) {
            const uint32_t p = (uint32_t)p64;
            const uint32_t m = tp.q[r].y & 0x7fffffffu;
            const uint32_t lv = (lt_levels4(G, p & ~3u) >> (2u * (p & 3u))) & 3u;
            const float th = lv == 0u ? C.th[0] : lv == 1u ? C.th[1] : lv == 2u ? C.th[2] : C.th[3];
            e.y = p;
            e.x = !bg_candidate(m) ? 0u : __uint_as_float(m) > th ? 2u : 1u;
        }
        row[k] = e;
    }
}

using CountScan = PairScan<Exact64, Granule62, kFlatTile, LoadPairs>;  // its prefix alone: the packed counts
constexpr int kRestShift = 31;
constexpr uint64_t kCountMask = (1ull << kRestShift) - 1;

// The look-back's derive path: (base, rest) counts of tile j of the unit's n pairs from its scratch row.
struct SplitCounts {
    const uint2* __restrict__ row;
    uint32_t Tk;
    template <class S, int TILE>
    __device__ __forceinline__ typename S::T tile_sum(int64_t j, typename S::K n, int l) const {
        using K = typename S::K;
        const K k0 = (K)j * TILE, k1 = min(k0 + (K)TILE, n);
        typename S::T a = 0;
        for (K k = k0 + (K)l; k < k1; k += 64) {
            const uint32_t key = row[k].x;
            a += key > Tk ? 1ull : key ? 1ull << kRestShift : 0ull;
        }
        return S::last(S::wave_incl(a));
    }
};

__global__ __launch_bounds__(kThreads) void k_split_compact(const ThinDesc* __restrict__ desc,
                                                          const uint64_t* __restrict__ rest_off,
                                                          const FTile* __restrict__ tiles,
                                                          const uint8_t* __restrict__ payload,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ ticket,
                                                          unsigned long long* __restrict__ status,
                                                          const uint2* __restrict__ s1, uint32_t* __restrict__ s2,
                                                          uint32_t* __restrict__ s3, const uint32_t* __restrict__ keyw,
                                                          uint8_t* __restrict__ out, uint8_t* __restrict__ rest,
                                                          uint32_t* __restrict__ keptw, uint32_t* __restrict__ restw,
                                                          uint32_t* __restrict__ err, int ordered) {
    using Scan = CountScan;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    if (!U.ok || ft.index >= U.T) return;  // uniform; before any atomic
    const uint32_t n = U.n;
    const uint32_t t = Scan::tile_index(ft.index, U.T, ordered, ticket + u, s_x);
    const SplitCounts src{s1 + (size_t)C.dt_begin * kFlatTile, keyw ? keyw[u] : 1u};

    const uint32_t kw = (uint32_t)Scan::wave_first(t, w);
    uint2 e[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        e[r] = k < n ? src.row[k] : make_uint2(0u, 0u);
    }
    // in the wave both counts fit one word: base in bits 0-15, rest in bits 16-31 (at most 1024 each)
    uint32_t incl[Scan::kRounds], wsum = 0u;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t s = wave_incl_sum32(e[r].x > src.Tk ? 1u : e[r].x ? 0x10000u : 0u);
        incl[r] = wsum + s;
        wsum += __builtin_amdgcn_readlane(s, 63);
    }
    const uint64_t wsum64 = (uint64_t)(wsum & 0xffffu) | ((uint64_t)(wsum >> 16) << kRestShift);
    const Scan::Prefix P = Scan::prefix(wsum64, t, (int64_t)n, src, status + C.dt_begin, Granule62{}, err, s_w, s_x, w, l);

    uint32_t* __restrict__ bpairs = reinterpret_cast<uint32_t*>(out + C.out_off + 20);
    uint32_t* __restrict__ rpairs = reinterpret_cast<uint32_t*>(rest + rest_off[u] + 20);
    uint32_t* __restrict__ row2 = s2 + (size_t)C.dt_begin * kFlatTile;
    uint32_t* __restrict__ row3 = s3 + (size_t)C.dt_begin * kFlatTile;
    const uint64_t before = P.excl + P.wexcl;  // neither field carries: each total is below 2^31
    const uint64_t bbase = before & kCountMask, rbase = before >> kRestShift;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        if (k >= n || !e[r].x) continue;
        const uint32_t val = U.runs[2 * (size_t)k + 1];
        if (e[r].x > src.Tk) {
            const uint64_t kp = bbase + (incl[r] & 0xffffu) - 1u;
            if (kp >= (uint64_t)C.cap) continue;  // never: kept <= cap by the rule; the slot's bound all the same
            bpairs[2 * kp + 1] = val;
            row2[kp] = e[r].y;
        } else {
            const uint64_t kp = rbase + (incl[r] >> 16) - 1u;
            if (kp >= (uint64_t)C.N) continue;  // never: a rest pair sits below N; the slot's bound all the same
            rpairs[2 * kp + 1] = val;
            row3[kp] = e[r].y;
        }
    }
    if (t == U.T - 1u && tid == 0) {
        const uint64_t all = P.excl + P.tot;
        keptw[u] = (uint32_t)min(all & kCountMask, (uint64_t)C.cap);
        restw[u] = (uint32_t)min(all >> kRestShift, (uint64_t)C.N);
    }
}

// Output tile ft.index of the unit's output blockIdx.y (0 base, 1 rest): the runs from the positions.
__global__ __launch_bounds__(kThreads) void k_split_diff(const ThinDesc* __restrict__ desc,
                                                       const uint64_t* __restrict__ rest_off,
                                                       const FTile* __restrict__ tiles,
                                                       const uint32_t* __restrict__ s2, const uint32_t* __restrict__ s3,
                                                       const uint32_t* __restrict__ keptw,
                                                       const uint32_t* __restrict__ restw, uint8_t* __restrict__ out,
                                                       uint8_t* __restrict__ rest) {
    const FTile ft = tiles[blockIdx.x];
    const bool second = blockIdx.y != 0;
    const uint32_t cnt = second ? restw[ft.unit] : keptw[ft.unit];
    const uint32_t k0 = ft.index * (uint32_t)kFlatTile;
    if (k0 >= cnt) return;  // uniform
    const ThinDesc C = desc[ft.unit];
    uint32_t* __restrict__ pairs =
        reinterpret_cast<uint32_t*>(second ? rest + rest_off[ft.unit] + 20 : out + C.out_off + 20);
    const uint32_t* __restrict__ row = (second ? s3 : s2) + (size_t)C.dt_begin * kFlatTile;
#pragma unroll
    for (int i = 0; i < kFlatPerThread; ++i) {
        const uint32_t kp = k0 + i * kThreads + threadIdx.x;
        if (kp >= cnt) continue;
        const uint32_t prev = kp ? row[kp - 1] : 0xffffffffu;  // pos_{-1} = -1
        pairs[2 * (size_t)kp] = row[kp] - prev - 1u;
    }
}

__device__ __forceinline__ void write_header(uint8_t* __restrict__ slot, const ThinDesc& C, uint32_t pairs) {
    int32_t* h = reinterpret_cast<int32_t*>(slot);
    h[0] = C.W;
    h[1] = C.H;
    h[2] = C.D;
    h[3] = C.want;
    h[4] = (int32_t)pairs;
}

// Thread u: unit u's two headers, counts and offsets; a unit whose header disagrees keeps both slots
// untouched (kErrHeader, counts 0).
__global__ __launch_bounds__(kThreads) void k_split_units(const ThinDesc* __restrict__ desc,
                                                        const uint64_t* __restrict__ rest_off, int n,
                                                        const uint8_t* __restrict__ payload,
                                                        const uint64_t* __restrict__ offsets,
                                                        const uint32_t* __restrict__ keptw,
                                                        const uint32_t* __restrict__ restw, uint8_t* __restrict__ out,
                                                        uint64_t* __restrict__ out_offsets, uint32_t* __restrict__ kept,
                                                        uint8_t* __restrict__ rest, uint64_t* __restrict__ rest_offsets,
                                                        uint32_t* __restrict__ rest_pairs, uint32_t* __restrict__ err) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= n) return;
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    const uint32_t kb = U.ok ? keptw[u] : 0u, kr = U.ok ? restw[u] : 0u;
    const uint64_t ro = rest_off[u];
    if (U.ok) {
        write_header(out + C.out_off, C, kb);
        write_header(rest + ro, C, kr);
    } else {
        atomicOr(err, kErrHeader);
    }
    kept[u] = kb;
    rest_pairs[u] = kr;
    out_offsets[u] = C.out_off;
    rest_offsets[u] = ro;
    if (u == n - 1) {
        out_offsets[n] = C.out_off + 20 + 8ull * kb;
        rest_offsets[n] = ro + 20 + 8ull * kr;
    }
}

hipError_t launch_split(hipStream_t st, const SplitLaunch& b) {
    const ThinLaunch& a = b.thin;
    if (a.n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.budget) {
        if ((e = launch_thin_front(st, a)) != hipSuccess) return e;
    } else if (a.ntiles) {
        k_split_tscan<<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0], a.status[0],
                                                   a.s1, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.ntiles) {
        k_split_compact<<<a.ntiles, kThreads, 0, st>>>(a.desc, b.rest_off, a.tiles, a.payload, a.offsets, a.ticket[1],
                                                     a.status[1], a.s1, a.s2, b.s3, a.budget ? a.keyw : nullptr, a.out,
                                                     b.rest, a.keptw, b.restw, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_split_diff<<<dim3(a.ntiles, 2), kThreads, 0, st>>>(a.desc, b.rest_off, a.tiles, a.s2, b.s3, a.keptw, b.restw,
                                                           a.out, b.rest);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    k_split_units<<<((uint32_t)a.n + kThreads - 1) / kThreads, kThreads, 0, st>>>(
        a.desc, b.rest_off, a.n, a.payload, a.offsets, a.keptw, b.restw, a.out, a.out_offsets, a.kept, b.rest,
        b.rest_offsets, b.rest_pairs, a.err);
    return hipGetLastError();
}

// ---- merge ---------------------------------------------------------------------------------------------
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
