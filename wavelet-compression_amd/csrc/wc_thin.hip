// wc_thin.hip — thinning of standard payloads in the compressed domain
// (wc_thin_budget and wc_thin_thresh in include/wavelet_amd.h): a payload P of a
// unit W x H x D with L levels becomes the payload the size-budget selection, or
// a per-level threshold test, gives on A(P), the flat array P decodes to.  No
// cell and no dense coefficient exists anywhere: the work follows the pairs.
//
// Not part of the reference's codec.  The rule needs (position, value) per kept
// pair and nothing else: the level of a coefficient follows from its flat
// position (wc_leveltol.h lt_levels4), the key from its value bits and level
// (wc_budget.h bg_key).  Positions come from the decoders' pair-tile scan
// (wc_pairscan.h PairScan<Sat32, Granule62, kFlatTile, LoadPairs>).
//
// Passes (one stream, nothing read back; tiles = the plan's decode tiles of the
// units, interleaved by tile index across units):
//   k_thin_scan<B>      per pair tile: the positions, then {key, pos} per pair into
//                       the scratch.  Budget form: key = bg_key of a candidate at a
//                       position below N, else 0.  Threshold form: key = 1 where
//                       |c| > t_lvl at a position below N, else 0 (and T = 0).
//   k_thin_solo         budget form, one workgroup per unit of up to
//                       WC_OPT_TOL_SOLO_TILES tiles: the three digits (12 + 12 + 7
//                       bits) of the radix select over the unit's keys, then
//                       thresh[u][1..L] / key[u] (wc_budget.h bg_walk, bg_write)
//   k_thin_digit<P> / k_thin_pick<P>   larger units, a run of tiles per workgroup
//                       and one wave per unit and digit, as k_budget_digit /
//                       k_budget_pick.  The key carries its level's offset, so a
//                       digit's counts are one plain bin set: 4096 + 24 (L - 1)
//                       bins for the first digit, no per-level sets and no walk
//                       over shifted sums.
//   k_thin_compact      per pair tile: kept = key > T; the look-back is the plain
//                       sum of kept counts (derive path: a tile's own scratch
//                       row); kept pair k' gets its value in the output slot and
//                       its position in the second scratch
//   k_thin_diff         run_k' = pos_k' - pos_{k'-1} - 1 (pos_{-1} = -1)
//   k_thin_units        per unit: header, d_kept, d_out_offsets; the header check
//                       of every unit (kErrHeader)
// Which tiles run: T = min(pair tiles of the payload, ceil(N / kFlatTile)), as in
// k_decode_region: pair k sits at a position >= k, so a tile t >= T holds only
// pairs at or past N; its blocks leave after the header, before any atomic, and
// no pass reads a scratch row of it.  A tile t < T always publishes, and writes a
// scratch entry for each of its pairs, whatever its prefix.  Both look-backs are
// lookback_sum's: after its bound a wave derives a predecessor's sum from that
// tile's own inputs (the payload's runs; the scratch row an earlier launch
// wrote), so no wait depends on which workgroups are resident.
//
// Scratch (wc_ctx::thin, grown before the first launch): 8 B ({key, pos}) + 4 B
// (kept positions) per pair a unit can hold below N, rounded up to whole tiles:
// 12 B x kFlatTile x ceil(N / kFlatTile) per unit.  The pair count of a payload is
// not known to the host without a read-back, so the bound is per coefficient.
//
// Bounds: a scratch entry is written for pair k < n of a tile t < T <= the unit's
// plan tiles, inside the unit's rows.  An output pair is written at k' < cap, a
// run at k' < kept <= cap, inside the unit's slot of 24 + 8 cap bytes.  A negative
// run counts as run 0 (Sat32; kErrNegativeRun), so positions still grow.
#include "wc_budget.h"
#include "wc_pairscan.h"
#include "wc_thinunit.h"

namespace wc {

constexpr int kThinTopBins = kHistBins + WC_LTOL_SHIFT * (WC_MAX_LEVELS - 1);  // the first digit's values at L = 4
constexpr int kThinBinStride = 4352;                                           // global bins per split unit
static_assert(kThinBinStride >= kThinTopBins, "a split unit's global bins hold the first digit");

template <bool kBudget>
__global__ __launch_bounds__(kThreads) void k_thin_scan(const ThinDesc* __restrict__ desc,
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
    const uint32_t n = U.n;
    const uint32_t t = Scan::tile_index(ft.index, U.T, ordered, ticket + u, s_x);

    // 1. this lane's pairs and the saturating in-wave inclusive sums of (run + 1);
    // 2. the sum over the unit's earlier tiles
    PayloadRuns src;
    src.runs = U.runs;
    const uint32_t kw = Scan::wave_first(t, w);
    uint2 q[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) q[r] = Scan::load(U.runs, kw + r * 64 + l, n);
    uint32_t incl[Scan::kRounds];
    Scan::WaveSums ws;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) incl[r] = ws.round(q[r], kw + r * 64 + l, n);
    const Scan::Prefix P = Scan::prefix(ws.finish(err), t, n, src, status + C.dt_begin, Granule62{}, err, s_w, s_x, w, l);

    // 3. {key, pos} of every pair of the tile (a pair at or past N: key 0)
    const LtGeom G{C.dmagic, C.hmagic, (uint32_t)C.W, (uint32_t)C.H, (uint32_t)C.D, (int)C.L};
    uint2* __restrict__ row = s1 + (size_t)C.dt_begin * kFlatTile;
    const uint64_t base = (uint64_t)P.excl + P.wexcl;  // + incl[r] - 1: position of the lane's pair in round r
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        if (k >= n) continue;
        const uint64_t p64 = base + incl[r] - 1u;  // incl >= 1 where k < n
        uint2 e = make_uint2(0u, 0xffffffffu);
        if (p64 < (uint64_t)C.N) {
            const uint32_t p = (uint32_t)p64;
            const uint32_t m = q[r].y & 0x7fffffffu;
            const uint32_t lv = (lt_levels4(G, p & ~3u) >> (2u * (p & 3u))) & 3u;
            e.y = p;
            if (kBudget) {
                e.x = bg_candidate(m) ? bg_key(m, lv) : 0u;
            } else {
                const float th = lv == 0u ? C.th[0] : lv == 1u ? C.th[1] : lv == 2u ? C.th[2] : C.th[3];
                e.x = __uint_as_float(m) > th ? 1u : 0u;  // strict: false for NaN
            }
        }
        row[k] = e;
    }
}

// ---- the radix select over a unit's keys ------------------------------------------------------------
// digit P of the keys of pairs [k0, k1) of a scratch row into the bins h
template <int P>
__device__ __forceinline__ void thin_bin(uint32_t* h, const uint2* __restrict__ row, uint32_t k0, uint32_t k1,
                                         uint32_t prefix) {
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += kLtThreads) {
        const uint32_t key = row[k].x;
        if (!key) continue;
        if (P == 1)
            atomicAdd(h + (key >> kHistShift), 1u);
        else if (P == 2 && (key >> kHistShift) == prefix)
            atomicAdd(h + ((key >> 7) & (kBgMidBins - 1)), 1u);
        else if (P == 3 && (key >> 7) == prefix)
            atomicAdd(h + (key & (kBgLowBins - 1)), 1u);
    }
}
__device__ __forceinline__ int thin_top_bins(int L) { return kHistBins + WC_LTOL_SHIFT * (L - 1); }

// T of unit u: the thresholds (entries past L: 0.0f), the pass's own key word and the caller's
__device__ __forceinline__ void thin_write(uint32_t T, int L, uint32_t u, float* __restrict__ thresh,
                                           uint32_t* __restrict__ keyw, uint32_t* __restrict__ key_out) {
    bg_write(T, L, thresh + (size_t)u * WC_MAX_LEVELS, keyw + u);
    if (key_out) key_out[u] = T;
}

// Workgroup u owns unit u unless the unit is split (desc[u].slot != kLtSolo).
__global__ __launch_bounds__(kLtThreads) void k_thin_solo(const ThinDesc* __restrict__ desc,
                                                        const uint8_t* __restrict__ payload,
                                                        const uint64_t* __restrict__ offsets,
                                                        const uint2* __restrict__ s1, float* __restrict__ thresh,
                                                        uint32_t* __restrict__ keyw, uint32_t* __restrict__ key_out) {
    const uint32_t u = blockIdx.x;
    const ThinDesc C = desc[u];
    if (C.slot != kLtSolo) return;  // uniform
    __shared__ uint32_t h[kThinTopBins];
    __shared__ uint32_t st[3];  // found, digit, above
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    const uint2* __restrict__ row = s1 + (size_t)C.dt_begin * kFlatTile;
    const uint32_t K = C.K, np = U.np;  // a refused unit: no key, T = 0
    const int L = (int)C.L, ln = (int)threadIdx.x;

    lt_zero(h, thin_top_bins(L));
    thin_bin<1>(h, row, 0u, np, 0u);
    __syncthreads();
    if (ln < kWave) {
        uint32_t above = 0u;
        int d = 0;
        const bool found = bg_walk([&](int s) { return h[s]; }, thin_top_bins(L), K, ln, above, d);
        if (ln == 0) {
            st[0] = found ? 1u : 0u;
            st[1] = (uint32_t)d;
            st[2] = above;
        }
    }
    __syncthreads();
    if (!st[0]) {  // uniform: at most K candidates
        if (ln == 0) thin_write(0u, L, u, thresh, keyw, key_out);
        return;
    }
    const uint32_t s = st[1];
    lt_zero(h, kBgMidBins);
    thin_bin<2>(h, row, 0u, np, s);
    __syncthreads();
    if (ln < kWave) {
        uint32_t above = st[2];
        int d = 0;
        (void)bg_walk([&](int i) { return h[i]; }, kBgMidBins, K, ln, above, d);
        if (ln == 0) {
            st[1] = (s << 12) | (uint32_t)d;
            st[2] = above;
        }
    }
    __syncthreads();
    const uint32_t prefix = st[1];
    lt_zero(h, kBgLowBins);
    thin_bin<3>(h, row, 0u, np, prefix);
    __syncthreads();
    if (ln < kWave) {
        uint32_t above = st[2];
        int d = 0;
        (void)bg_walk([&](int i) { return h[i]; }, kBgLowBins, K, ln, above, d);
        if (ln == 0) thin_write((prefix << 7) | (uint32_t)d, L, u, thresh, keyw, key_out);
    }
}

// Work item i: pair tiles [items[i].y, + chunk) of split unit items[i].x, digit P's
// bins added to the unit's global bins gbins + slot * kThinBinStride (zeroed by
// the caller).
template <int P>
__global__ __launch_bounds__(kLtThreads) void k_thin_digit(const ThinDesc* __restrict__ desc,
                                                         const uint8_t* __restrict__ payload,
                                                         const uint64_t* __restrict__ offsets,
                                                         const uint2* __restrict__ items, uint32_t chunk,
                                                         const uint2* __restrict__ s1,
                                                         const BudgetState* __restrict__ state,
                                                         uint32_t* __restrict__ gbins) {
    constexpr int kBins = P == 1 ? kThinTopBins : P == 2 ? kBgMidBins : kBgLowBins;
    const uint2 it = items[blockIdx.x];
    const ThinDesc C = desc[it.x];
    BudgetState S{0u, 0u, 0u, 0u};
    if (P > 1) {
        S = state[C.slot];
        if (S.done) return;  // uniform
    }
    const ThinUnit U = thin_open(C, payload, offsets[it.x]);
    const uint32_t k0 = it.y * (uint32_t)kFlatTile;  // < 2^31: a tile of the plan
    const uint32_t k1 = (uint32_t)min((uint64_t)U.np, (uint64_t)k0 + (uint64_t)chunk * kFlatTile);
    if (k0 >= k1) return;  // uniform: no pair of the payload in these tiles
    __shared__ uint32_t h[kBins];
    const int nb = P == 1 ? thin_top_bins((int)C.L) : kBins;
    lt_zero(h, nb);
    thin_bin<P>(h, s1 + (size_t)C.dt_begin * kFlatTile, k0, k1, S.prefix);
    __syncthreads();
    uint32_t* __restrict__ g = gbins + (size_t)C.slot * kThinBinStride;
    for (int i = threadIdx.x; i < nb; i += kLtThreads)
        if (h[i]) atomicAdd(g + i, h[i]);
}

// Workgroup s (one wave): the walk of split unit split_units[s] over digit P's global bins.
template <int P>
__global__ __launch_bounds__(kWave) void k_thin_pick(const ThinDesc* __restrict__ desc,
                                                   const uint32_t* __restrict__ split_units,
                                                   const uint32_t* __restrict__ gbins,
                                                   BudgetState* __restrict__ state, float* __restrict__ thresh,
                                                   uint32_t* __restrict__ keyw, uint32_t* __restrict__ key_out) {
    const uint32_t u = split_units[blockIdx.x];
    const int L = (int)desc[u].L, ln = (int)threadIdx.x;
    const uint32_t K = desc[u].K;
    const uint32_t* h = gbins + (size_t)blockIdx.x * kThinBinStride;
    BudgetState S = state[blockIdx.x];
    int d = 0;
    if (P == 1) {
        uint32_t above = 0u;
        const bool found = bg_walk([&](int s) { return h[s]; }, thin_top_bins(L), K, ln, above, d);
        if (ln == 0) {
            state[blockIdx.x] = {(uint32_t)d, above, found ? 0u : 1u, 0u};
            if (!found) thin_write(0u, L, u, thresh, keyw, key_out);
        }
        return;
    }
    if (S.done) return;  // uniform
    (void)bg_walk([&](int i) { return h[i]; }, P == 2 ? kBgMidBins : kBgLowBins, K, ln, S.above, d);
    if (ln != 0) return;
    if (P == 2) {
        state[blockIdx.x] = {(S.prefix << 12) | (uint32_t)d, S.above, 0u, 0u};
    } else {
        state[blockIdx.x] = {S.prefix, S.above, 1u, 0u};
        thin_write((S.prefix << 7) | (uint32_t)d, L, u, thresh, keyw, key_out);
    }
}

// ---- compaction ---------------------------------------------------------------------------------------
// The look-back's derive path: the kept count of tile j of the unit's n pairs from its scratch row.
struct ThinKept {
    const uint2* __restrict__ row;
    uint32_t Tk;
    template <class S, int TILE>
    __device__ __forceinline__ typename S::T tile_sum(int64_t j, typename S::K n, int l) const {
        using K = typename S::K;
        const K k0 = (K)j * TILE, k1 = min(k0 + (K)TILE, n);
        typename S::T a = 0;
        for (K k = k0 + (K)l; k < k1; k += 64) a += row[k].x > Tk ? 1u : 0u;
        return S::last(S::wave_incl(a));
    }
};

__global__ __launch_bounds__(kThreads) void k_thin_compact(const ThinDesc* __restrict__ desc,
                                                         const FTile* __restrict__ tiles,
                                                         const uint8_t* __restrict__ payload,
                                                         const uint64_t* __restrict__ offsets,
                                                         uint32_t* __restrict__ ticket,
                                                         unsigned long long* __restrict__ status,
                                                         const uint2* __restrict__ s1, uint32_t* __restrict__ s2,
                                                         const uint32_t* __restrict__ keyw, uint8_t* __restrict__ out,
                                                         uint32_t* __restrict__ keptw, uint32_t* __restrict__ err,
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
    const uint32_t n = U.n;
    const uint32_t t = Scan::tile_index(ft.index, U.T, ordered, ticket + u, s_x);
    const ThinKept src{s1 + (size_t)C.dt_begin * kFlatTile, keyw[u]};

    const uint32_t kw = Scan::wave_first(t, w);
    uint2 e[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        e[r] = k < n ? src.row[k] : make_uint2(0u, 0u);
    }
    uint32_t incl[Scan::kRounds], wsum = 0u;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t s = wave_incl_sum32(e[r].x > src.Tk ? 1u : 0u);
        incl[r] = wsum + s;
        wsum += __builtin_amdgcn_readlane(s, 63);
    }
    const Scan::Prefix P = Scan::prefix(wsum, t, n, src, status + C.dt_begin, Granule62{}, err, s_w, s_x, w, l);

    uint32_t* __restrict__ pairs = reinterpret_cast<uint32_t*>(out + C.out_off + 20);
    uint32_t* __restrict__ row2 = s2 + (size_t)C.dt_begin * kFlatTile;
    const uint64_t base = (uint64_t)P.excl + P.wexcl;  // + incl[r] - 1: the kept pair's index in the output
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        if (k >= n || !(e[r].x > src.Tk)) continue;
        const uint64_t kp = base + incl[r] - 1u;
        if (kp >= (uint64_t)C.cap) continue;  // never: kept <= cap by the rule; the slot's bound all the same
        pairs[2 * kp + 1] = U.runs[2 * (size_t)k + 1];
        row2[kp] = e[r].y;
    }
    if (t == U.T - 1u && tid == 0) keptw[u] = (uint32_t)min((uint64_t)P.excl + P.tot, (uint64_t)C.cap);
}

// Output tile ft.index of the unit: the runs of its kept pairs from their positions.
__global__ __launch_bounds__(kThreads) void k_thin_diff(const ThinDesc* __restrict__ desc,
                                                      const FTile* __restrict__ tiles,
                                                      const uint32_t* __restrict__ s2,
                                                      const uint32_t* __restrict__ keptw, uint8_t* __restrict__ out) {
    const FTile ft = tiles[blockIdx.x];
    const uint32_t kept = keptw[ft.unit];
    const uint32_t k0 = ft.index * (uint32_t)kFlatTile;
    if (k0 >= kept) return;  // uniform
    const ThinDesc C = desc[ft.unit];
    uint32_t* __restrict__ pairs = reinterpret_cast<uint32_t*>(out + C.out_off + 20);
    const uint32_t* __restrict__ row2 = s2 + (size_t)C.dt_begin * kFlatTile;
#pragma unroll
    for (int i = 0; i < kFlatPerThread; ++i) {
        const uint32_t kp = k0 + i * kThreads + threadIdx.x;
        if (kp >= kept) continue;
        const uint32_t prev = kp ? row2[kp - 1] : 0xffffffffu;  // pos_{-1} = -1
        pairs[2 * (size_t)kp] = row2[kp] - prev - 1u;
    }
}

// Thread u: unit u's header, kept count and offset; a unit whose header disagrees
// keeps its slot untouched (kErrHeader, kept 0).
__global__ __launch_bounds__(kThreads) void k_thin_units(const ThinDesc* __restrict__ desc, int n,
                                                       const uint8_t* __restrict__ payload,
                                                       const uint64_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ keptw, uint8_t* __restrict__ out,
                                                       uint64_t* __restrict__ out_offsets, uint32_t* __restrict__ kept,
                                                       uint32_t* __restrict__ err) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= n) return;
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    const uint32_t k = U.ok ? keptw[u] : 0u;
    if (U.ok) {
        int32_t* h = reinterpret_cast<int32_t*>(out + C.out_off);
        h[0] = C.W;
        h[1] = C.H;
        h[2] = C.D;
        h[3] = C.want;
        h[4] = (int32_t)k;
    } else {
        atomicOr(err, kErrHeader);
    }
    kept[u] = k;
    out_offsets[u] = C.out_off;
    if (u == n - 1) out_offsets[n] = C.out_off + 20 + 8ull * k;
}

// The scan and, in the budget form, the select: {key, pos} per pair in s1, T per unit in keyw
// (wc_layers.hip's split runs these and then its own compaction).
hipError_t launch_thin_front(hipStream_t st, const ThinLaunch& a) {
    if (a.n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.ntiles) {
        if (a.budget)
            k_thin_scan<true><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0],
                                                           a.status[0], a.s1, a.err, a.ordered);
        else
            k_thin_scan<false><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0],
                                                            a.status[0], a.s1, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.budget) {
        if ((uint32_t)a.n > a.nsplit) {
            k_thin_solo<<<(uint32_t)a.n, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.s1, a.thresh, a.keyw,
                                                            a.key_out);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        if (a.nsplit) {
            const size_t bytes = sizeof(uint32_t) * kThinBinStride * (size_t)a.nsplit;
            if ((e = hipMemsetAsync(a.gbins, 0, bytes, st)) != hipSuccess) return e;
            k_thin_digit<1><<<a.nitems, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.items, a.chunk, a.s1,
                                                           a.state, a.gbins);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            k_thin_pick<1><<<a.nsplit, kWave, 0, st>>>(a.desc, a.split_units, a.gbins, a.state, a.thresh, a.keyw,
                                                     a.key_out);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemsetAsync(a.gbins, 0, bytes, st)) != hipSuccess) return e;
            k_thin_digit<2><<<a.nitems, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.items, a.chunk, a.s1,
                                                           a.state, a.gbins);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            k_thin_pick<2><<<a.nsplit, kWave, 0, st>>>(a.desc, a.split_units, a.gbins, a.state, a.thresh, a.keyw,
                                                     a.key_out);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemsetAsync(a.gbins, 0, bytes, st)) != hipSuccess) return e;
            k_thin_digit<3><<<a.nitems, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.items, a.chunk, a.s1,
                                                           a.state, a.gbins);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            k_thin_pick<3><<<a.nsplit, kWave, 0, st>>>(a.desc, a.split_units, a.gbins, a.state, a.thresh, a.keyw,
                                                     a.key_out);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_thin(hipStream_t st, const ThinLaunch& a) {
    if (a.n <= 0) return hipSuccess;
    hipError_t e = launch_thin_front(st, a);
    if (e != hipSuccess) return e;
    if (a.ntiles) {
        k_thin_compact<<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[1], a.status[1],
                                                    a.s1, a.s2, a.keyw, a.out, a.keptw, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_thin_diff<<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.s2, a.keptw, a.out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    k_thin_units<<<((uint32_t)a.n + kThreads - 1) / kThreads, kThreads, 0, st>>>(a.desc, a.n, a.payload, a.offsets,
                                                                               a.keptw, a.out, a.out_offsets, a.kept,
                                                                               a.err);
    return hipGetLastError();
}

}  // namespace wc
