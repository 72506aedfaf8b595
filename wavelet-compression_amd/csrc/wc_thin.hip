// wc_thin.hip — pair selection in the compressed domain: thinning (wc_thin_budget,
// wc_thin_thresh and wc_thin_tol in include/wavelet_amd.h) and the split into
// progressive layers (wc_split_budget, wc_split_thresh and wc_split_tol).  A payload
// P of a unit W x H x D with L levels becomes the payload the size-budget selection,
// a per-level threshold test, or the RMSE-tolerance rule's thresholds give on A(P),
// the flat array P decodes to (thinning; a split's
// base), and, for a split, also its complement inside the canonical form of P
// (the rest).  Thinning is a split whose rest is thrown away: one pipeline, whose
// rest side a thin call leaves out.  No cell and no dense coefficient exists
// anywhere: the work follows the pairs.
//
// Not part of the reference's codec.  The rule needs (position, value) per kept
// pair and nothing else: the level of a coefficient follows from its flat
// position (wc_leveltol.h lt_levels4), the key from its value bits and level
// (wc_budget.h bg_key).  Positions come from the decoders' pair-tile scan
// (wc_thinunit.h tile_positions, on wc_pairscan.h
// PairScan<Sat32, Granule62, kFlatTile, LoadPairs>).
//
// Passes (one stream, nothing read back; tiles = the plan's decode tiles of the
// units, interleaved by tile index across units):
//   k_pair_keys<B>      per pair tile: the positions, then {key, pos} per pair into
//                       the scratch.  Budget form: key = bg_key of a candidate at a
//                       position below N, else 0.  Threshold form: key 2 where
//                       |c| > t_lvl, 1 for any other candidate below N, 0 otherwise,
//                       and T = 1 for every unit.  Tolerance form: the order key of
//                       the rule's walk (tol_key), else 0.
//   k_thin_solo         budget form, one workgroup per unit of up to
//                       WC_OPT_TOL_SOLO_TILES tiles: the radix select over the unit's
//                       keys (wc_budget.h bg_solo), then thresh[u][1..L] / key[u]
//   k_thin_digit<P> / k_thin_pick<P>   larger units, a run of tiles per workgroup
//                       and one wave per unit and digit (bg_pick).  The key carries
//                       its level's offset, so a digit's counts are one plain bin
//                       set: 4096 + 24 (L - 1) bins for the first digit, no
//                       per-level sets and no walk over shifted sums.
//   k_thin_tol_solo<NL>  tolerance form (wc_thin_tol / wc_split_tol), one workgroup per
//                       unit of up to WC_OPT_TOL_SOLO_TILES tiles: the per-level LDS bins
//                       of wc_leveltol.h filled from the scratch row's keys, the zeros
//                       of the box added to bin 0, the rule's walk (lt_pick), then
//                       thresh[u][1..L] / bound[u] and T = the key of the stop
//   k_thin_tol_bins<NL> / k_thin_tol_pick   larger units: LDS bins of a run of tiles
//                       added to the unit's 4 x 16 KiB global bins, then one wave per
//                       unit: the zeros and the walk
//   k_pair_compact<R>   per pair tile: kept = key > T, rest = 0 < key <= T; the
//                       look-back is the plain sum of the counts (derive path: a
//                       tile's own scratch row); a kept pair gets its value in the
//                       output slot and its position in the second scratch.  <false>
//                       (thinning) counts the kept pairs alone, in 32 bits.  <true>
//                       (split) carries the pair (base count, rest count) as one
//                       62-bit granule, base in bits 0-30 and rest in bits 31-61:
//                       both are sums of counts below 2^31, so neither field carries
//                       into the other and lookback_sum's algebra holds; a rest pair
//                       goes to the rest's slot and the third scratch.
//   k_pair_diff         grid y = output (base; rest): run_k' = pos_k' - pos_{k'-1} - 1
//                       (pos_{-1} = -1)
//   k_pair_units        per unit: header, count and offsets of the output, and of
//                       the rest where there is one; the header check (kErrHeader)
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
// 12 B x kFlatTile x ceil(N / kFlatTile) per unit; a split has 4 B more for the
// rest's positions.  The pair count of a payload is not known to the host without
// a read-back, so the bound is per coefficient.
//
// Bounds: a scratch entry is written for pair k < n of a tile t < T <= the unit's
// plan tiles, inside the unit's rows.  An output pair is written at k' < cap, a
// run at k' < kept <= cap, inside the unit's slot of 24 + 8 cap bytes; a rest pair
// at k' < N inside its slot of 24 + 8 N bytes.  A negative run counts as run 0
// (Sat32; kErrNegativeRun), so positions still grow.
#include "wc_budget.h"
#include "wc_pairscan.h"
#include "wc_thinunit.h"

#include <type_traits>

namespace wc {

constexpr int kThinTopBins = kHistBins + WC_LTOL_SHIFT * (WC_MAX_LEVELS - 1);  // bg_top_bins(4)
constexpr int kThinBinStride = 4352;                                           // global bins per split unit
static_assert(kThinBinStride >= kThinTopBins, "a split unit's global bins hold the first digit");

// The tolerance form's order key.  The rule (include/wavelet_amd.h, wc_tol_levels_threshold) visits the
// nonempty (s, l), s = b + WC_LTOL_SHIFT (l - 1), in lexicographic order and drops what it visits before
// its stop (s*, l*): with code(s, l) = (s << 2) | (l - 1) a candidate is kept iff code >= code(s*, l*),
// which is |c| > thresh_l for the thresholds the rule derives (bstar_l = s* + (l < l*) - WC_LTOL_SHIFT
// (l - 1) is the first b of level l with code >= code(s*, l*)).  key = code + 1, so that 0 stays "no
// candidate", and T = code(s*, l*): kept = key > T.  +-inf is above every threshold the rule can give
// (FLT_MAX at most), yet without a stop (a budget of +inf) the walk passes its bin: it gets s = kTolInfS,
// past every s of the walk, and T = kTolNoStop keeps exactly the +-inf pairs then.
constexpr uint32_t kTolInfS = 0x3ffffffeu;
constexpr uint32_t kTolNoStop = kTolInfS << 2;
__device__ __forceinline__ uint32_t tol_key(uint32_t m, uint32_t lv) {
    const uint32_t s = m == kBgInf ? kTolInfS : (m >> kHistShift) + (uint32_t)WC_LTOL_SHIFT * lv;
    return ((s << 2) | lv) + 1u;
}
// (level index, bin) of a key
__device__ __forceinline__ uint2 tol_unkey(uint32_t key) {
    const uint32_t c = key - 1u, lv = c & 3u, s = c >> 2;
    return make_uint2(lv, s == kTolInfS ? kBgInf >> kHistShift : s - (uint32_t)WC_LTOL_SHIFT * lv);
}

enum { kFormThresh = 0, kFormBudget = 1, kFormTol = 2 };

// {key, pos} of every pair of the tile (a pair at or past N: key 0).  The threshold form's three
// classes select for thinning what key = (|c| > t) would: the host refuses a threshold that is NaN
// or negative, so t >= 0, and then float(m) > t implies 1 <= m <= 0x7F800000, which is
// bg_candidate(m) (+-0 and NaN are not above t, and denormals are not flushed in this build): the
// pairs with key 2 are the pairs with |c| > t, and T = 1 keeps exactly those.
template <int kForm>
__global__ __launch_bounds__(kThreads) void k_pair_keys(const ThinDesc* __restrict__ desc,
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
            e.y = p;
            if (kForm == kFormBudget) {
                e.x = bg_candidate(m) ? bg_key(m, lv) : 0u;
            } else if (kForm == kFormTol) {
                e.x = bg_candidate(m) ? tol_key(m, lv) : 0u;
            } else {
                const float th = lv == 0u ? C.th[0] : lv == 1u ? C.th[1] : lv == 2u ? C.th[2] : C.th[3];
                e.x = !bg_candidate(m) ? 0u : __uint_as_float(m) > th ? 2u : 1u;  // strict
            }
        }
        row[k] = e;
    }
}

// ---- the radix select over a unit's keys (wc_budget.h) ----------------------------------------------
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
    __shared__ uint32_t st[3];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    const uint2* __restrict__ row = s1 + (size_t)C.dt_begin * kFlatTile;
    const uint32_t np = U.np;  // a refused unit: no key, T = 0
    const int L = (int)C.L;
    bg_solo(
        h, st, L, C.K,
        [&] {
            lt_zero(h, bg_top_bins(L));
            thin_bin<1>(h, row, 0u, np, 0u);
            __syncthreads();
        },
        [&](int s) { return h[s]; }, [&](uint32_t s) { thin_bin<2>(h, row, 0u, np, s); },
        [&](uint32_t prefix) { thin_bin<3>(h, row, 0u, np, prefix); },
        [&](uint32_t T) { thin_write(T, L, u, thresh, keyw, key_out); });
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
    const int nb = P == 1 ? bg_top_bins((int)C.L) : kBins;
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
    const int L = (int)desc[u].L;
    const uint32_t* h = gbins + (size_t)blockIdx.x * kThinBinStride;
    bg_pick<P>(
        state + blockIdx.x, L, desc[u].K, [&](int s) { return h[s]; }, h,
        [&](uint32_t T) { thin_write(T, L, u, thresh, keyw, key_out); });
}

// ---- the tolerance rule over a unit's keys (wc_leveltol.h) ----------------------------------------------
// cnt[l][b] of A(P) from the pairs alone: a candidate counts in the bin of its key; every position of
// level l that holds no pair, or a +-0 pair, is a zero of bin 0; a NaN pair counts nowhere.  So bin 0 of
// level l gets N_l - (candidates of level l) - (NaN pairs of level l below N) more, N_l the positions of
// level l in the box.
static_assert(kThinTolBinStride == WC_MAX_LEVELS * kHistBins + WC_MAX_LEVELS, "a split unit's bin sets and NaN counts");

__device__ __forceinline__ uint32_t tol_level_size(const ThinDesc& C, int l) {  // l = level - 1
    const uint32_t a = ((uint32_t)C.W >> l) * ((uint32_t)C.H >> l) * ((uint32_t)C.D >> l);
    const int j = l + 1;
    return j < (int)C.L ? a - ((uint32_t)C.W >> j) * ((uint32_t)C.H >> j) * ((uint32_t)C.D >> j) : a;
}

// Pairs [k0, k1) of a scratch row into the per-level LDS bins h (lt_add1's layout) and the NaN pairs
// below N into nan[level - 1].  A key-0 pair below N is +-0 or NaN: its value decides, its level comes
// from its position (such pairs are rare: no encoder of this project emits one).
__device__ __forceinline__ void tol_bin(uint32_t* h, uint32_t* nan, const ThinDesc& C, const ThinUnit& U,
                                        const uint2* __restrict__ row, uint32_t k0, uint32_t k1) {
    const uint32_t set = threadIdx.x & 1u;
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += kLtThreads) {
        const uint2 e = row[k];
        if (e.x) {
            const uint2 lb = tol_unkey(e.x);
            lt_add1(h, set, __uint_as_float(lb.y << kHistShift), lb.x);
        } else if (e.y != 0xffffffffu && (U.runs[2 * (size_t)k + 1] & 0x7fffffffu) > kBgInf) {
            const LtGeom G{C.dmagic, C.hmagic, (uint32_t)C.W, (uint32_t)C.H, (uint32_t)C.D, (int)C.L};
            atomicAdd(nan + ((lt_levels4(G, e.y & ~3u) >> (2u * (e.y & 3u))) & 3u), 1u);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t a) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, kWave);
    return a;
}

// T and the outputs of unit u from the stop of the walk
__device__ __forceinline__ void tol_write(int2 stop, uint32_t u, uint32_t* __restrict__ keyw) {
    keyw[u] = stop.x < 0 ? kTolNoStop : ((uint32_t)stop.x << 2) | (uint32_t)(stop.y - 1);
}

// A unit whose header disagrees: no pair is read; thresholds and bound 0 (its slot stays untouched).
__device__ __forceinline__ void tol_refused(uint32_t u, float* __restrict__ thresh, double* __restrict__ bound,
                                            uint32_t* __restrict__ keyw) {
#pragma unroll
    for (int l = 0; l < WC_MAX_LEVELS; ++l) thresh[(size_t)u * WC_MAX_LEVELS + l] = 0.0f;
    if (bound) bound[u] = 0.0;
    keyw[u] = kTolNoStop;
}

// Workgroup u owns unit u unless the unit is split (desc[u].slot != kLtSolo).  NL = the largest L of
// the call; LDS as k_ltol_solo<NL>: (NL + 1) x 16 KiB.
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_thin_tol_solo(const ThinDesc* __restrict__ desc,
                                                            const uint8_t* __restrict__ payload,
                                                            const uint64_t* __restrict__ offsets,
                                                            const uint2* __restrict__ s1, float* __restrict__ thresh,
                                                            double* __restrict__ bound, uint32_t* __restrict__ keyw) {
    const uint32_t u = blockIdx.x;
    const ThinDesc C = desc[u];
    if (C.slot != kLtSolo) return;  // uniform
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    __shared__ uint32_t cnt[2 * WC_MAX_LEVELS];  // per level: candidates, then NaN pairs
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    if (!U.ok) {  // uniform
        if (threadIdx.x == 0) tol_refused(u, thresh, bound, keyw);
        return;
    }
    const int L = min((int)C.L, NL);  // (C.L <= NL by the caller; the bound of h all the same)
    if (threadIdx.x < 2 * WC_MAX_LEVELS) cnt[threadIdx.x] = 0u;
    lt_zero(h, (NL + 1) * kHistBins);
    tol_bin(h, cnt + WC_MAX_LEVELS, C, U, s1 + (size_t)C.dt_begin * kFlatTile, 0u, U.np);
    lt_fold(h);
    for (int l = 0; l < L; ++l) {
        const uint32_t* hl = h + lt_base(l + 1);
        uint32_t a = 0u;
        for (int i = threadIdx.x; i < kHistBins; i += kLtThreads) a += hl[i];
        a = wave_sum32(a);
        if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(cnt + l, a);
    }
    __syncthreads();
    if ((int)threadIdx.x < L) {
        const int l = (int)threadIdx.x;
        h[lt_base(l + 1)] += tol_level_size(C, l) - cnt[l] - cnt[WC_MAX_LEVELS + l];
    }
    __syncthreads();
    if (threadIdx.x < kWave) {
        const int2 stop = lt_pick(h, 2 * kHistBins, L, (uint64_t)C.N, C.tol, (int)threadIdx.x,
                                  thresh + (size_t)u * WC_MAX_LEVELS, bound ? bound + u : nullptr);
        if (threadIdx.x == 0) tol_write(stop, u, keyw);
    }
}

// Work item i: pair tiles [items[i].y, + chunk) of split unit items[i].x, added to the unit's global
// bins gbins + slot * kThinTolBinStride (zeroed by the caller).
template <int NL>
__global__ __launch_bounds__(kLtThreads) void k_thin_tol_bins(const ThinDesc* __restrict__ desc,
                                                            const uint8_t* __restrict__ payload,
                                                            const uint64_t* __restrict__ offsets,
                                                            const uint2* __restrict__ items, uint32_t chunk,
                                                            const uint2* __restrict__ s1,
                                                            uint32_t* __restrict__ gbins) {
    const uint2 it = items[blockIdx.x];
    const ThinDesc C = desc[it.x];
    const ThinUnit U = thin_open(C, payload, offsets[it.x]);
    const uint32_t k0 = it.y * (uint32_t)kFlatTile;  // < 2^31: a tile of the plan
    const uint32_t k1 = (uint32_t)min((uint64_t)U.np, (uint64_t)k0 + (uint64_t)chunk * kFlatTile);
    if (k0 >= k1) return;  // uniform: no pair of the payload in these tiles (a refused unit: np = 0)
    __shared__ uint32_t h[(NL + 1) * kHistBins];
    __shared__ uint32_t nan[WC_MAX_LEVELS];
    if (threadIdx.x < WC_MAX_LEVELS) nan[threadIdx.x] = 0u;
    lt_zero(h, (NL + 1) * kHistBins);
    tol_bin(h, nan, C, U, s1 + (size_t)C.dt_begin * kFlatTile, k0, k1);
    lt_fold(h);
    uint32_t* __restrict__ g = gbins + (size_t)C.slot * kThinTolBinStride;
    const int L = min((int)C.L, NL);
    for (int l = 0; l < L; ++l) {
        const uint32_t* hl = h + lt_base(l + 1);
        for (int i = threadIdx.x; i < kHistBins; i += kLtThreads)
            if (hl[i]) atomicAdd(g + l * kHistBins + i, hl[i]);
    }
    if ((int)threadIdx.x < L && nan[threadIdx.x])
        atomicAdd(g + WC_MAX_LEVELS * kHistBins + threadIdx.x, nan[threadIdx.x]);
}

// Workgroup s (one wave): the zeros of bin 0 and the walk of split unit split_units[s] over its global bins.
__global__ __launch_bounds__(kWave) void k_thin_tol_pick(const ThinDesc* __restrict__ desc,
                                                       const uint8_t* __restrict__ payload,
                                                       const uint64_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ split_units, uint32_t* gbins,
                                                       float* __restrict__ thresh, double* __restrict__ bound,
                                                       uint32_t* __restrict__ keyw) {
    const uint32_t u = split_units[blockIdx.x];
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    if (!U.ok) {  // uniform
        if (threadIdx.x == 0) tol_refused(u, thresh, bound, keyw);
        return;
    }
    uint32_t* g = gbins + (size_t)blockIdx.x * kThinTolBinStride;
    const int L = (int)C.L;
    for (int l = 0; l < L; ++l) {
        uint32_t a = 0u;
        for (int i = threadIdx.x; i < kHistBins; i += kWave) a += g[l * kHistBins + i];
        a = wave_sum32(a);
        if (threadIdx.x == 0) g[l * kHistBins] += tol_level_size(C, l) - a - g[WC_MAX_LEVELS * kHistBins + l];
    }
    __syncthreads();  // (one wave: lane 0's stores before every lane's loads)
    const int2 stop = lt_pick(g, kHistBins, L, (uint64_t)C.N, C.tol, (int)threadIdx.x, thresh + (size_t)u * WC_MAX_LEVELS,
                              bound ? bound + u : nullptr);
    if (threadIdx.x == 0) tol_write(stop, u, keyw);
}

// ---- compaction ---------------------------------------------------------------------------------------
using CountScan = PairScan<Exact64, Granule62, kFlatTile, LoadPairs>;  // its prefix alone: the packed counts
constexpr int kRestShift = 31;
constexpr uint64_t kCountMask = (1ull << kRestShift) - 1;

// The look-back's derive path: the counts of tile j of the unit's n pairs from its scratch row
// (kRest: the rest's count beside the kept one, from bit kRestShift).
template <bool kRest>
struct PairCounts {
    const uint2* __restrict__ row;
    uint32_t Tk;
    template <class S, int TILE>
    __device__ __forceinline__ typename S::T tile_sum(int64_t j, typename S::K n, int l) const {
        using K = typename S::K;
        const K k0 = (K)j * TILE, k1 = min(k0 + (K)TILE, n);
        typename S::T a = 0;
        for (K k = k0 + (K)l; k < k1; k += 64) {
            const uint32_t key = row[k].x;
            a += key > Tk ? 1u : kRest && key ? (typename S::T)1 << kRestShift : 0u;
        }
        return S::last(S::wave_incl(a));
    }
};

template <bool kRest>
__global__ __launch_bounds__(kThreads) void k_pair_compact(
    const ThinDesc* __restrict__ desc, const FTile* __restrict__ tiles, const uint8_t* __restrict__ payload,
    const uint64_t* __restrict__ offsets, uint32_t* __restrict__ ticket, unsigned long long* __restrict__ status,
    const uint2* __restrict__ s1, uint32_t* __restrict__ s2, uint32_t* __restrict__ s3,
    const uint32_t* __restrict__ keyw, uint8_t* __restrict__ out, uint8_t* __restrict__ rest,
    uint32_t* __restrict__ keptw, uint32_t* __restrict__ restw, uint32_t* __restrict__ err, int ordered) {
    using Scan = std::conditional_t<kRest, CountScan, ThinScan>;
    __shared__ typename Scan::T s_w[4];
    __shared__ typename Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const ThinDesc C = desc[u];
    const ThinUnit U = thin_open(C, payload, offsets[u]);
    if (!U.ok || ft.index >= U.T) return;  // uniform; before any atomic
    const uint32_t n = U.n;
    const uint32_t t = Scan::tile_index(ft.index, U.T, ordered, ticket + u, s_x);
    const PairCounts<kRest> src{s1 + (size_t)C.dt_begin * kFlatTile, keyw ? keyw[u] : 1u};  // threshold form: T = 1

    const uint32_t kw = (uint32_t)Scan::wave_first(t, w);
    uint2 e[Scan::kRounds];
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        e[r] = k < n ? src.row[k] : make_uint2(0u, 0u);
    }
    // kRest: in the wave both counts fit one word, base in bits 0-15, rest in bits 16-31 (at most 1024 each)
    uint32_t incl[Scan::kRounds], wsum = 0u;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t s = wave_incl_sum32(e[r].x > src.Tk ? 1u : kRest && e[r].x ? 0x10000u : 0u);
        incl[r] = wsum + s;
        wsum += __builtin_amdgcn_readlane(s, 63);
    }
    typename Scan::T wtot = wsum;
    if constexpr (kRest) wtot = (uint64_t)(wsum & 0xffffu) | ((uint64_t)(wsum >> 16) << kRestShift);
    const typename Scan::Prefix P =
        Scan::prefix(wtot, t, (typename Scan::K)n, src, status + C.dt_begin, Granule62{}, err, s_w, s_x, w, l);

    uint32_t* __restrict__ pairs = reinterpret_cast<uint32_t*>(out + C.out_off + 20);
    uint32_t* __restrict__ row2 = s2 + (size_t)C.dt_begin * kFlatTile;
    // + the lane's in-wave count - 1: the pair's index in its output (kRest: neither field carries,
    // each total is below 2^31)
    const uint64_t before = (uint64_t)P.excl + P.wexcl;
    const uint64_t bbase = kRest ? before & kCountMask : before;
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        if (k >= n) continue;
        if (e[r].x > src.Tk) {
            const uint64_t kp = bbase + (kRest ? incl[r] & 0xffffu : incl[r]) - 1u;
            if (kp >= (uint64_t)C.cap) continue;  // never: kept <= cap by the rule; the slot's bound all the same
            pairs[2 * kp + 1] = U.runs[2 * (size_t)k + 1];
            row2[kp] = e[r].y;
        } else if (kRest && e[r].x) {
            const uint64_t kp = (before >> kRestShift) + (incl[r] >> 16) - 1u;
            if (kp >= (uint64_t)C.N) continue;  // never: a rest pair sits below N; the slot's bound all the same
            reinterpret_cast<uint32_t*>(rest + C.rest_off + 20)[2 * kp + 1] = U.runs[2 * (size_t)k + 1];
            (s3 + (size_t)C.dt_begin * kFlatTile)[kp] = e[r].y;
        }
    }
    if (t == U.T - 1u && tid == 0) {
        const uint64_t all = (uint64_t)P.excl + P.tot;
        keptw[u] = (uint32_t)min(kRest ? all & kCountMask : all, (uint64_t)C.cap);
        if constexpr (kRest) restw[u] = (uint32_t)min(all >> kRestShift, (uint64_t)C.N);
    }
}

// Output tile ft.index of the unit's output blockIdx.y (0: the kept pairs, 1: the rest): the runs from
// the positions.
__global__ __launch_bounds__(kThreads) void k_pair_diff(const ThinDesc* __restrict__ desc,
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
    uint32_t* __restrict__ pairs = reinterpret_cast<uint32_t*>(second ? rest + C.rest_off + 20 : out + C.out_off + 20);
    const uint32_t* __restrict__ row = (second ? s3 : s2) + (size_t)C.dt_begin * kFlatTile;
#pragma unroll
    for (int i = 0; i < kFlatPerThread; ++i) {
        const uint32_t kp = k0 + i * kThreads + threadIdx.x;
        if (kp >= cnt) continue;
        const uint32_t prev = kp ? row[kp - 1] : 0xffffffffu;  // pos_{-1} = -1
        pairs[2 * (size_t)kp] = row[kp] - prev - 1u;
    }
}

// Thread u: unit u's header, kept count and offset, and the same of its rest where `rest` is given;
// a unit whose header disagrees keeps its slots untouched (kErrHeader, counts 0).
__global__ __launch_bounds__(kThreads) void k_pair_units(const ThinDesc* __restrict__ desc, int n,
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
    const uint32_t kb = U.ok ? keptw[u] : 0u, kr = U.ok && rest ? restw[u] : 0u;
    if (U.ok) {
        write_header(out + C.out_off, C, kb);
        if (rest) write_header(rest + C.rest_off, C, kr);
    } else {
        atomicOr(err, kErrHeader);
    }
    kept[u] = kb;
    out_offsets[u] = C.out_off;
    if (u == n - 1) out_offsets[n] = C.out_off + 20 + 8ull * kb;
    if (!rest) return;
    rest_pairs[u] = kr;
    rest_offsets[u] = C.rest_off;
    if (u == n - 1) rest_offsets[n] = C.rest_off + 20 + 8ull * kr;
}

// f(std::integral_constant<int, NL>), NL = the call's largest L
template <class F>
static void by_levels(int maxl, F f) {
    switch (maxl) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

hipError_t launch_thin(hipStream_t st, const ThinLaunch& a) {
    if (a.n <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.ntiles) {
        if (a.budget)
            k_pair_keys<kFormBudget><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0],
                                                                  a.status[0], a.s1, a.err, a.ordered);
        else if (a.tol)
            k_pair_keys<kFormTol><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0],
                                                               a.status[0], a.s1, a.err, a.ordered);
        else
            k_pair_keys<kFormThresh><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[0],
                                                                  a.status[0], a.s1, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.budget && (uint32_t)a.n > a.nsplit) {
        k_thin_solo<<<(uint32_t)a.n, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.s1, a.thresh, a.keyw,
                                                        a.key_out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.budget && a.nsplit) {
        e = bg_passes<1>(
            st, a.gbins, sizeof(uint32_t) * kThinBinStride * (size_t)a.nsplit,
            [&](auto P) {
                k_thin_digit<decltype(P)::value><<<a.nitems, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.items,
                                                                                  a.chunk, a.s1, a.state, a.gbins);
            },
            [&](auto P) {
                k_thin_pick<decltype(P)::value><<<a.nsplit, kWave, 0, st>>>(a.desc, a.split_units, a.gbins, a.state,
                                                                            a.thresh, a.keyw, a.key_out);
            });
        if (e != hipSuccess) return e;
    }
    if (a.tol && (uint32_t)a.n > a.nsplit) {
        by_levels(a.maxl, [&](auto NL) {
            k_thin_tol_solo<decltype(NL)::value><<<(uint32_t)a.n, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.s1,
                                                                                      a.thresh, a.bound, a.keyw);
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.tol && a.nsplit) {
        if ((e = hipMemsetAsync(a.gbins, 0, sizeof(uint32_t) * kThinTolBinStride * (size_t)a.nsplit, st)) != hipSuccess)
            return e;
        by_levels(a.maxl, [&](auto NL) {
            k_thin_tol_bins<decltype(NL)::value><<<a.nitems, kLtThreads, 0, st>>>(a.desc, a.payload, a.offsets, a.items,
                                                                                 a.chunk, a.s1, a.gbins);
        });
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_thin_tol_pick<<<a.nsplit, kWave, 0, st>>>(a.desc, a.payload, a.offsets, a.split_units, a.gbins, a.thresh, a.bound,
                                                   a.keyw);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint32_t* keyw = a.budget || a.tol ? a.keyw : nullptr;  // threshold form: T = 1
    if (a.ntiles) {
        if (a.rest)
            k_pair_compact<true><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[1],
                                                              a.status[1], a.s1, a.s2, a.s3, keyw, a.out, a.rest,
                                                              a.keptw, a.restw, a.err, a.ordered);
        else
            k_pair_compact<false><<<a.ntiles, kThreads, 0, st>>>(a.desc, a.tiles, a.payload, a.offsets, a.ticket[1],
                                                               a.status[1], a.s1, a.s2, nullptr, keyw, a.out, nullptr,
                                                               a.keptw, nullptr, a.err, a.ordered);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_pair_diff<<<dim3(a.ntiles, a.rest ? 2 : 1), kThreads, 0, st>>>(a.desc, a.tiles, a.s2, a.s3, a.keptw, a.restw,
                                                                        a.out, a.rest);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    k_pair_units<<<((uint32_t)a.n + kThreads - 1) / kThreads, kThreads, 0, st>>>(
        a.desc, a.n, a.payload, a.offsets, a.keptw, a.restw, a.out, a.out_offsets, a.kept, a.rest, a.rest_offsets,
        a.rest_pairs, a.err);
    return hipGetLastError();
}

}  // namespace wc
