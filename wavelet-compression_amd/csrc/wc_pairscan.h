// wc_pairscan.h — the pair-tile scan shared by the decoders: k_rowindex and
// k_decode (wc_inverse.hip), k_decode_region (wc_region.hip).
//
// rle_decode (src/decompressor.cpp:14-30) puts pair k at flat position
// p_k = (sum of run + 1 over pairs <= k) - 1.  A workgroup takes one pair tile
// t of a unit (TILE pairs; wave w, round r, lane l holds pair t*TILE +
// w*TILE/4 + r*64 + l, loaded coalesced), sums run + 1 inside each wave on DPP
// lane moves, combines its four waves through LDS and gets the sum over the
// unit's earlier tiles from a decoupled look-back (wc_device.h lookback_sum).
//
// Which tiles run, and why no look-back waits on a tile that has left:
//   - Each kernel derives from the header alone how many tiles T of the unit
//     run (k_decode: the payload's pair tiles; k_rowindex: through the tile of
//     the virtual pair k = nrle; both: at most the tiles the plan launched for
//     the unit, which hold every pair below ncoeff whatever the surplus, so
//     that T - 1 - index never names a tile without a block or a granule;
//     k_decode_region: min(pair tiles, ceil(end /
//     TILE)): a tile t >= T has its first pair index t*TILE >= end, so every
//     pair of it and of every later tile lies at or past end).  Blocks whose
//     plan index is >= T exit after the header, before any atomic.  In the
//     ordered forms t is the plan index (or T - 1 - index, the test hook): the
//     plan interleaves tiles by index across units, so a tile's predecessors
//     have lower block ids; in the ticket form exactly T blocks draw the
//     tickets 0..T-1.  A look-back of tile t < T reads only granules of tiles
//     < t < T, all of which run; none of them belongs to a block that has left.
//   - A tile that learns from its exclusive prefix that it has nothing to write
//     still publishes its inclusive sum first (PairScan::prefix returns after
//     the publish): tiles after it (still < T) may be waiting on its granule.
//   - No further skipping.  A tile that cannot know its prefix cannot know that
//     it is past the range it writes, and leaving before publishing would make
//     its successors derive its sum from its pairs: more work, not less.
// The wait itself is lookback_sum's: after its bound a wave derives the
// predecessor's sum from that tile's pairs and publishes it (DESIGN.md §Forward
// progress), so no wait depends on which workgroups are resident.
#pragma once

#include "wc_device.h"

namespace wc {

__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { return __builtin_elementwise_add_sat(a, b); }

// wave_incl_sum32 with saturating adds (v_add_u32 clamp)
__device__ __forceinline__ uint32_t wave_incl_sum32_sat(uint32_t v) {
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false));
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false));
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false));
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false));
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false));
    v = sat_add(v, __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false));
    return v;
}

// Header check: the 20-byte header must carry the box (W, H, D), the ncoeff
// field `want` (W*H*D, or -L for a multi-level unit) and nrle >= 0.  More pairs
// than coefficients are accepted: rle_decode drops every pair whose index
// reaches ncoeff (src/decompressor.cpp:20-27), as the decoders do.  W, H, D:
// fields of a UnitDev or a RegionDesc, by reference: one still in memory is
// loaded where it is compared.
__device__ __forceinline__ bool header_ok(const int32_t& W, const int32_t& H, const int32_t& D, int32_t want,
                                          const uint8_t* __restrict__ ph, int32_t& nrle) {
    const int32_t* h = reinterpret_cast<const int32_t*>(ph);
    nrle = h[4];
    return h[0] == W && h[1] == H && h[2] == D && h[3] == want && nrle >= 0;
}

// The sum arithmetic.  T: a sum; K: a pair index; term: what a run adds.  The
// two differ on a negative run (malformed, kErrNegativeRun; the reference's
// behaviour is undefined), and each decoder keeps what it did:
//   Sat32    32-bit saturating sums, a negative run counts as run 0, so
//            positions never decrease.  Every position its users act on is
//            below ncoeff < 2^31, and a sum clamped at 2^32 - 1 is past it like
//            the exact one (k_rowindex, k_decode_region).
//   Exact64  64-bit wrapping sums, a negative run adds (int64_t)run + 1:
//            positions may step back (k_decode).
struct Sat32 {
    using T = uint32_t;
    using K = uint32_t;
    static __device__ __forceinline__ T term(int32_t run) { return run < 0 ? 1u : (uint32_t)run + 1u; }
    static __device__ __forceinline__ T add(T a, T b) { return sat_add(a, b); }
    static __device__ __forceinline__ T wave_incl(T v) { return wave_incl_sum32_sat(v); }
    static __device__ __forceinline__ T last(T s) { return __builtin_amdgcn_readlane(s, 63); }
    // an exact sum of terms (a packed chunk's, wc_packsrc.h) as the saturating adds would leave it
    static __device__ __forceinline__ T from64(uint64_t x) { return x > 0xffffffffull ? 0xffffffffu : (T)x; }
};
struct Exact64 {
    using T = uint64_t;
    using K = int64_t;
    static __device__ __forceinline__ T term(int32_t run) { return (uint64_t)(int64_t)run + 1; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T wave_incl(T v) {  // wave_incl_sum32's pattern on 64-bit values
        v += dpp_u64<0x111, 0xf>(v);  // row_shr:1
        v += dpp_u64<0x112, 0xf>(v);  // row_shr:2
        v += dpp_u64<0x114, 0xf>(v);  // row_shr:4
        v += dpp_u64<0x118, 0xf>(v);  // row_shr:8
        v += dpp_u64<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
        v += dpp_u64<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
        return v;
    }
    static __device__ __forceinline__ T last(T s) {
        // through uint32_t: the builtin returns int, and a low half with bit 31
        // set (a sum past 2^31 - 1) would sign-extend over the high half
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)s, 63);
        const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(s >> 32), 63);
        return ((uint64_t)hi << 32) | lo;
    }
    static __device__ __forceinline__ T from64(uint64_t x) { return x; }
};

// What a lane keeps of a pair: the run alone (the values stay in the payload;
// read once: nontemporal), or the whole pair.
struct LoadRuns {
    using E = uint32_t;
    template <class K>
    static __device__ __forceinline__ E load(const uint32_t* __restrict__ runs, K k) {
        // nontemporal: K5 -12 % at C2, K6r after it +1 %, C5 even (profiles/r05/experiments/gpu_nt.txt)
        return __builtin_nontemporal_load(runs + 2 * k);
    }
    static __device__ __forceinline__ E none() { return 0u; }
    static __device__ __forceinline__ int32_t run(E e) { return (int32_t)e; }
};
struct LoadPairs {
    using E = uint2;
    template <class K>
    static __device__ __forceinline__ E load(const uint32_t* __restrict__ runs, K k) {
        return reinterpret_cast<const uint2*>(runs)[k];
    }
    static __device__ __forceinline__ E none() { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ int32_t run(E e) { return (int32_t)e.x; }
};

// Where k_decode and k_decode_region take a unit's pairs from: a standard
// payload (here) or a packed unit (wc_packsrc.h PackedPairs).  open(): the
// unit's header at its offset, against the box and the standard ncoeff field
// `want`; enter(): once per block, after the tile index is known; fetch(): round
// r's load for this lane, pair k of n, and unpack(): the pair from it (the loads
// of all rounds are issued before the first is used); lim(): the pair count that round's tests
// of k < n use (a packed chunk that was refused holds no pair); tile_sum(): the
// look-back's derive path, the sum of run + 1 over tile j of the unit's n pairs by
// one wave, as tile j's own block publishes it.
struct PayloadRuns {  // the derive path alone (k_rowindex)
    const uint32_t* __restrict__ runs = nullptr;
    template <class S, int TILE>
    __device__ __forceinline__ typename S::T tile_sum(int64_t j, typename S::K n, int l) const {
        using K = typename S::K;
        const K k0 = (K)j * TILE, k1 = min(k0 + (K)TILE, n);
        typename S::T a = 0;
        for (K k = k0 + (K)l; k < k1; k += 64) a = S::add(a, S::term((int32_t)runs[2 * k]));
        return S::last(S::wave_incl(a));
    }
};
struct PayloadPairs : PayloadRuns {
    using Arg = const uint8_t* __restrict__;  // the kernel argument: the payload buffer
    static constexpr bool kLds = false;
    struct Lds;  // none
    const uint8_t* __restrict__ payload;
    __device__ __forceinline__ PayloadPairs(Arg p, uint32_t*) : payload(p) {}
    __device__ __forceinline__ bool open(uint64_t off, const int32_t& W, const int32_t& H, const int32_t& D,
                                         int32_t want, int32_t& nrle) {
        const uint8_t* ph = payload + off;
        runs = reinterpret_cast<const uint32_t*>(ph + 20);
        return header_ok(W, H, D, want, ph, nrle);
    }
    __device__ __forceinline__ void enter(uint32_t, Lds*, int, int) {}
    template <class K>
    __device__ __forceinline__ uint2 fetch(int, K k, K n, int, int) const {
        return k < n ? LoadPairs::load(runs, k) : LoadPairs::none();
    }
    __device__ __forceinline__ uint2 unpack(int, uint2 q, int, int) const { return q; }
    template <class K>
    __device__ __forceinline__ K lim(int, K n) const {
        return n;
    }
};

// The scan of one pair tile, from the tile index to the exclusive prefix known
// to all four waves.  S: Sat32 or Exact64; G: the granule form (wc_device.h
// Granule62, GranuleEpoch32); L: LoadRuns or LoadPairs.  The kernel owns the LDS
// words (s_w[4] of S::T, s_x[2] of G::V) and the place of the per-round sums.
template <class S, class G, int TILE, class L>
struct PairScan {
    using T = typename S::T;
    using K = typename S::K;
    using V = typename G::V;
    using E = typename L::E;
    static constexpr int kRounds = TILE / kThreads;

    // Tile of this block among the unit's ntiles running tiles: the plan index,
    // the reversed one (ordered 2, test hook) or the unit's next ticket
    // (ordered 0).  The caller has left already if index >= ntiles.
    static __device__ __forceinline__ uint32_t tile_index(uint32_t index, uint32_t ntiles, int ordered,
                                                          uint32_t* __restrict__ ticket, V* s_x) {
        uint32_t t = ordered == 2 ? ntiles - 1u - index : index;
        if (!ordered) {
            if (threadIdx.x == 0) s_x[0] = atomicAdd(ticket, 1u);
            __syncthreads();
            t = (uint32_t)s_x[0];
        }
        return t;
    }

    // First pair of wave w of tile t.
    static __device__ __forceinline__ K wave_first(uint32_t t, int w) { return (K)t * TILE + (K)w * (TILE / 4); }

    // Pair k of the n the payload holds, as a lane keeps it (runs: the first
    // pair's run).  The kernels write the loops over their rounds, pair
    // k = wave_first + r*64 + l in round r, and choose where the sums live
    // (no loop in here: the rounds unroll in the kernel, beside its other
    // tests of k < n).
    static __device__ __forceinline__ E load(const uint32_t* __restrict__ runs, K k, K n) {
        return k < n ? L::load(runs, k) : L::none();
    }

    // In-wave inclusive sums of run + 1 (0 past pair n) over a wave's rounds,
    // with the running wave carry.
    struct WaveSums {
        T wsum = 0;
        bool neg = false;
        // A round, pair k of this lane: the sum through it.
        __device__ __forceinline__ T round(E e, K k, K n) {
            const int32_t run = L::run(e);
            neg |= k < n && run < 0;
            const T s = S::wave_incl(k < n ? S::term(run) : (T)0);
            const T incl = S::add(wsum, s);
            wsum = S::add(wsum, S::last(s));
            return incl;
        }
        // After the last round: raises kErrNegativeRun; the wave's sum.
        __device__ __forceinline__ T finish(uint32_t* __restrict__ err) const {
            if (neg) atomicOr(err, kErrNegativeRun);
            return wsum;
        }
    };

    struct Prefix {
        V excl;   // sum over the unit's earlier tiles
        T wexcl;  // sum over this tile's earlier waves
        T tot;    // this tile's sum
    };

    // The four waves' sums through s_w; wave 0 publishes the tile's aggregate
    // at st[t], looks back over st[0..t) and publishes the inclusive prefix;
    // the result reaches every wave through s_x[1].  src: the source of the
    // unit's n pairs (PayloadRuns, PayloadPairs, or PackedPairs of wc_packsrc.h).
    template <class Src>
    static __device__ __forceinline__ Prefix prefix(T wsum, uint32_t t, K n, const Src& src, unsigned long long* st,
                                                    G g, uint32_t* __restrict__ err, T* s_w, V* s_x, int w, int l) {
        if (l == 0) s_w[w] = wsum;
        __syncthreads();
        Prefix P{0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            P.wexcl = i < w ? S::add(P.wexcl, s_w[i]) : P.wexcl;
            P.tot = S::add(P.tot, s_w[i]);
        }
        if (w == 0) {
            V excl = 0;
            if (t == 0) {
                if (l == 0) st_rlx(st, g.encode(kFlagIncl, P.tot));
            } else {
                if (l == 0) st_rlx(st + t, g.encode(kFlagAgg, P.tot));
                // a predecessor tile unpublished after the wait bound: its sum from its pairs
                excl = lookback_sum(st, (int64_t)t, l, err, g,
                                    [&](int64_t j) -> T { return src.template tile_sum<S, TILE>(j, n, l); });
                if (l == 0) st_rlx(st + t, g.encode(kFlagIncl, G::add(excl, P.tot)));
            }
            if (l == 0) s_x[1] = excl;
        }
        __syncthreads();
        P.excl = s_x[1];
        return P;
    }
};

}  // namespace wc
