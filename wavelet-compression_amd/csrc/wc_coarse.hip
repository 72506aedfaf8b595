// wc_coarse.hip — corner decode of the reduced-resolution inverse
// (wc_inverse_coarse in include/wavelet_amd.h).
//
// Not part of the reference's codec.  A unit W x H x D with L levels and a
// reduction r needs only the low-pass corner (w, h, d) = (W, H, D) >> r of its
// flat array A (x-slowest order (I*H + J)*D + K): the synthesis of level l
// touches only the corner (W, H, D) >> (l - 1), so levels L..r+1 act on that
// corner exactly as levels L-r..1 act on a w x h x d unit.  k_decode_corner
// turns a payload's pairs into the compact corner C[(I*h + J)*d + K] in the
// coefficient scratch, at the place the plan of the derived units (w, h, d)
// gives it; k_level<false>, k_level_copy and k_inverse{,_fast} then run
// unchanged on those derived units.  A unit with r == L has nothing left to
// run: its corner IS the result, and k_corner_box copies it to its Box3D place
// out[I + w*(J + h*K)].  Nothing of size W*H*D is written or read.
//
//   k_decode_corner  pair tiles -> the corner's coefficients (scattered 4-B
//                    stores, neighbours in K side by side; the zeros between
//                    them come from a memset of the compact scratch before)
//   k_corner_box     units with r == L: compact corner -> Box3D cells, 32 x 32
//                    (I, K) tiles through LDS so that both sides move whole
//                    rows.  (Scattering the pairs straight into Box3D order
//                    was measured first: neighbouring K are w*h cells apart
//                    there, one store per cache line, and the decode of the
//                    one-level C2 payloads took 0.55 ms against 0.17 ms into
//                    the compact order.)
//
// k_decode_corner keeps k_decode's structure (wc_inverse.hip): pair tile t
// (kFlatTile pairs; wave w, round r, lane l holds pair t*kFlatTile + w*1024 +
// r*64 + l), in-wave DPP scans of run + 1, the sum over the unit's earlier
// tiles from a decoupled look-back over zeroed 62-bit granules, the tile index
// from the launch order or a per-unit ticket (WC_OPT_ORDERED).  Sums are
// 32-bit and saturate, as in k_rowindex: every position this kernel acts on is
// below end <= W*H*D < 2^31, and a saturated sum is past it like the exact one.
// A negative run (malformed, kErrNegativeRun) counts as run 0, so positions
// never decrease: pair k lands at a position >= k.
//
// Which tiles run, and why no look-back waits on a tile that has left:
//   - The unit's tiles are [0, T), T = min(pair tiles of the payload,
//     ceil(end / kFlatTile)): a tile t >= T has its first pair index
//     t*kFlatTile >= end (or no pair at all), so every pair of it and of every
//     later tile lies at or past end.  Blocks whose plan index is >= T exit
//     after the header, before any atomic, exactly as k_decode's blocks past
//     the payload's pair tiles do: in the ordered forms t is the plan index (or
//     T - 1 - index), in the ticket form exactly T blocks draw the tickets
//     0..T-1.  A look-back of tile t < T reads only granules of tiles < t < T,
//     all of which run; none of them belongs to a block that has left.
//   - A tile t < T whose exclusive prefix turns out >= end still publishes its
//     inclusive sum, then skips the scatter: tiles after it (still < T) may be
//     waiting on its granule.
//   - No further skipping.  A tile that cannot know its prefix cannot know that
//     it is past the corner, and leaving before publishing would make its
//     successors derive its sum from its pairs: more work, not less.
// The wait itself is lookback_sum62's: after its bound a wave derives the
// predecessor's sum from that tile's pairs and publishes it (DESIGN.md §Forward
// progress), so no wait depends on which workgroups are resident.
//
// Bounds: a pair is stored only if its position p < end and its (I, J, K) from
// p lies inside (w, h, d), so every store is inside the unit's w*h*d elements
// at dst_off, whatever the payload holds; pair loads are bounded by the header's
// pair count, as in k_decode.
#include "wc_device.h"

namespace wc {

constexpr int kCornerRounds = kFlatTile / kThreads;  // 16 pairs per lane

__device__ __forceinline__ uint32_t sat_add32(uint32_t a, uint32_t b) { return __builtin_elementwise_add_sat(a, b); }

// wave_incl_sum32 with saturating adds (wc_inverse.hip wave_incl_sum32_sat)
__device__ __forceinline__ uint32_t wave_incl_sum32_sat_c(uint32_t v) {
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false));
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false));
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false));
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false));
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false));
    v = sat_add32(v, __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false));
    return v;
}

// The header must carry the unit's box and its levels (ncoeff = -L for L >= 2)
// and nrle >= 0, as read_header of wc_inverse.hip asks for wc_inverse_levels.
__device__ __forceinline__ bool corner_header(const CornerDesc& C, const uint8_t* __restrict__ ph, int32_t& nrle) {
    const int32_t* h = reinterpret_cast<const int32_t*>(ph);
    nrle = h[4];
    return h[0] == C.W && h[1] == C.H && h[2] == C.D && h[3] == C.want && nrle >= 0;
}

// tiles: the decode tiles of the plan of the FULL units (interleaved by tile
// index across units; a prefix of that list: every tile index below the
// batch's largest ceil(end / kFlatTile)).  bad[u] (written by the unit's first
// tile, read by later launches): kCornerRefused = the header disagrees
// (kErrHeader; nothing past the header is read, no cell is written, every later
// launch skips the unit); kCornerBox = r == L (k_corner_box writes the cells, the
// level passes and the inverse skip the unit); kCornerRun otherwise.
__global__ __launch_bounds__(kThreads) void k_decode_corner(const CornerDesc* __restrict__ desc,
                                                          const FTile* __restrict__ tiles,
                                                          const uint8_t* __restrict__ payload,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ ticket,
                                                          unsigned long long* __restrict__ status,
                                                          float* __restrict__ corner,
                                                          uint32_t* __restrict__ err, int ordered,
                                                          uint32_t* __restrict__ bad) {
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const CornerDesc C = desc[u];
    const uint8_t* ph = payload + offsets[u];
    int32_t nrle;
    const bool hok = corner_header(C, ph, nrle);
    if (ft.index == 0 && tid == 0) {
        bad[u] = !hok ? kCornerRefused : C.direct ? kCornerBox : kCornerRun;
        if (!hok) atomicOr(err, kErrHeader);
    }
    if (!hok) return;  // uniform
    const uint32_t n = (uint32_t)nrle;
    const uint32_t ptiles = n ? (n - 1u) / (uint32_t)kFlatTile + 1u : 1u;
    const uint32_t T = min(ptiles, (C.end - 1u) / (uint32_t)kFlatTile + 1u);  // end >= 1: the unit has cells
    if (ft.index >= T) return;  // uniform; before any atomic
    uint32_t t = ordered == 2 ? T - 1u - ft.index : ft.index;  // 2: reversed (test hook)
    if (!ordered) {
        if (tid == 0) s_x[0] = atomicAdd(ticket + u, 1u);
        __syncthreads();
        t = (uint32_t)s_x[0];
    }

    // 1. this lane's pairs and the saturating in-wave inclusive sums of (run + 1)
    const uint2* __restrict__ pr = reinterpret_cast<const uint2*>(ph + 20);
    const uint32_t kw = t * (uint32_t)kFlatTile + (uint32_t)w * (kFlatTile / 4);
    uint2 q[kCornerRounds];
#pragma unroll
    for (int r = 0; r < kCornerRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        q[r] = k < n ? pr[k] : make_uint2(0u, 0u);
    }
    uint32_t incl[kCornerRounds];
    uint32_t wsum = 0;
    bool neg = false;
#pragma unroll
    for (int r = 0; r < kCornerRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        const int32_t run = (int32_t)q[r].x;
        neg |= k < n && run < 0;
        const uint32_t x = k < n ? (run < 0 ? 1u : (uint32_t)run + 1u) : 0u;
        const uint32_t s = wave_incl_sum32_sat_c(x);
        incl[r] = sat_add32(wsum, s);
        wsum = sat_add32(wsum, __builtin_amdgcn_readlane(s, 63));
    }
    if (neg) atomicOr(err, kErrNegativeRun);
    if (l == 0) s_w[w] = wsum;
    __syncthreads();
    uint32_t wexcl = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wexcl = i < w ? sat_add32(wexcl, s_w[i]) : wexcl;
        tot = sat_add32(tot, s_w[i]);
    }

    // 2. the sum over the unit's earlier tiles: look-back
    if (w == 0) {
        unsigned long long* st = status + C.dt_begin;
        unsigned long long excl = 0;
        if (t == 0) {
            if (l == 0) st_rlx(st, kFlagIncl | (unsigned long long)tot);
        } else {
            if (l == 0) st_rlx(st + t, kFlagAgg | (unsigned long long)tot);
            // a predecessor tile unpublished after the wait bound: its sum from its pairs
            excl = lookback_sum62(st, (int64_t)t, l, err, [&](int64_t j) -> unsigned long long {
                const uint32_t k0 = (uint32_t)j * (uint32_t)kFlatTile, k1 = min(k0 + (uint32_t)kFlatTile, n);
                uint32_t a = 0;
                for (uint32_t k = k0 + (uint32_t)l; k < k1; k += 64) {
                    const int32_t run = (int32_t)pr[k].x;
                    a = sat_add32(a, run < 0 ? 1u : (uint32_t)run + 1u);
                }
                return (unsigned long long)__builtin_amdgcn_readlane(wave_incl_sum32_sat_c(a), 63);
            });
            if (l == 0) st_rlx(st + t, kFlagIncl | ((excl + tot) & kMask62));
        }
        if (l == 0) s_x[1] = excl;
    }
    __syncthreads();
    const uint64_t A = s_x[1];  // positions before this tile's first pair
    if (A >= (uint64_t)C.end) return;  // uniform: the whole tile is past the corner (its sum is published)

    // 3. the pairs inside the corner, to their compact places
    float* __restrict__ dst = corner + C.dst_off;
    const uint64_t base = A + wexcl;  // + incl[r] - 1: position of the lane's pair in round r
#pragma unroll
    for (int r = 0; r < kCornerRounds; ++r) {
        const uint32_t k = kw + r * 64 + l;
        const uint64_t p64 = base + incl[r] - 1u;  // incl >= 1 where k < n
        if (k >= n || p64 >= (uint64_t)C.end) continue;
        const uint32_t p = (uint32_t)p64;  // < end <= W*H*D < 2^31
        const uint32_t row = div_rows(p, C.dmagic), K = p - row * (uint32_t)C.D;
        const uint32_t I = div_rows(row, C.hmagic), J = row - I * (uint32_t)C.H;
        if (I >= C.w || J >= C.h || K >= C.d) continue;
        dst[(I * C.h + J) * C.d + K] = __uint_as_float(q[r].y);
    }
}

// tiles: the flat tiles (kFlatTile cells) of the plan of the DERIVED units:
// block (u, i) of a unit with r == L whose header agreed takes the unit's
// transposition tiles i, i + nft, ... (nft = the unit's flat tiles), a tile
// being 32 I x 32 K at one J: rows of K are contiguous in the compact corner,
// rows of I in the Box3D.  Every cell of the unit is written (the zeros of the
// cleared scratch included); a refused unit keeps its cells.
constexpr int kBoxTile = 32;
__global__ __launch_bounds__(kThreads) void k_corner_box(const CornerDesc* __restrict__ desc,
                                                       const FTile* __restrict__ tiles,
                                                       const float* __restrict__ corner, float* __restrict__ out,
                                                       const uint32_t* __restrict__ bad) {
    __shared__ float tile[kBoxTile][kBoxTile + 1];
    const FTile ft = tiles[blockIdx.x];
    if (bad[ft.unit] != kCornerBox) return;  // uniform
    const CornerDesc C = desc[ft.unit];
    const uint32_t w = C.w, h = C.h, d = C.d;
    const uint32_t ti = (w + kBoxTile - 1) / kBoxTile, tk = (d + kBoxTile - 1) / kBoxTile;
    const uint32_t ntiles = h * ti * tk;
    const uint32_t nft = (w * h * d + (uint32_t)kFlatTile - 1) / (uint32_t)kFlatTile;
    const float* __restrict__ src = corner + C.dst_off;
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

hipError_t launch_decode_corner(hipStream_t st, const CornerDesc* desc, const FTile* dtiles, uint32_t ndt,
                                const uint8_t* payload, const uint64_t* offsets, uint32_t* ticket,
                                unsigned long long* status, float* corner, uint32_t* err, int ordered, uint32_t* bad) {
    if (ndt)
        k_decode_corner<<<ndt, kThreads, 0, st>>>(desc, dtiles, payload, offsets, ticket, status, corner, err, ordered,
                                                  bad);
    return hipGetLastError();
}

hipError_t launch_corner_box(hipStream_t st, const CornerDesc* desc, const FTile* ftiles, uint32_t nft,
                             const float* corner, float* out, const uint32_t* bad) {
    if (nft) k_corner_box<<<nft, kThreads, 0, st>>>(desc, ftiles, corner, out, bad);
    return hipGetLastError();
}

}  // namespace wc
