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
// k_decode_corner runs the decoders' shared pair-tile scan (wc_pairscan.h
// PairScan, which also owns the rule for which tiles run and why no look-back
// waits on a tile that has left) over zeroed 62-bit granules.  Sums are Sat32,
// as in k_rowindex: every position this kernel acts on is below end <= W*H*D <
// 2^31, and a saturated sum is past it like the exact one; a negative run counts
// as run 0, so pair k lands at a position >= k.  The unit's tiles are [0, T),
// T = min(pair tiles of the payload, ceil(end / kFlatTile)); a tile t < T whose
// exclusive prefix turns out >= end has published its inclusive sum by then and
// skips the scatter.
//
// Bounds: a pair is stored only if its position p < end and its (I, J, K) from
// p lies inside (w, h, d), so every store is inside the unit's w*h*d elements
// at dst_off, whatever the payload holds; pair loads are bounded by the header's
// pair count, as in k_decode.
#include "wc_pairscan.h"

namespace wc {

// tiles: the decode tiles of the plan of the FULL units (interleaved by tile
// index across units; a prefix of that list: every tile index below the
// batch's largest ceil(end / kFlatTile)).  bad[u] (written by the unit's first
// tile, read by later launches): kUnitRefused = the header disagrees
// (kErrHeader; nothing past the header is read, no cell is written, every later
// launch skips the unit); kUnitBox = r == L (k_corner_box writes the cells, the
// level passes and the inverse skip the unit); kUnitRun otherwise.
__global__ __launch_bounds__(kThreads) void k_decode_corner(const CornerDesc* __restrict__ desc,
                                                          const FTile* __restrict__ tiles,
                                                          const uint8_t* __restrict__ payload,
                                                          const uint64_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ ticket,
                                                          unsigned long long* __restrict__ status,
                                                          float* __restrict__ corner,
                                                          uint32_t* __restrict__ err, int ordered,
                                                          uint32_t* __restrict__ bad) {
    using Scan = PairScan<Sat32, Granule62, kFlatTile, LoadPairs>;
    __shared__ Scan::T s_w[4];
    __shared__ Scan::V s_x[2];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const CornerDesc C = desc[u];
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
    const uint32_t T = min(ptiles, (C.end - 1u) / (uint32_t)kFlatTile + 1u);  // end >= 1: the unit has cells
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
    if (A >= (uint64_t)C.end) return;  // uniform: the whole tile is past the corner (its sum is published)

    // 3. the pairs inside the corner, to their compact places
    float* __restrict__ dst = corner + C.dst_off;
    const uint64_t base = A + P.wexcl;  // + incl[r] - 1: position of the lane's pair in round r
#pragma unroll
    for (int r = 0; r < Scan::kRounds; ++r) {
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
    if (bad[ft.unit] != kUnitBox) return;  // uniform
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
