// wc_pack.hip — device transcoders of the packed payload format (wc_pack and
// wc_unpack in include/wavelet_amd.h; the format and the value rule q are
// stated there, wc_packfmt.h holds what host and device share of them).
//
// A chunk is 64 pairs, one wave: a plane of its run area is the 8 bytes of a
// wave64 ballot, a plane of its value area 64 bytes, one per lane.
//
// No workgroup waits on another.  A chunk's place in its unit follows from the
// widths of the chunks before it, and those sit in the unit's width table at a
// known place (20 bytes into the unit).  So k_pack_widths writes every table
// first, and k_pack_body, stream-ordered after it, and k_unpack each sum the
// table bytes before their tile themselves.  This is a deliberate choice over a
// decoupled look-back: it needs no per-call state, no tickets and no forward
// progress argument, at the price of the re-read below.
//
// Tile: kPackTile = 2048 pairs = 32 chunks per workgroup, 8 chunks per wave.
// Tile t of a unit reads the 32 t table bytes before it, so a unit of n pairs
// reads n^2 / (128 * 2048) table bytes in all against 8 n pair bytes: a share of
// n / 2^21 of the pair bytes.  A 64^3 unit at keep 0.999 (about 30 000 pairs):
// 1.5 %; a fully kept 64^3 unit: 12.5 %; the largest unit the device calls take
// (kPackMaxCells = 2^21, all kept: a 32-KiB table): as many table bytes as pair
// bytes, all of them hits of a 32-KiB range in L2, 8-byte loads over 256
// threads (16 loads per thread at the last tile).  A larger tile would lower the
// share further but leaves a 64^3 unit at keep 0.999 with fewer workgroups than
// it has waves to fill, so the device calls refuse units above kPackMaxCells
// instead (WC_ERR_INVALID; the host rule has no such limit).
//
// Bounds.  Pack: a unit is written only after its header is accepted, which
// includes nrle <= cells; widths are taken from runs with bit 31 cleared (a
// negative run raises kErrNegativeRun and packs as its low 31 bits), so every
// w <= 31 and the unit's bytes stay inside S(cells) (pack_worst), its slot.
// Pair loads are bounded by nrle.  Unpack: a header is read only if it lies
// below packed_capacity, the table only if its end does; a table byte above 31
// before or inside a tile refuses the tile, and a chunk is read only if its end,
// from the table sum, lies below packed_capacity.  Pairs go to 20 + 8 k of the
// unit's forward slot with k < nrle <= cells.  All refusals raise kErrHeader.
#include "wc_packsrc.h"

namespace wc {

constexpr int kPackChunks = kPackTile / 64;          // chunks per tile
constexpr int kPackWaveChunks = kPackChunks / 4;     // chunks per wave
static_assert(kPackWaveChunks == 8, "a wave's table bytes are one aligned 8-byte group");

// The source unit's header: a standard or multi-level header of the unit with
// 0 <= nrle <= cells.
__device__ __forceinline__ bool source_ok(const PackDesc& C, const uint8_t* __restrict__ ph, int& L, int32_t& nrle) {
    const int32_t* h = reinterpret_cast<const int32_t*>(ph);
    int V = 0;
    nrle = h[4];
    return h[0] == C.W && h[1] == C.H && h[2] == C.D && pack_header(C.W, C.H, C.D, h[3], L, V) && V == 0 &&
           nrle >= 0 && (uint32_t)nrle <= C.ncells;
}

// Blocks past the unit's ceil(n / kPackTile) tiles exit after reading the header.
__global__ __launch_bounds__(kThreads) void k_pack_widths(const PackDesc* __restrict__ desc,
                                                        const FTile* __restrict__ tiles,
                                                        const uint8_t* __restrict__ payload,
                                                        const uint64_t* __restrict__ offsets, int vbytes,
                                                        uint8_t* __restrict__ packed,
                                                        uint64_t* __restrict__ packed_offsets,
                                                        uint32_t* __restrict__ err) {
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const PackDesc C = desc[u];
    const uint8_t* __restrict__ ph = payload + offsets[u];
    int L = 1;
    int32_t nrle;
    const bool ok = source_ok(C, ph, L, nrle);
    if (ft.index == 0 && tid == 0) {
        packed_offsets[u] = C.pk_off;
        if (!ok) atomicOr(err, kErrHeader);
    }
    if (!ok) return;  // uniform
    const uint32_t n = (uint32_t)nrle;
    const uint32_t ntiles = n ? (n - 1u) / (uint32_t)kPackTile + 1u : 1u;
    if (ft.index >= ntiles) return;  // uniform
    uint8_t* __restrict__ pk = packed + C.pk_off;
    if (ft.index == 0 && tid < 5) {
        const int32_t* h = reinterpret_cast<const int32_t*>(ph);
        reinterpret_cast<int32_t*>(pk)[tid] = tid == 3 ? -(16 * vbytes + L) : h[tid];
    }
    const uint32_t nch = (n + 63u) >> 6, npad = (nch + 7u) & ~7u;
    const uint32_t cw = ft.index * (uint32_t)kPackChunks + (uint32_t)w * kPackWaveChunks;  // the wave's first chunk
    const uint32_t* __restrict__ pr = reinterpret_cast<const uint32_t*>(ph + 20);
    uint32_t mine = 0, neg = 0;
#pragma unroll
    for (int i = 0; i < kPackWaveChunks; ++i) {
        const uint32_t k = (cw + i) * 64u + (uint32_t)l;
        const uint32_t run = k < n ? pr[2u * k] : 0u;
        const uint32_t o = wave_or_u32_u(run);
        neg |= o >> 31;
        if (l == i) mine = 32u - (uint32_t)__clz((int)(o & 0x7FFFFFFFu));
    }
    // the wave's table bytes, the pad after the last chunk included (chunks at or past nch have no runs: 0)
    if (l < kPackWaveChunks && cw + l < npad) pk[20u + cw + l] = (uint8_t)mine;
    if (neg && l == 0) atomicOr(err, kErrNegativeRun);
}

__global__ __launch_bounds__(kThreads) void k_pack_body(const PackDesc* __restrict__ desc,
                                                      const FTile* __restrict__ tiles,
                                                      const uint8_t* __restrict__ payload,
                                                      const uint64_t* __restrict__ offsets, int vbytes, int nunits,
                                                      uint8_t* __restrict__ packed,
                                                      uint64_t* __restrict__ packed_offsets,
                                                      unsigned long long* __restrict__ packed_bytes) {
    __shared__ uint32_t s_red[8];
    __shared__ uint32_t s_w[kPackChunks];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const PackDesc C = desc[u];
    const uint8_t* __restrict__ ph = payload + offsets[u];
    int L = 1;
    int32_t nrle;
    const bool ok = source_ok(C, ph, L, nrle);
    // the unit's exact length, by the one thread that knows it; the last unit's end closes the offsets
    auto length = [&](unsigned long long bytes) {
        packed_bytes[u] = bytes;
        if ((int)u == nunits - 1) packed_offsets[nunits] = C.pk_off + bytes;
    };
    const uint32_t n = ok ? (uint32_t)nrle : 0u;
    if (n == 0u) {  // uniform: a refused unit has no packed bytes, a unit without pairs its header alone
        if (ft.index == 0 && tid == 0) length(ok ? 20ull : 0ull);
        return;
    }
    if (ft.index > (n - 1u) / (uint32_t)kPackTile) return;  // uniform
    uint8_t* __restrict__ pk = packed + C.pk_off;
    const uint8_t* __restrict__ table = pk + 20;
    const uint32_t nch = (n + 63u) >> 6, npad = (nch + 7u) & ~7u;
    const uint32_t c0 = ft.index * (uint32_t)kPackChunks;
    if (tid < kPackChunks) s_w[tid] = c0 + tid < nch ? table[c0 + tid] : 0u;
    uint32_t bad;  // not here: k_pack_widths wrote the table
    const uint32_t before = block_table_sum(table, c0 >> 3, bad, s_red, w, l);  // its barrier covers s_w
    (void)bad;
    const uint32_t V = (uint32_t)vbytes;
    // bytes of the unit before this wave's first chunk: every chunk before it is full
    uint32_t pre = before;
    for (int j = 0; j < w * kPackWaveChunks; ++j) pre += s_w[j];
    const uint32_t cw = c0 + (uint32_t)w * kPackWaveChunks;
    const uint32_t* __restrict__ pr = reinterpret_cast<const uint32_t*>(ph + 20);
    for (int i = 0; i < kPackWaveChunks; ++i) {
        const uint32_t c = cw + i;
        if (c >= nch) break;  // uniform
        const uint32_t wd = __builtin_amdgcn_readfirstlane(s_w[w * kPackWaveChunks + i]);
        const unsigned long long base = 20ull + npad + 8ull * pre + 64ull * V * c;
        pre += wd;
        const uint32_t m = min(64u, n - 64u * c), k = 64u * c + (uint32_t)l;
        const bool valid = (uint32_t)l < m;
        const uint32_t run = valid ? pr[2u * k] & 0x7FFFFFFFu : 0u;
        const uint32_t q = pack_value(valid ? pr[2u * k + 1u] : 0u, vbytes);
        unsigned long long plane = 0;
        for (uint32_t b = 0; b < wd; ++b) {
            const unsigned long long bal = __ballot((run >> b) & 1u);
            if ((uint32_t)l == b) plane = bal;
        }
        uint8_t* __restrict__ dst = pk + base;  // 8-B aligned: the unit starts at 4 (mod 8)
        if (m == 64u) {
            if ((uint32_t)l < wd) reinterpret_cast<unsigned long long*>(dst)[l] = plane;
            uint8_t* __restrict__ vd = dst + 8u * wd;
            for (uint32_t p = 0; p < V; ++p) vd[p * 64u + l] = (uint8_t)(q >> (8u * (3u - p)));
            if (c == nch - 1u && l == 0) length(base + 8ull * wd + 64ull * V);
        } else {  // the unit's last chunk: planes of ceil(m / 8) bytes, value planes of m bytes
            const uint32_t pl = (m + 7u) >> 3;
            if ((uint32_t)l < wd)
                for (uint32_t j = 0; j < pl; ++j) dst[l * pl + j] = (uint8_t)(plane >> (8u * j));
            uint8_t* __restrict__ vd = dst + wd * pl;
            if (valid)
                for (uint32_t p = 0; p < V; ++p) vd[p * m + l] = (uint8_t)(q >> (8u * (3u - p)));
            if (l == 0) length(base + (unsigned long long)wd * pl + (unsigned long long)V * m);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_unpack(const PackDesc* __restrict__ desc,
                                                   const FTile* __restrict__ tiles,
                                                   const uint8_t* __restrict__ packed,
                                                   const uint64_t* __restrict__ packed_offsets, uint64_t cap,
                                                   int nunits, uint8_t* __restrict__ payload,
                                                   uint64_t* __restrict__ offsets, uint32_t* __restrict__ kept,
                                                   uint32_t* __restrict__ err) {
    __shared__ uint32_t s_red[8];
    __shared__ uint32_t s_w[kPackChunks];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FTile ft = tiles[blockIdx.x];
    const uint32_t u = ft.unit;
    const PackDesc C = desc[u];
    const uint64_t off = packed_offsets[u];
    int L = 1, V = 0;
    uint32_t n = 0, nch = 0, npad = 0;
    bool ok = (off & 7u) == 4u && cap >= 20u && off <= cap - 20u;
    const uint8_t* __restrict__ pk = packed + (ok ? off : 0u);
    if (ok) {
        const int32_t* h = reinterpret_cast<const int32_t*>(pk);
        const int32_t nrle = h[4];
        ok = h[0] == C.W && h[1] == C.H && h[2] == C.D && pack_header(C.W, C.H, C.D, h[3], L, V) && V >= 2 &&
             nrle >= 0 && (uint32_t)nrle <= C.ncells;
        if (ok) {
            n = (uint32_t)nrle;
            nch = (n + 63u) >> 6;
            npad = (nch + 7u) & ~7u;
            ok = npad <= cap - 20u - off;  // the table lies below the capacity
        }
    }
    if (!ok) n = 0;
    if (ft.index == 0 && tid == 0) {
        offsets[u] = C.pay_off;
        kept[u] = n;
        if ((int)u == nunits - 1) offsets[nunits] = C.pay_off + 20u + 8ull * n;
        if (!ok) atomicOr(err, kErrHeader);
    }
    if (!ok) return;  // uniform
    uint8_t* __restrict__ out = payload + C.pay_off;
    if (ft.index == 0 && tid < 5) {
        const int32_t* h = reinterpret_cast<const int32_t*>(pk);
        reinterpret_cast<int32_t*>(out)[tid] = tid == 3 ? (L >= 2 ? -L : (int32_t)C.ncells) : h[tid];
    }
    if (n == 0u || ft.index > (n - 1u) / (uint32_t)kPackTile) return;  // uniform
    const uint8_t* __restrict__ table = pk + 20;
    const uint32_t c0 = ft.index * (uint32_t)kPackChunks;
    if (tid < kPackChunks) s_w[tid] = c0 + tid < nch ? table[c0 + tid] : 0u;
    uint32_t bad;
    const uint32_t before = block_table_sum(table, c0 >> 3, bad, s_red, w, l);  // its barrier covers s_w
    for (int j = 0; j < kPackChunks; ++j) bad |= s_w[j] > 31u ? 1u : 0u;
    if (bad) {  // uniform: a width above 31 before or inside the tile
        if (tid == 0) atomicOr(err, kErrHeader);
        return;
    }
    uint32_t pre = before;
    for (int j = 0; j < w * kPackWaveChunks; ++j) pre += s_w[j];
    const uint32_t cw = c0 + (uint32_t)w * kPackWaveChunks;
    const uint64_t room = cap - off;  // bytes of the buffer from the unit's start
    for (int i = 0; i < kPackWaveChunks; ++i) {
        const uint32_t c = cw + i;
        if (c >= nch) break;  // uniform
        const uint32_t wd = __builtin_amdgcn_readfirstlane(s_w[w * kPackWaveChunks + i]);
        const unsigned long long base = 20ull + npad + 8ull * pre + 64ull * (uint32_t)V * c;
        pre += wd;
        const uint32_t m = min(64u, n - 64u * c), k = 64u * c + (uint32_t)l, pl = (m + 7u) >> 3;
        if (base + (unsigned long long)wd * pl + (unsigned long long)V * m > room) {  // uniform: the chunk would pass the capacity
            if (l == 0) atomicOr(err, kErrHeader);
            break;
        }
        const bool valid = (uint32_t)l < m;
        const uint8_t* __restrict__ src = pk + base;
        unsigned long long plane = 0;
        if ((uint32_t)l < wd) {
            if (m == 64u)
                plane = reinterpret_cast<const unsigned long long*>(src)[l];
            else
                for (uint32_t j = 0; j < pl; ++j) plane |= (unsigned long long)src[l * pl + j] << (8u * j);
        }
        const uint32_t plo = (uint32_t)plane, phi = (uint32_t)(plane >> 32);
        uint32_t run = 0;
        for (uint32_t b = 0; b < wd; ++b) {
            const uint32_t lo = __builtin_amdgcn_readlane(plo, b), hi = __builtin_amdgcn_readlane(phi, b);
            run |= (((l < 32 ? lo : hi) >> (l & 31)) & 1u) << b;
        }
        const uint8_t* __restrict__ vs = src + wd * pl;
        uint32_t val = 0;
        if (valid)
            for (int p = 0; p < V; ++p) val |= (uint32_t)vs[(uint32_t)p * m + l] << (8 * (3 - p));
        if (valid) *reinterpret_cast<uint2*>(out + 20u + 8ull * k) = make_uint2(run, val);
    }
}

// The _host forms pack the slots densely before the copy back, as wc_forward_host
// does (wc_compact.hip): unit u's bytes (STD: 20 + 8 * kept[u] of a standard
// payload, else bytes[u] of a packed unit) move from src_off[u] to dense[u],
// dense[0] = 4 and every dense[u] == 4 (mod 8); dense[n] = the end of the last
// unit's bytes.
template <bool STD>
__device__ __forceinline__ uint64_t dense_bytes(const unsigned long long* bytes, const uint32_t* kept, int u) {
    return STD ? 20u + 8ull * kept[u] : bytes[u];
}

template <bool STD>
__global__ __launch_bounds__(1024) void k_dense_offsets(int n, const unsigned long long* __restrict__ bytes,
                                                      const uint32_t* __restrict__ kept,
                                                      uint64_t* __restrict__ dense) {
    __shared__ uint64_t s_w[16];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t carry = 4;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int u = c0 + threadIdx.x;
        const bool ok = u < n;
        const uint64_t b = ok ? dense_bytes<STD>(bytes, kept, u) : 0;
        const uint64_t sz = !ok ? 0 : STD ? b + 4 : ((b + 7) & ~uint64_t(7));  // STD: 24 + 8 * kept, as wc_forward_host
        uint64_t incl = sz;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint64_t t = __shfl_up(incl, o);
            if (l >= o) incl += t;
        }
        if (l == 63) s_w[w] = incl;
        __syncthreads();
        uint64_t wb = 0, tot = 0;
        for (int i = 0; i < 16; ++i) {
            if (i < w) wb += s_w[i];
            tot += s_w[i];
        }
        __syncthreads();
        if (ok) {
            const uint64_t off = carry + wb + incl - sz;
            dense[u] = off;
            if (u == n - 1) dense[n] = off + b;
        }
        carry += tot;
    }
}

constexpr int kDenseParts = 8;  // workgroups per unit of the dense copy

template <bool STD>
__global__ __launch_bounds__(kThreads) void k_dense_copy(const unsigned long long* __restrict__ bytes,
                                                       const uint32_t* __restrict__ kept,
                                                       const uint64_t* __restrict__ src_off,
                                                       const uint8_t* __restrict__ src,
                                                       const uint64_t* __restrict__ dense,
                                                       uint8_t* __restrict__ dst) {
    const int u = blockIdx.x;
    const uint64_t b = dense_bytes<STD>(bytes, kept, u);
    const uint64_t words = b >> 2;  // both ends are 4-B aligned; a packed unit's last 1..3 bytes follow
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + src_off[u]);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + dense[u]);
    for (uint64_t i = (uint64_t)blockIdx.y * kThreads + threadIdx.x; i < words; i += (uint64_t)kDenseParts * kThreads)
        d[i] = s[i];
    if (blockIdx.y == 0 && threadIdx.x < (b & 3))
        dst[dense[u] + 4 * words + threadIdx.x] = src[src_off[u] + 4 * words + threadIdx.x];
}

hipError_t launch_dense(hipStream_t st, bool standard, int n, const uint64_t* bytes, const uint32_t* kept,
                        const uint64_t* src_off, const uint8_t* src, uint64_t* dense, uint8_t* dst) {
    if (!n) return hipSuccess;
    const unsigned long long* by = (const unsigned long long*)bytes;
    if (standard) {
        k_dense_offsets<true><<<1, 1024, 0, st>>>(n, by, kept, dense);
        k_dense_copy<true><<<dim3(n, kDenseParts), kThreads, 0, st>>>(by, kept, src_off, src, dense, dst);
    } else {
        k_dense_offsets<false><<<1, 1024, 0, st>>>(n, by, kept, dense);
        k_dense_copy<false><<<dim3(n, kDenseParts), kThreads, 0, st>>>(by, kept, src_off, src, dense, dst);
    }
    return hipGetLastError();
}

hipError_t launch_pack_units(hipStream_t st, const PackDesc* desc, const FTile* tiles, uint32_t ntiles,
                             const uint8_t* payload, const uint64_t* offsets, int vbytes, int n, uint8_t* packed,
                             uint64_t* packed_offsets, uint64_t* packed_bytes, uint32_t* err) {
    if (!ntiles) return hipSuccess;
    k_pack_widths<<<ntiles, kThreads, 0, st>>>(desc, tiles, payload, offsets, vbytes, packed, packed_offsets, err);
    k_pack_body<<<ntiles, kThreads, 0, st>>>(desc, tiles, payload, offsets, vbytes, n, packed, packed_offsets,
                                            (unsigned long long*)packed_bytes);
    return hipGetLastError();
}

hipError_t launch_unpack_units(hipStream_t st, const PackDesc* desc, const FTile* tiles, uint32_t ntiles,
                               const uint8_t* packed, const uint64_t* packed_offsets, uint64_t cap, int n,
                               uint8_t* payload, uint64_t* offsets, uint32_t* kept, uint32_t* err) {
    if (!ntiles) return hipSuccess;
    k_unpack<<<ntiles, kThreads, 0, st>>>(desc, tiles, packed, packed_offsets, cap, n, payload, offsets, kept, err);
    return hipGetLastError();
}

}  // namespace wc
