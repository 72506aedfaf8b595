// wc_packsrc.h — the packed payload format on the device, shared by the
// transcoders (wc_pack.hip) and by the decoders that read packed units directly
// (k_decode<true, PackedPairs> in wc_inverse.hip, k_decode_region<*, PackedPairs>
// in wc_region.hip): the sum of a unit's width table before a tile, and
// PackedPairs, the pair source of those kernels (the interface of PayloadPairs,
// wc_pairscan.h) over a packed unit.
//
// Geometry of a decode tile over a packed unit.  The tile stays kFlatTile = 4096
// pairs = 64 chunks; wave w, round r of tile t holds chunk 64 t + 16 w + r, one
// pair per lane: exactly PairScan's lane <-> pair map wave_first + r*64 + l.  A
// chunk's place follows from the widths before it, as in k_unpack: the block
// sums the 8 t aligned 8-byte table words before its tile (block_table_sum),
// keeps its own 64 widths, and chunk c starts at
//   20 + pad8(nch) + 8 (sum of widths before c) + 64 V c;
// only the unit's last chunk is short (planes of ceil(m / 8) bytes, value
// planes of m bytes).  The table re-read grows as n^2, which is why the device
// calls keep WC_PACK_MAX_CELLS (wc_pack.hip has the arithmetic).
//
// Bounds, the contract of k_unpack.  A header is read only if its 20 bytes lie
// below the capacity and the offset is 4 (mod 8); the table only if its padded
// end does; a chunk only if its end, from the table sums, does.  A header that
// is not a packed one of the unit with the expected L, n above the cell count or
// a table past the capacity refuse the unit (open() false: nothing more of it
// is read).  Past the header a width above 31 before or inside a tile refuses
// the tile, a chunk whose end would pass the capacity refuses the chunk: a
// refused chunk counts as EMPTY (its pairs add 0 to every sum and are not
// stored), in the tile's own scan and in the sum another wave derives for it
// (tile_sum), so a refusing tile publishes the aggregate its successors would
// derive and no look-back is left waiting.  All refusals raise kErrHeader.
// Runs have at most 31 bits: a packed unit never raises kErrNegativeRun.
#pragma once

#include "wc_device.h"
#include "wc_packfmt.h"

namespace wc {

__device__ __forceinline__ uint32_t wave_or_u32_u(uint32_t v) {
    v |= dpp_u32<0x111, 0xf>(v);
    v |= dpp_u32<0x112, 0xf>(v);
    v |= dpp_u32<0x114, 0xf>(v);
    v |= dpp_u32<0x118, 0xf>(v);
    v |= dpp_u32<0x142, 0xa>(v);
    v |= dpp_u32<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

// Sum of the table bytes of the `words` 8-byte groups at `table` (8-B aligned),
// over the block; bad: some byte was above 31.  s: 8 words of LDS.
__device__ __forceinline__ uint32_t block_table_sum(const uint8_t* __restrict__ table, uint32_t words, uint32_t& bad,
                                                    uint32_t* s, int w, int l) {
    const unsigned long long* __restrict__ t = reinterpret_cast<const unsigned long long*>(table);
    uint32_t acc = 0, hi = 0;
    for (uint32_t i = threadIdx.x; i < words; i += kThreads) {
        const unsigned long long x = t[i];
        acc = __builtin_amdgcn_sad_u8((uint32_t)x, 0u, acc);
        acc = __builtin_amdgcn_sad_u8((uint32_t)(x >> 32), 0u, acc);
        hi |= (x & 0xE0E0E0E0E0E0E0E0ull) ? 1u : 0u;
    }
    acc = wave_sum_u32_u(acc);
    hi = wave_or_u32_u(hi);
    if (l == 0) {
        s[w] = acc;
        s[4 + w] = hi;
    }
    __syncthreads();
    bad = s[4] | s[5] | s[6] | s[7];
    return s[0] + s[1] + s[2] + s[3];
}

// The same sum by one wave (the look-back's derive path).
__device__ __forceinline__ uint32_t wave_table_sum(const uint8_t* __restrict__ table, uint32_t words, uint32_t& bad,
                                                   int l) {
    const unsigned long long* __restrict__ t = reinterpret_cast<const unsigned long long*>(table);
    uint32_t acc = 0, hi = 0;
    for (uint32_t i = (uint32_t)l; i < words; i += 64u) {
        const unsigned long long x = t[i];
        acc = __builtin_amdgcn_sad_u8((uint32_t)x, 0u, acc);
        acc = __builtin_amdgcn_sad_u8((uint32_t)(x >> 32), 0u, acc);
        hi |= (x & 0xE0E0E0E0E0E0E0E0ull) ? 1u : 0u;
    }
    bad = wave_or_u32_u(hi);
    return wave_sum_u32_u(acc);
}

// Plane b of a chunk of m pairs at src (pl = ceil(m / 8) bytes a plane; a full
// chunk's planes are aligned 8-byte words).
__device__ __forceinline__ unsigned long long packed_plane(const uint8_t* __restrict__ src, uint32_t b, uint32_t m,
                                                          uint32_t pl) {
    if (m == 64u) return reinterpret_cast<const unsigned long long*>(src)[b];
    unsigned long long plane = 0;
    for (uint32_t j = 0; j < pl; ++j) plane |= (unsigned long long)src[b * pl + j] << (8u * j);
    return plane;
}

// Pair source of the decoders over a packed unit (the interface of
// PayloadPairs, wc_pairscan.h).  TILE = 4096: 64 chunks a tile, 16 a wave.
struct PackedPairs {
    static constexpr int kTileChunks = kFlatTile / 64;   // 64: one width per lane of a wave
    static constexpr int kWaveChunks = kTileChunks / 4;  // 16: one chunk per round
    struct Arg {  // the kernel argument
        const uint8_t* packed;
        uint64_t cap;  // packed_capacity
    };
    static constexpr bool kLds = true;
    struct Lds {
        uint32_t red[8];           // block_table_sum
        uint32_t wd[kTileChunks];  // the tile's widths
    };

    const uint8_t* __restrict__ packed;
    uint64_t cap;  // packed_capacity: nothing at or past it is read
    uint32_t* __restrict__ err;
    // the unit, after open()
    const uint8_t* __restrict__ pk = nullptr;
    uint64_t room = 0;  // bytes of the buffer from the unit's start
    uint32_t np = 0, nch = 0, npad = 0, V = 0;  // pairs, chunks, padded table bytes, value bytes
    // the tile, after enter(): this wave's part
    uint32_t widths = 0;  // lane j: the width of the tile's chunk j
    uint32_t pre = 0;     // widths before the wave's next chunk
    uint32_t cw = 0;      // the wave's first chunk
    uint32_t live = 0;    // bit r: round r's chunk was read (uniform)
    uint2 tail = make_uint2(0u, 0u);  // the unit's short last chunk as fetch() hands it on, if this wave holds it

    __device__ __forceinline__ PackedPairs(const Arg& a, uint32_t* e) : packed(a.packed), cap(a.cap), err(e) {}

    // The unit's header at offset `off`: a packed header of the box with the
    // levels the standard ncoeff field `want` stands for (W*H*D: 1; -L: L),
    // 0 <= n <= cells, and the padded table below the capacity.
    __device__ __forceinline__ bool open(uint64_t off, const int32_t& W, const int32_t& H, const int32_t& D,
                                         int32_t want, int32_t& nrle) {
        nrle = 0;
        if ((off & 7u) != 4u || cap < 20u || off > cap - 20u) return false;
        pk = packed + off;
        const int32_t* h = reinterpret_cast<const int32_t*>(pk);
        int L = 1, v = 0;
        const int32_t n = h[4];
        if (!(h[0] == W && h[1] == H && h[2] == D && pack_header(W, H, D, h[3], L, v) && v >= 2 &&
              L == (want < 0 ? -want : 1) && n >= 0 && (uint64_t)n <= (uint64_t)W * (uint64_t)H * (uint64_t)D))
            return false;
        nch = ((uint32_t)n + 63u) >> 6;
        npad = (nch + 7u) & ~7u;
        if (npad > cap - 20u - off) return false;
        room = cap - off;
        V = (uint32_t)v;
        np = (uint32_t)n;
        nrle = n;
        return true;
    }

    // Tile t of the unit (block-uniform; holds a barrier): the sum of the table
    // before it and its own widths.
    __device__ __forceinline__ void enter(uint32_t t, Lds* s, int w, int l) {
        const uint8_t* __restrict__ table = pk + 20;
        const uint32_t c0 = t * (uint32_t)kTileChunks;
        if (threadIdx.x < (uint32_t)kTileChunks) s->wd[threadIdx.x] = c0 + threadIdx.x < nch ? table[c0 + threadIdx.x] : 0u;
        uint32_t bad;
        const uint32_t before = block_table_sum(table, c0 >> 3, bad, s->red, w, l);  // its barrier covers wd
        const int wu = __builtin_amdgcn_readfirstlane(w);
        widths = s->wd[l];
        bad |= __ballot(widths > 31u) ? 1u : 0u;
        cw = c0 + (uint32_t)wu * kWaveChunks;
        pre = before + wave_sum_u32_u(l < wu * kWaveChunks ? widths : 0u);
        live = 0;
        if (bad) {  // uniform: a width above 31 before or inside the tile: every chunk of it is empty
            if (threadIdx.x == 0) atomicOr(err, kErrHeader);
            cw = nch;
        }
        // The unit's short last chunk, in the wave that holds it: its dwords put together from its bytes here,
        // once, so that no round of fetch() waits on byte loads (the same bound as there: a chunk that would
        // pass the capacity is not read).
        const uint32_t last = nch - 1u, m = np - 64u * last;
        if (nch && m < 64u && last >= cw && last - cw < (uint32_t)kWaveChunks) {  // uniform
            const uint32_t idx = last - c0, wd = __builtin_amdgcn_readlane(widths, idx), pl = (m + 7u) >> 3;
            const uint32_t upto = before + wave_sum_u32_u((uint32_t)l < idx ? widths : 0u);
            const unsigned long long base = 20ull + npad + 8ull * upto + 64ull * V * last;
            if (base + (unsigned long long)wd * pl + (unsigned long long)V * m <= room) {
                const uint8_t* __restrict__ src = pk + base;
                const uint32_t ul = (uint32_t)l, b = ul >> 1, o = 4u * (ul & 1u);
                if (b < wd)
                    for (uint32_t j = 0; j < 4u; ++j)
                        if (o + j < pl) tail.x |= (uint32_t)src[b * pl + o + j] << (8u * j);
                const uint8_t* __restrict__ vs = src + wd * pl;
                const uint32_t p = ul >> 4, o2 = 4u * (ul & 15u);
                if (p < V)
                    for (uint32_t j = 0; j < 4u; ++j)
                        if (o2 + j < m) tail.y |= (uint32_t)vs[p * m + o2 + j] << (8u * j);
            }
        }
    }

    // Round r's chunk, as loaded (rounds in order: pre runs along; k, n as PairScan::load).  The loads of all
    // rounds are issued before the first is used (fetch for every r, then unpack for every r): the chunk's
    // place needs the widths alone.  What a lane holds: x = dword l of the run area (plane l / 2, half l % 2,
    // lanes < 2 w_c), y = dword l of the value area (plane l / 16, lanes < 16 V): one load each for a full
    // chunk; the unit's short last chunk gives the same dwords, put together from its bytes in enter().
    template <class K>
    __device__ __forceinline__ uint2 fetch(int r, K /*k*/, K n, int w, int l) {
        const uint32_t c = cw + (uint32_t)r;
        if (c >= nch) return make_uint2(0u, 0u);  // uniform: past the unit's chunks, or a refused tile
        const int wu = __builtin_amdgcn_readfirstlane(w);
        const uint32_t wd = __builtin_amdgcn_readlane(widths, wu * kWaveChunks + r);
        const unsigned long long base = 20ull + npad + 8ull * pre + 64ull * V * c;
        pre += wd;
        const uint32_t m = min(64u, (uint32_t)n - 64u * c), pl = (m + 7u) >> 3;
        if (base + (unsigned long long)wd * pl + (unsigned long long)V * m > room) {  // uniform: the chunk would pass the capacity
            if (l == 0) atomicOr(err, kErrHeader);
            return make_uint2(0u, 0u);
        }
        live |= 1u << r;
        const uint8_t* __restrict__ src = pk + base;  // 8-B aligned: the unit starts at 4 (mod 8)
        const uint32_t ul = (uint32_t)l;
        uint32_t ra = 0, va = 0;
        if (m == 64u) {  // uniform
            if (ul < 2u * wd) ra = reinterpret_cast<const uint32_t*>(src)[ul];
            if (ul < 16u * V) va = reinterpret_cast<const uint32_t*>(src + 8u * wd)[ul];
        } else {  // the unit's last chunk: enter() loaded it
            ra = tail.x;
            va = tail.y;
        }
        return make_uint2(ra, va);
    }

    // Round r's pair of this lane from what fetch() loaded: the planes transposed (bit l of plane b is bit b of
    // the lane's run), the value's top V bytes from the byte planes, the missing low bytes zero.
    __device__ __forceinline__ uint2 unpack(int r, uint2 raw, int w, int l) const {
        if (!((live >> r) & 1u)) return make_uint2(0u, 0u);  // uniform: no chunk was read
        const int wu = __builtin_amdgcn_readfirstlane(w);
        const uint32_t wd = __builtin_amdgcn_readlane(widths, wu * kWaveChunks + r);
        uint32_t run = 0;
        for (uint32_t b = 0; b < wd; ++b) {
            const uint32_t lo = __builtin_amdgcn_readlane(raw.x, 2u * b), hi = __builtin_amdgcn_readlane(raw.x, 2u * b + 1u);
            run |= (((l < 32 ? lo : hi) >> (l & 31)) & 1u) << b;
        }
        uint32_t val = 0;
        for (uint32_t p = 0; p < V; ++p) {
            const uint32_t dw = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * (16u * p + ((uint32_t)l >> 2))), (int)raw.y);
            val |= ((dw >> (8u * ((uint32_t)l & 3u))) & 0xFFu) << (8u * (3u - p));
        }
        return make_uint2(run, val);
    }

    // The pair count round r's tests of k < n use: 0 for a chunk that was not read.
    template <class K>
    __device__ __forceinline__ K lim(int r, K n) const {
        return (live >> r) & 1u ? n : (K)0;
    }

    // The sum of run + 1 over tile j's pairs, by one wave (lane l: chunk 64 j + l),
    // as tile j's own block publishes it: the look-back's derive path.  A chunk's
    // sum is m + the sum over its planes of 2^b popcount(plane b): no transpose.
    template <class S, int TILE>
    __device__ __forceinline__ typename S::T tile_sum(int64_t j, typename S::K n64, int l) const {
        static_assert(TILE == kFlatTile, "64 chunks a tile");
        const uint32_t n = (uint32_t)n64;
        const uint8_t* __restrict__ table = pk + 20;
        const uint32_t c = (uint32_t)j * (uint32_t)kTileChunks + (uint32_t)l;
        const uint32_t wd = c < nch ? table[c] : 0u;
        uint32_t bad;
        const uint32_t before = wave_table_sum(table, ((uint32_t)j * (uint32_t)kTileChunks) >> 3, bad, l);
        if (bad || __ballot(wd > 31u)) return 0;  // uniform: the tile refuses, every chunk empty
        const uint32_t excl = wave_incl_sum32(wd) - wd;
        unsigned long long sum = 0;
        if (c < nch) {
            const unsigned long long base = 20ull + npad + 8ull * (before + excl) + 64ull * V * c;
            const uint32_t m = min(64u, n - 64u * c), pl = (m + 7u) >> 3;
            if (base + (unsigned long long)wd * pl + (unsigned long long)V * m <= room) {
                const unsigned long long keep = m == 64u ? ~0ull : (1ull << m) - 1ull;  // a short chunk's unused bits are not pairs
                sum = m;
                for (uint32_t b = 0; b < wd; ++b)
                    sum += (unsigned long long)__popcll(packed_plane(pk + base, b, m, pl) & keep) << b;
            }
        }
        return S::last(S::wave_incl(S::from64(sum)));
    }
};

}  // namespace wc
