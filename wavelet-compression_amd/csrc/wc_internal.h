// wc_internal.h — device-side plan structures shared by the HIP kernels and
// the C-ABI host code.  Not part of the public boundary (include/wavelet_amd.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wc {

constexpr int kThreads = 256;          // 4 waves of 64 lanes
constexpr int kWave = 64;
constexpr int kMaxTileBlocks = 1024;   // 2x2x2 blocks per transform tile (8192 coefficients)
constexpr int kFlatTile = 4096;        // coefficients per threshold/compaction tile
constexpr int kFlatPerThread = kFlatTile / kThreads;  // 16 = 4 x float4

// One Box3D component in the batch, with its transform tiling.
// Blocks: the reference's axis sweeps pair (2b, 2b+1) on every axis
// (src/compressor.cpp:107-111), so coefficient (I,J,K) depends only on the
// 2x2x2 input block (I mod h, J mod h, K mod h); an odd axis adds one
// pass-through "tail" block at b = n/2.
struct UnitDev {
    uint64_t cell_off;   // element offset of the unit's cells
    uint64_t coef_off;   // element offset in the flat coefficient scratch (128-B aligned)
    uint64_t ncells;     // W*H*D
    int32_t nx, ny, nz;  // W, H, D
    int32_t hx, hy, hz;  // n/2 per axis (number of pairs)
    int32_t nbx, nby, nbz;  // blocks per axis = ceil(n/2)
    int32_t lbx, lby, lbz;  // log2 of the transform tile shape in blocks
    uint32_t ftile_begin;   // first flat tile (kFlatTile) of this unit: staged forward, decode, RMSE
    uint32_t nftiles;       // number of flat tiles = ceil(ncells / kFlatTile)
    uint64_t pay_off;       // payload slot: prefix of worst-case sizes, == 4 (mod 8)
    int32_t ntz;            // z tiles per unit
    int32_t fast;           // 1: even dims, D % 8 == 0 -> the fast transform body
    uint32_t ntx;           // transform tiles of the unit
    uint32_t xt_begin;      // first transform tile of the unit in the plan's tile list
    uint32_t et_begin;      // first emit tile (kEmitTile coefficients) of the unit
    uint32_t net;           // emit tiles = max(1, ceil(ncells / kEmitTile))
    uint32_t sparse;        // 1: staged forward stores only flagged 32-coefficient segments (wc_xform.h)
    // inverse (wc_inverse.hip)
    uint32_t dt_begin;      // first decode tile (kFlatTile pairs) of the unit: look-back status index
    uint32_t ndt;           // decode tiles launched for the unit
    int32_t rix;            // 1: row-indexed inverse (K5 row index + K6r), 0: dense flat scratch
    int32_t ilbx, ilby;     // log2 of K6r's tile in blocks along x and y (all of z)
    uint64_t row_off;       // first rowinfo entry of the unit (W*H + 1 entries)
    uint32_t rt_begin;      // first K6r tile of the unit (row-indexed units)
    uint32_t nrt;           // K6r tiles of the unit
    uint64_t dmagic;        // m | (31 + l) << 32: row = floor(position / D) = (position * m) >> (31 + l)
    uint64_t flag_off;      // sparse units: byte offset of the segment flags (whole 2048-coefficient blocks, flag_pos)
};

// A transform tile: a (1<<lbx) x (1<<lby) x (1<<lbz) box of 2x2x2 blocks.
struct XTile {
    uint32_t unit;
    uint32_t bx0, by0, bz0;
};

// A K6r tile (row-indexed inverse, wc_inverse.hip): everything the kernel
// needs about the tile and its unit in one record (one scalar load batch).
struct RTile {
    uint64_t row_off;   // the unit's first rowinfo entry
    uint64_t cell_off;  // the unit's first output cell
    uint32_t unit;
    int32_t bx0, by0;   // first block of the tile along x and y (all of z)
    int32_t W, H, D;
    int32_t lbx, lby;   // log2 of the tile's blocks along x and y
    int32_t tyv;        // blocks along y in this tile (<= 1 << lby at the unit's edge)
    uint32_t nat;       // index in unit order (the fused RMSE's partial-sum slot)
};

// LDS layout of a K6r tile: 4 wave regions of TX ranges of RS = TY*D + 4
// floats, regions 16 floats apart (bank offset), 16-B aligned.
#ifndef WC_RIX_RSPAD
#define WC_RIX_RSPAD 4   // floats between ranges (bank offset)
#endif
#ifndef WC_RIX_WRPAD
#define WC_RIX_WRPAD 16  // floats between wave regions
#endif
__host__ __device__ inline int rix_rs(int lby, int D) { return (D << lby) + WC_RIX_RSPAD; }
__host__ __device__ inline int rix_wr(int lbx, int lby, int D) { return (rix_rs(lby, D) << lbx) + WC_RIX_WRPAD; }

// A flat tile: kFlatTile consecutive coefficients (flat order) of one unit.
struct FTile {
    uint32_t unit;
    uint32_t index;  // tile index within the unit
};

// One unit of the reduced-resolution and of the sub-box decode (wc_region.hip
// k_decode_region): the payload's box, the primed unit (w, h, d) = (W, H, D) >> r
// with L' = L - r levels, and the region's origin and extent in cells of that
// resolution (wc_regionmap.h).  wc_inverse_coarse's region is the whole primed
// box: o = 0, s = (w, h, d).  Built per call (neither the reduce nor the region
// is part of a plan).
struct RegionDesc {
    uint64_t dst_off;      // element offset of the compact unit in the coefficient scratch (the derived unit's coef_off)
    uint64_t out_off;      // the unit's first output cell
    uint64_t dmagic;       // div_rows magic of D: row = floor(position / D)
    uint64_t hmagic;       // div_rows magic of H: I = floor(row / H)
    int32_t W, H, D;       // the payload's box
    int32_t want;          // the header's ncoeff field: W*H*D, or -L for L >= 2
    uint32_t w, h, d;      // the primed box
    uint32_t L;            // L' = L - r
    uint32_t ox, oy, oz;   // the region's origin >> r
    uint32_t sx, sy, sz;   // the region's extent >> r: the compact unit
    uint32_t end;          // no needed pair at or past this flat position: region_end, or of the whole primed box
                           // ((w-1)*H + (h-1))*D + d; 0: the region has no cells
    uint32_t dt_begin;     // the unit's first look-back granule
    uint32_t direct;       // 1: L' = 0, the compact unit is the result: k_corner_box copies it out, no pass or inverse runs
    uint32_t pad;
};
static_assert(sizeof(RegionDesc) == 104, "descriptor of 8-B members first");

// One unit of the multi-level RMSE-tolerance mode (wc_leveltol.hip).  Built per
// call: the levels and tolerances are not part of a plan.
struct LtUnit {
    uint64_t dmagic;  // div_rows magic of D: row = floor(position / D)
    uint64_t hmagic;  // div_rows magic of H: I = floor(row / H)
    double tol;
    uint32_t levels;  // L
    uint32_t slot;    // kLtSolo, or the unit's index among the split units (its row of the global bins)
};
static_assert(sizeof(LtUnit) == 32, "descriptor of 8-B members first");
constexpr uint32_t kLtSolo = 0xffffffffu;

// The radix select of one split unit in the size-budget mode (wc_budget.hip),
// between its passes: it stays on the device.
struct BudgetState {
    uint32_t prefix;  // the key's digits found so far (12, then 24 bits)
    uint32_t above;   // candidates whose key is above every key with this prefix
    uint32_t done;    // 1: thresh / key are written, the later passes skip the unit
    uint32_t pad;
};
static_assert(sizeof(BudgetState) == 16, "one 16-B load");

// One unit of the pair selection (wc_thin.hip: thinning and split).  Built per call: the
// levels, the budget or thresholds and the output slots are not part of a plan.
struct ThinDesc {
    uint64_t dmagic;     // div_rows magic of D: row = floor(position / D)
    uint64_t hmagic;     // div_rows magic of H: I = floor(row / H)
    uint64_t out_off;    // the unit's output slot: prefix of 24 + 8 * cap, == 4 (mod 8)
    uint64_t rest_off;   // a split: the rest's slot, prefix of 24 + 8 * N, == 4 (mod 8); else 0
    int32_t W, H, D;     // the box
    int32_t want;        // the header's ncoeff field: W*H*D, or -L for L >= 2
    uint32_t N;          // W*H*D
    uint32_t L;
    uint32_t dt_begin;   // the unit's first pair tile: look-back granules and scratch rows
    uint32_t slot;       // kLtSolo, or the unit's index among the split units (its global bins)
    uint32_t K;          // budget form: max_pairs
    uint32_t cap;        // pairs the slot holds: min(K, N), or N
    union {
        float th[4];     // threshold form: t_1..t_L
        double tol;      // tolerance form (offset 72: 8-B aligned)
    };
};
static_assert(sizeof(ThinDesc) == 88, "descriptor of 8-B members first");
// The tolerance form's global bins of a split unit: WC_MAX_LEVELS level-major bin sets, then the NaN
// pairs of each level.
constexpr uint32_t kThinTolBinStride = 4 * 4096 + 4;  // (WC_MAX_LEVELS, WC_HIST_BINS: asserted in wc_thin.hip)

// What launch_thin (wc_thin.hip) takes: the passes of wc_thin_budget / wc_thin_thresh / wc_thin_tol and of
// wc_split_budget / wc_split_thresh / wc_split_tol over the plan's decode tiles of the units (budget: the
// radix select between the key pass and the compaction; tol: the bin pass and the rule's walk there).  The kept pairs are the output (a split's base);
// a split also gives the rest's side, which a thin call leaves null.
struct ThinLaunch {
    const ThinDesc* desc;
    int n;
    const FTile* tiles;
    uint32_t ntiles;
    const uint8_t* payload;
    const uint64_t* offsets;
    bool budget;
    int ordered;
    uint32_t* ticket[2];            // key pass, compaction: per unit, zeroed
    unsigned long long* status[2];  // their look-back granules, per decode tile, zeroed
    uint2* s1;                      // {key, pos} per pair
    uint32_t* s2;                   // positions of the kept pairs
    uint32_t* keyw;                 // per unit: T (budget)
    uint32_t* keptw;                // per unit: kept pairs (zeroed)
    float* thresh;                  // n x WC_MAX_LEVELS (budget)
    uint32_t* key_out;              // the caller's d_key or null
    const uint2* items;             // split units' tile runs of `chunk` tiles
    uint32_t nitems, chunk;
    const uint32_t* split_units;
    uint32_t nsplit;
    uint32_t* gbins;                // nsplit x 4352 words
    BudgetState* state;             // nsplit
    uint8_t* out;
    uint64_t* out_offsets;
    uint32_t* kept;
    uint32_t* err;
    uint8_t* rest;                  // a split: the rest's buffer, else null (and so the four below)
    uint64_t* rest_offsets;
    uint32_t* rest_pairs;
    uint32_t* s3;                   // positions of the rest's pairs
    uint32_t* restw;                // per unit: rest pairs (zeroed)
    // the tolerance form (wc_thin_tol / wc_split_tol): budget is false, T comes from the rule's walk over
    // the unit's bins; gbins: nsplit x kThinTolBinStride words
    bool tol;
    int maxl;                       // the largest L of the call
    double* bound;                  // the caller's d_bound or null
};

// What launch_merge (wc_layers.hip) takes, and its kernels by value: side 0 is a, side 1 is b.  The units'
// descriptors are ThinDesc's (box, header field, N, dt_begin, out_off; cap = N).
struct MergeLaunch {
    const ThinDesc* desc;
    int n;
    const FTile* tiles;
    uint32_t ntiles;
    const uint8_t* pay[2];
    const uint64_t* off[2];
    int ordered;
    uint32_t* ticket[2];            // per side and unit, zeroed
    unsigned long long* status[2];  // per side: look-back granules per decode tile, zeroed
    uint32_t* pos[2];               // per side: the positions of its pairs below N
    uint32_t* live;                 // [2][n]: their counts (zeroed)
    uint32_t* overlap;              // [n]: nonzero where a and b hold a pair at one position (zeroed)
    uint8_t* out;
    uint64_t* out_offsets;
    uint32_t* pairs;
    uint32_t* err;
};

// One unit of the packed-payload transcoders (wc_pack.hip): the box, the unit's
// slot in the packed buffer (wc_packed_bound's scheme) and its slot in the
// standard payload buffer (wc_payload_bound's).  Kept on the device while a
// batch recurs.
struct PackDesc {
    uint64_t pk_off;   // packed slot: prefix of pad8(S(cells) + 4), == 4 (mod 8)
    uint64_t pay_off;  // forward slot: prefix of 24 + 8 * cells, == 4 (mod 8)
    int32_t W, H, D;
    uint32_t ncells;
};
static_assert(sizeof(PackDesc) == 32, "descriptor of 8-B members first");
constexpr int kPackTile = 2048;                        // pairs per transcoder workgroup (wc_pack.hip has the arithmetic)
constexpr uint64_t kPackMaxCells = uint64_t(1) << 21;  // the device transcoders' largest unit (WC_PACK_MAX_CELLS)

// Per-unit skip words (bad[u]) that k_decode<true> and k_decode_region leave for
// the launches after them: the level passes and k_inverse{,_fast}<true> skip a
// unit unless its word is kUnitRun.
constexpr uint32_t kUnitRun = 0u;      // the level passes and the one-level inverse run
constexpr uint32_t kUnitRefused = 1u;  // the header disagrees: nothing more runs, the cells stay untouched
constexpr uint32_t kUnitBox = 2u;      // wc_inverse_coarse and wc_inverse_region, r == L: k_corner_box writes the cells, the rest skip

// Sentinel for a unit whose flat[0] is NaN: std::max_element then returns
// flat[0] itself (every comparison with NaN is false), so thresh is NaN.
constexpr unsigned long long kKeyNaNFirst = ~0ull;

// Error bits raised by kernels (ctx->d_err).
constexpr uint32_t kErrHeader = 1u;      // payload header disagrees with the unit
constexpr uint32_t kErrNegativeRun = 2u; // a run length < 0 (reference: UB)
constexpr uint32_t kErrOverlap = 4u;     // wc_merge: both inputs hold a pair at one position

constexpr uint32_t kEpochMask = 0x3fffffffu;  // epoch bits of a look-back granule (wc_device.h GranuleEpoch32)

#ifndef WC_EMIT_EW
#define WC_EMIT_EW 4  // waves per emit block of the small-unit launch (2048 coefficients per wave)
#endif
constexpr int kEmitTile = WC_EMIT_EW * 2048;  // coefficients per emit tile (32 per thread)
constexpr int kEmitTileBig = 16384;      // emit tile of units of >= kEmitBigCells (8 waves)
constexpr uint64_t kEmitBigCells = uint64_t(1) << 21;  // 128^3: longer tiles pay

// Parameter block of k_emit (wc_emit.hip), filled by wc_capi.cpp.
// An emit block: its tile and every unit field the emit reads, so that a
// block's first memory round trip (one uniform load) already yields the
// addresses of its flags, key and coefficients.
struct EmitDesc {
    uint64_t coef_off;  // the unit's staged coefficients (UnitDev::coef_off)
    uint64_t pay_off;   // the unit's payload slot
    uint32_t ncells;    // W*H*D (< 2^31)
    uint32_t unit;
    uint32_t index;     // tile index within the unit (the ordered form's)
    uint32_t et_begin;  // the unit's first look-back granule
    uint32_t net;       // emit tiles of the unit
    int32_t nx, ny, nz;
    uint32_t mode;      // bit 0: UnitDev::sparse; bits 1-3: lbz, log2 of the staged segment length;
                        // bits 8-15: the row divisor's shift (div_rows)
    uint32_t flag_off;  // UnitDev::flag_off (the plan keeps every flag range below 4 GiB)
    uint32_t row_off;   // the unit's first row-index entry (UnitDev::row_off; the plan keeps it < 2^32)
    uint32_t dmul;      // the row divisor's multiplier (div_rows; UnitDev::dmagic); row_shift 0: no row index
};
static_assert(sizeof(EmitDesc) == 64, "one 64-B descriptor per emit block (one scalar load)");

struct EmitParams {
    const UnitDev* units;
    const EmitDesc* edesc;         // emit blocks in launch order (interleaved, wc_capi.cpp build_etiles)
    int n;
    uint32_t ordered;              // 1: tile index from edesc (dispatch order), 0: from tickets[unit]
    uint32_t* tickets;             // per-unit tile tickets (ticket form), zeroed per call
    const unsigned long long* key; // unit max keys (wc_xform.h coef_key)
    unsigned long long* status;    // decoupled look-back granules, per emit tile, zeroed per call
    uint8_t* payload;
    uint64_t* offsets;             // [n + 1]
    uint32_t* kept;                // [n]
    uint32_t* err;                 // the context's error word (atomicOr; read and cleared at wc_synchronize)
    double keep;
    uint32_t use_gthresh;          // 1: every unit uses gthresh (global histogram mode), 0: reference rule
    float gthresh;                 // fp32 threshold: keep |c| > gthresh
    const uint8_t* flags;          // sparse-staging segment flags (null: every unit dense)
    uint2* rowinfo;                // wc_forward_rows: the payloads' row index out (null: not written);
                                   // unit u's entries at units[u].row_off, units with dmagic != 0
    const float* uthresh;          // RMSE-tolerance mode: unit u keeps |c| > uthresh[u] (null: the rules above)
};

constexpr int kSegShift = 4;    // sparse staging: flag index space of 16 coefficients per byte (min segment)
// Byte position of sparse-staging segment s (= flat index >> sh, sh = log2 of
// the segment length, 4 or 5) in its unit's flag range: within
// each 2048-coefficient block of a unit (one emit wave's share of a tile) the
// 8 flags one emit thread reads (element groups it = 0..7: segment it * G + g,
// G = 256 >> sh, g = its lane group) sit in 8 consecutive bytes, g * 8 + it:
// one 8-B load instead of eight byte loads (wc_emit.hip).  Each sparse unit's
// flag range (UnitDev::flag_off) is 8-B aligned and spans whole blocks, so
// permuted positions never leave it.
__host__ __device__ inline uint64_t flag_pos(uint64_t s, int sh) {
    const int lb = 11 - sh, lg = 8 - sh;
    const uint64_t sw = s & ((1ull << lb) - 1);
    return (s & ~((1ull << lb) - 1)) | ((sw & ((1ull << lg) - 1)) << 3) | (sw >> lg);
}
// flag_pos on 32-bit segment indices (K1's S32 form: units of < 2^30 cells).
__host__ __device__ inline uint32_t flag_pos32(uint32_t s, int sh) {
    const int lb = 11 - sh, lg = 8 - sh;
    const uint32_t sw = s & ((1u << lb) - 1);
    return (s & ~((1u << lb) - 1)) | ((sw & ((1u << lg) - 1)) << 3) | (sw >> lg);
}
#ifndef WC_RIX_TILE
#define WC_RIX_TILE 4096
#endif
constexpr int kRixTile = WC_RIX_TILE;   // pairs per row-index (K5) tile
constexpr int kRixRounds5 = kRixTile / kThreads;
constexpr int kRixLds = 9216;   // K6r tile: default LDS budget in floats (36 KB: 4 workgroups per CU)

}  // namespace wc
