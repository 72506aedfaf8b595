// wc_ctx.h — the library context and batch plan, shared by the translation
// units behind the C-ABI (include/wavelet_amd.h).  Internal: not installed.
//
//   wc_common.cpp    errors, device buffers, unit validation, the process-wide
//                    context registry (launch-order vs ticket look-backs), the
//                    kernel error word
//   wc_plan.cpp      batch plans (tile lists, emit descriptors, row-index
//                    layout) mirrored in HBM, scratch sizing
//   wc_capi.cpp      context lifetime, options and the device-pointer entry
//                    points (kernel launches)
//   wc_hostpipe.cpp  the _host entry points: pipelined unit runs over PCIe,
//                    pinned bounce slots, helper threads (no kernels of its
//                    own: it calls the device entry points), also built
//                    against a CPU fake of the HIP runtime for the sanitizer
//                    tests (tests/cpp/test_hostpipe.cpp)
//   wc_hostserial.cpp the two serial drivers of the opt-in modes' _host entry points
//                    (unit runs one after another on the context's stream):
//                    forward_serial (cells in) and payload_serial (payload bytes
//                    in), the run splitter, the span helpers, the one error exit;
//                    built against the CPU fake too (tests/cpp/test_hostserial.cpp)
//   wc_tolhost.cpp   host side of the RMSE-tolerance mode: the selection rule
//                    on one unit's counts, the mode's argument checks and
//                    wc_forward_tol_host (a call of forward_serial)
//   wc_levelsrule.cpp / wc_levelshost.cpp  the multi-level mode: wc_levels_for,
//                    wc_payload_levels and the argument checks (no device entry
//                    point called), and the _levels_host entry points
//   wc_leveltolrule.cpp / wc_leveltolhost.cpp  the RMSE tolerance on the
//                    multi-level transform: the per-level selection rule (plain
//                    C++, linked alone by tests/cpp/test_leveltol.cpp) and
//                    wc_forward_levels_tol_host
//   wc_budgetrule.cpp / wc_budgethost.cpp  the size-budget mode: the exact top-K
//                    selection rule on one unit's final array (plain C++, linked
//                    alone by tests/cpp/test_budget.cpp), the argument checks
//                    and wc_forward_levels_budget_host
//   wc_maxerrrule.cpp / wc_maxerrhost.cpp  the pointwise (max-abs) error bound: the
//                    search on one unit by full masked inverses (plain C++, linked
//                    alone by tests/cpp/test_maxerr.cpp), the argument checks,
//                    wc_forward_levels_maxerr_host and wc_maxerr_host
//   wc_packrule.cpp / wc_packhost.cpp  packed payloads: the format's host rule
//                    (plain C++, linked alone with wc_packfmt.h by
//                    tests/cpp/test_pack.cpp), and wc_pack, wc_unpack and their
//                    _host forms
//   wc_thinrule.cpp / wc_thinhost.cpp  thinning in the compressed domain: the rule on
//                    one payload (wc_thin_unit, plain C++), wc_thin_bound and the
//                    _host forms of wc_thin_budget / wc_thin_thresh (payload_serial)
//   wc_layersrule.cpp / wc_layershost.cpp  progressive layers: the rule on one unit
//                    (wc_split_unit, wc_merge_unit, plain C++, on wc_thin_unit), the bounds and
//                    the _host forms of wc_split_budget / wc_split_thresh / wc_merge
//                    (payload_serial with its second stream)
//   wc_thintolrule.cpp / wc_thintolhost.cpp  the tolerance forms of both: the rule on one
//                    payload (wc_thin_tol_unit, wc_split_tol_unit, plain C++, on
//                    wc_tol_levels_threshold, wc_thin_unit and wc_split_unit) and
//                    wc_thin_tol_host / wc_split_tol_host (payload_serial)
//   wc_coarsehost.cpp host side of the reduced-resolution inverse: wc_coarse_units,
//                    the argument checks and wc_inverse_coarse_host (a call of
//                    wc_regionhost.cpp's inverse_compact_host)
//   wc_regionrule.cpp / wc_regionhost.cpp  the sub-box inverse: wc_region_align
//                    and wc_region_units (plain C++, linked alone with
//                    wc_regionmap.h by tests/cpp/test_regionrule.cpp), the
//                    argument checks, wc_inverse_region_host and what it shares
//                    with wc_inverse_coarse_host (inverse_compact_host)
//   wc_packdecodehost.cpp  the _host forms of the decoders over packed units
#pragma once

#include "wavelet_amd.h"
#include "wc_hostmem.h"
#include "wc_internal.h"

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace wc {

size_t transform_lds_bytes(int lbx, int lby, int lbz);
size_t transform_fast_lds_bytes(int lbx, int lby, int lbz);
hipError_t launch_transform(hipStream_t, const void*, int, const UnitDev*, const XTile*, uint32_t, size_t,
                            float*, int, unsigned long long*);
hipError_t launch_transform_fast(hipStream_t, const void*, int, const UnitDev*, const XTile*, uint32_t, size_t,
                                 float*, int, unsigned long long*, uint8_t*, uint32_t*, double, uint32_t);
uint32_t transform_pf_grid(size_t lds);
size_t transform_hist_lds_bytes(size_t lds_fast);
uint32_t transform_hist_grid(size_t lds);
hipError_t launch_transform_hist(hipStream_t, const void*, int, const UnitDev*, const XTile*, uint32_t, size_t,
                                 float*, unsigned long long*, unsigned long long*, uint32_t);
uint32_t inverse_rows_grid(size_t lds);
hipError_t launch_transform_fallback(hipStream_t, const void*, int, const UnitDev*, int, const XTile*, size_t, float*,
                                     const unsigned long long*, const uint32_t*, double);
hipError_t launch_pack(hipStream_t, const UnitDev*, int, const uint32_t*, const uint8_t*, uint64_t*, uint8_t*);
hipError_t launch_decode(hipStream_t, const UnitDev*, const FTile*, uint32_t, const FTile*, uint32_t,
                         unsigned long long*, uint32_t, const uint8_t*, const uint64_t*, uint32_t*,
                         unsigned long long*, float*, uint2*, uint32_t*, int, uint32_t*,
                         const int32_t* levels = nullptr);
// the dense decode of every unit from packed units, read below cap (wc_inverse_packed)
hipError_t launch_decode_packed(hipStream_t, const UnitDev*, const FTile*, uint32_t nft, const uint8_t* packed,
                                const uint64_t* offsets, uint64_t cap, uint32_t* ticket, unsigned long long* status,
                                float* flat, uint32_t* err, int ordered, const int32_t* levels, uint32_t* bad);
hipError_t launch_pair_counts(hipStream_t, const UnitDev*, int, const uint8_t*, const uint64_t*, uint32_t*, uint32_t*);
hipError_t launch_inverse_rows(hipStream_t, const RTile*, uint32_t, size_t, uint32_t, const uint8_t*,
                               const uint64_t*, const uint2*, float*, int, const void*, int, const UnitDev*, int,
                               double*, double*, bool, const uint32_t*);
hipError_t launch_inverse(hipStream_t, const float*, int, const UnitDev*, const XTile*, uint32_t, size_t, uint32_t,
                          size_t, float*, const uint32_t* bad = nullptr);
hipError_t launch_rmse(hipStream_t, const void*, int, const float*, const UnitDev*, int, const FTile*,
                       uint32_t, double*, double*);
hipError_t launch_emit(hipStream_t, const EmitParams&, const float*, uint32_t, uint32_t);
hipError_t launch_hist(hipStream_t, const UnitDev*, const FTile*, uint32_t, const float*, uint32_t,
                       unsigned long long*, bool);
hipError_t launch_tol(hipStream_t, const UnitDev*, int, const uint32_t*, const uint2*, uint32_t, uint32_t,
                      const uint32_t*, uint32_t, const float*, uint32_t*, const double*, float*, double*);
// wc_levels.hip: one level pass (analysis or synthesis into the side scratch, then
// the copy back), the key pass over the final array, the header patch, and the
// copy between the coefficient scratch and a caller's flat buffer
hipError_t launch_level(hipStream_t, bool fwd, const UnitDev*, const uint2* items, uint32_t nitems, int shift,
                        float* coef, float* side, unsigned long long* key, const uint32_t* bad);
hipError_t launch_level_key(hipStream_t, const UnitDev*, const uint2* items, uint32_t nitems, uint32_t chunk,
                            const float* coef, unsigned long long* key);
hipError_t launch_level_headers(hipStream_t, const UnitDev*, const uint2* items, uint32_t nitems, uint8_t* payload);
hipError_t launch_level_flat(hipStream_t, const UnitDev*, const FTile*, uint32_t ntiles, float* coef, float* flat,
                             int to_flat);
uint32_t level_chunk_blocks();
// wc_leveltol.hip: per-level bins + pick of the multi-level RMSE-tolerance mode,
// and the mask pass that applies the per-level thresholds to the staged array
hipError_t launch_leveltol(hipStream_t, const UnitDev*, int, const LtUnit*, const uint2* items, uint32_t nitems,
                           uint32_t chunk, const uint32_t* split_units, uint32_t nsplit, int maxl, const float* coef,
                           uint32_t* gbins, float* thresh, double* bound);
hipError_t launch_leveltol_mask(hipStream_t, const UnitDev*, const LtUnit*, const FTile*, uint32_t ntiles, float* coef,
                                const float* thresh);
// wc_budget.hip: the radix select of the size-budget mode (thresh / key per unit;
// launch_leveltol_mask then applies the thresholds)
hipError_t launch_budget(hipStream_t, const UnitDev*, int, const LtUnit*, const uint32_t* max_pairs, const uint2* items,
                         uint32_t nitems, uint32_t chunk, const uint32_t* split_units, uint32_t nsplit, int maxl,
                         const float* coef, uint32_t* gbins, BudgetState* state, float* thresh, uint32_t* key);
// wc_maxerr.hip: the three probe passes and the pick of the max-error mode (thresh per unit into the mask pass's
// slots; launch_leveltol_mask then applies them), the probe tiles of a unit, and the max-abs metric
hipError_t launch_maxerr_select(hipStream_t, const UnitDev*, int, const LtUnit*, const uint32_t* prefix, uint32_t ntiles,
                                int maxl, const void* cells, int dtype, const float* coef, unsigned long long* state,
                                float* slots, float* thresh, double* err);
uint32_t maxerr_tiles(int maxl, int32_t nx, int32_t ny, int32_t nz);
hipError_t launch_maxerr(hipStream_t, const void* orig, int dtype, const float* regen, const UnitDev*, const FTile*,
                         uint32_t, double* err);
// wc_region.hip: the decode of the reduced-resolution and the sub-box inverse
// (over a prefix of the full plan's decode tiles) into the compact units (whole:
// every region is its whole primed box, wc_inverse_coarse), and the copy of the
// compact units with r == L to their Box3D cells (over the derived plan's flat tiles)
hipError_t launch_decode_region(hipStream_t, const RegionDesc*, const FTile* dtiles, uint32_t ndt,
                                const uint8_t* payload, const uint64_t* offsets, uint32_t* ticket,
                                unsigned long long* status, float* compact, uint32_t* err, int ordered, uint32_t* bad,
                                bool whole, const uint64_t* packed_cap = nullptr);
hipError_t launch_corner_box(hipStream_t, const RegionDesc*, const FTile* ftiles, uint32_t nft, const float* compact,
                             float* out, const uint32_t* bad);

// wc_pack.hip: the packed payload format's transcoders (k_pack_widths + k_pack_body, k_unpack)
hipError_t launch_pack_units(hipStream_t, const PackDesc*, const FTile* tiles, uint32_t ntiles, const uint8_t* payload,
                             const uint64_t* offsets, int vbytes, int n, uint8_t* packed, uint64_t* packed_offsets,
                             uint64_t* packed_bytes, uint32_t* err);
hipError_t launch_unpack_units(hipStream_t, const PackDesc*, const FTile* tiles, uint32_t ntiles, const uint8_t* packed,
                               const uint64_t* packed_offsets, uint64_t cap, int n, uint8_t* payload, uint64_t* offsets,
                               uint32_t* kept, uint32_t* err);

// wc_thin.hip: the passes of wc_thin_budget / wc_thin_thresh and, with the rest's side set, of
// wc_split_budget / wc_split_thresh (wc_internal.h ThinLaunch)
hipError_t launch_thin(hipStream_t, const ThinLaunch&);
// wc_layers.hip: the passes of wc_merge
hipError_t launch_merge(hipStream_t, const MergeLaunch&);

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// A batch plan: unit descriptors and tile lists, mirrored in HBM.
//   xtiles = [generic | fast]   transform tiles, unit-major in each part
//   ixtiles                     the same, fast tiles in reverse unit order (inverse)
//   ftiles                      kFlatTile flat tiles (RMSE, histogram)
//   dtiles                      decode blocks, interleaved by tile index across units
//   edesc                       emit blocks (tile + unit fields), interleaved order
struct Plan {
    std::vector<wc_unit> key;
    std::vector<UnitDev> units;
    std::vector<XTile> xtiles;
    std::vector<XTile> ixtiles;  // dense inverse tiles of the non-row-indexed units: [generic | fast]
    std::vector<RTile> rtiles;   // K6r tiles of the row-indexed units
    std::vector<FTile> ftiles, dtiles, rdtiles;  // dtiles: dense decode, rdtiles: row index (K5)
    int rix_lds = kRixLds;              // WC_OPT_RIX_LDS the plan was built with
    int rix_lx = 4;                     // WC_OPT_RIX_TX the plan was built with
    bool rix_xcd = false;               // WC_OPT_RIX_XCD the plan was built with
    int inv_groups = 1;                 // WC_OPT_INV_GROUPS the plan was built with
    // row-indexed inverse in unit groups (pipelined: K5 of group g + 1 runs
    // beside K6r of group g): group g's row-index tiles are rdtiles
    // [ig_rd[g], ig_rd[g+1]) and its K6r tiles rtiles [ig_rt[g], ig_rt[g+1])
    std::vector<uint32_t> ig_rd, ig_rt;
    std::vector<EmitDesc> edesc;  // [units of kEmitTile tiles | units of kEmitTileBig tiles]
    uint32_t nedesc_small = 0;
    uint32_t ngen = 0, nfast = 0, netiles = 0;
    uint32_t ign = 0, ifast = 0;  // ixtiles split
    bool inv_rows = true;         // WC_OPT_INVERSE_ROWS the plan was built with
    uint64_t rowinfo_entries = 0;
    size_t lds_rows = 0;
    bool any_sparse = false;
    uint64_t coef_extent = 0;  // floats of staged coefficient scratch
    uint64_t flag_bytes = 0;   // bytes of sparse-staging segment flags (UnitDev::flag_off ranges + slack)
    size_t lds_gen = 0, lds_fast = 0, lds_inverse = 0;
    size_t state_bytes = 0;    // forward per-call state: 16 | key[n] | tickets[n] | status[netiles]
    DevBuf d_units, d_xtiles, d_ftiles, d_dtiles, d_edesc, d_ixtiles, d_rtiles, d_rdtiles;
};

inline int ceil_log2(int64_t v) {
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}

inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

}  // namespace wc

using wc::kRixLds;

struct wc_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    wc::Plan plan;
    bool plan_valid = false;
    bool opt_ordered = true;  // WC_OPT_ORDERED (see include/wavelet_amd.h)
    bool force_tickets = false;  // WC_OPT_TICKETS: the ticket form of the look-backs
    bool opt_reverse = false;    // WC_OPT_REVERSE_TILES (test hook): each unit's look-back tiles in reverse launch order
    uint32_t opt_spin_limit = 0; // WC_OPT_SPIN_LIMIT (0: kSpinSelf), mirrored in errflag[1]
    bool opt_sparse = true;   // WC_OPT_SPARSE
    bool opt_inv_rows = true; // WC_OPT_INVERSE_ROWS
    int opt_rix_lds = kRixLds; // WC_OPT_RIX_LDS
    int opt_rix_lx = 4;        // WC_OPT_RIX_TX
    bool opt_rix_blocked = false; // WC_OPT_RIX_BLOCKED
    bool opt_rix_xcd = false;     // WC_OPT_RIX_XCD
    int opt_inv_groups = 1;       // WC_OPT_INV_GROUPS
    hipStream_t aux = nullptr;    // second stream of the pipelined inverse
    std::vector<hipEvent_t> iev;  // its events
    // A kernel that may raise error bits ran since the last check.  Kernels
    // atomicOr into ONE persistent error word (errflag, zeroed at creation and
    // after each read), so errors of several async calls accumulate until the
    // next wc_synchronize / _host call reads them.
    bool err_check_pending = false;
    // wc_forward_stage left this plan's coefficients + unit keys in coef/state
    // (cleared by set_device, i.e. by every other compute entry point)
    bool staged = false;
    bool sparse_staged = false;  // the last stage_transform used sparse staging
    uint64_t plan_gen = 0;  // bumped whenever get_plan rebuilds the plan
    // scratch (grow-only)
    wc::DevBuf coef, part, errflag, state, flags, rowinfo, npairs;
    // row index (wc_inverse): epoch-tagged look-back granules, zeroed when
    // allocated and never again (a granule of an earlier call reads as
    // unpublished); epoch: the call counter they are tagged with
    wc::DevBuf istate;
    uint32_t epoch = 0;
    // host-path staging
    wc::DevBuf h_cells, h_payload, h_packed, h_offsets, h_poff, h_kept, h_out;
    wc::DevBuf h_rows, h_rmse;  // wc_round_trip_host: a run's row index, the per-unit RMSE
    // wc_forward_host pipeline: copy streams, per-run events, pinned metadata
    int64_t opt_host_chunk = int64_t(1) << 25;  // WC_OPT_HOST_CHUNK
    hipStream_t up = nullptr, down = nullptr;
    std::vector<hipEvent_t> hev;
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // host pages of a copy's destination faulted in ahead of it (wc_hostmem.h)
    int opt_host_threads = -1;    // WC_OPT_HOST_THREADS (-1: not yet resolved from the environment)
    bool opt_host_thp = false;    // WC_OPT_HOST_THP (opt-in: the advice changes the caller's mappings)
    // RMSE-tolerance mode (wc_forward_tol): the call's tolerances and split
    // layout go through pinned memory of the context (the caller's array need
    // not outlive the call); tol_ev orders the next call's rewrite after the copy
    int opt_tol_solo = 64;        // WC_OPT_TOL_SOLO_TILES
    void* tol_pin = nullptr;
    size_t tol_pin_bytes = 0;
    hipEvent_t tol_ev = nullptr;
    bool tol_ev_live = false;
    wc::DevBuf tol_in;            // tol[n] | slot[n] | split_units[nsplit] | items[nitems] | thresh[n]
    wc::DevBuf tol_bins;          // kHistBins uint32 per split unit and level (none without split units)
    wc::DevBuf h_thresh, h_bound; // wc_forward_tol_host: per-unit thresholds and bounds (_budget_host: the keys)
    // multi-level mode (wc_forward_levels / wc_inverse_levels): the side scratch
    // of the level passes (coef_extent / 8 floats); the call's levels and work
    // lists go through the same pinned block and tol_in
    wc::DevBuf lv_side;
    // wc_inverse_coarse / wc_inverse_region: the call's descriptors on the host
    // (kept between calls: a batch's 104 B per unit are not allocated anew each time)
    std::vector<wc::RegionDesc> cdesc;
    // packed payloads (wc_pack / wc_unpack): the batch's descriptors and tiles
    // (PackDesc[n] | FTile[ntiles]) stay on the device while the units and the
    // value bytes recur (pk_key, pk_vbytes); the _host forms' staging
    wc::DevBuf pk_desc;
    std::vector<wc_unit> pk_key;
    int pk_vbytes = 0;
    uint32_t pk_ntiles = 0;
    wc::DevBuf pk_in, pk_out, pk_off, pk_bytes;
    // wc_thin_budget / wc_thin_thresh / wc_split_*: per-call state, select bins and the pair scratches (wc_thin.hip)
    wc::DevBuf thin;
    // wc_merge: per-call state and the two position rows (wc_layers.hip).  payload_serial's second stream:
    // a split's rest slots with their offsets and counts, or a merge's second input with its offsets
    wc::DevBuf merge, h_second, h_second_off, h_second_cnt;
    std::unique_ptr<wc::HostPool> hpool;
    // uploads from pageable host memory: copied by upool's threads into pinned
    // bounce slots, each slot's copy to the device ordered by an event
    std::unique_ptr<wc::HostPool> upool;
    void* bounce = nullptr;
    std::vector<hipEvent_t> bev;   // per slot: recorded after the slot's last queued copy
    std::vector<bool> bev_live;    // per slot: bev recorded (wait on it before the slot is rewritten)
    uint32_t bnext = 0;            // next slot (rotates across calls)
    // plans of earlier batches (most recent last), swapped in when a batch recurs
    std::vector<wc::Plan> plan_cache;
    // persistent-grid sizes (resident workgroups for an LDS size) on this device
    std::map<std::pair<int, size_t>, uint32_t> grids;
    // per-kernel event timing (wc_profile_enable / wc_profile_read)
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    struct Mark {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Mark> marks;
};

namespace wc {

// wc_common.cpp
int fail(wc_ctx* c, int code, const std::string& msg);
int hip_fail(wc_ctx* c, hipError_t e, const char* what);
int ensure(wc_ctx* c, DevBuf& b, size_t bytes);      // grow-only device buffer
int validate_units(wc_ctx* c, const wc_unit* units, int n);
int check_aligned(wc_ctx* c, const void* p, const char* what, uintptr_t align = 16);
hipEvent_t take_event(wc_ctx* c);
int upload(wc_ctx* c, DevBuf& d, const void* h, size_t bytes, const char* what);
int set_device(wc_ctx* c);
bool use_ordered(const wc_ctx* c);
// the look-back kernels' tile-order argument: 0 tickets, 1 plan order, 2 reversed (WC_OPT_REVERSE_TILES)
inline int tile_order(const wc_ctx* c) { return use_ordered(c) ? (c->opt_reverse ? 2 : 1) : 0; }
// levels, or n ones in `storage` where the caller gave none (every unit L = 1)
inline const int32_t* levels_or_ones(const int32_t* levels, int n, std::vector<int32_t>& storage) {
    if (levels) return levels;
    storage.assign(n, 1);
    return storage.data();
}
int check_kernel_errors(wc_ctx* c);
uint64_t cells_extent(const wc_unit* units, int n);

// wc_plan.cpp
int get_plan(wc_ctx* c, const wc_unit* units, int n);
void free_plan(Plan& P);
size_t decode_state_bytes(const Plan& P);
int ensure_scratch(wc_ctx* c);
uint32_t persistent_grid(wc_ctx* c, int which, size_t lds);
int inverse_stream(wc_ctx* c, int nev);

// wc_hostpipe.cpp
int host_threads_default();

// wc_tolhost.cpp
int validate_tol(wc_ctx* c, const wc_unit* units, int n, const double* tol);

// wc_levelsrule.cpp
int validate_levels(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels);

// wc_hostserial.cpp: the serial host drivers (the callers have checked their arguments and called set_device)
// end[u] of a standard payload from its header; with from_headers, each unit's L as well
int payload_ends(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, int n, std::vector<uint64_t>& end,
                 std::vector<int32_t>* from_headers);
// a per-unit result, back at the call's end: stride bytes per unit from dev to host (NULL: not asked for)
struct UnitResult {
    const void* dev;
    void* host;
    size_t stride;
};
// the device call of run [a, a + m) into wc_forward's slots, and the round trip of its payloads (rmse only)
using ForwardStep = std::function<int(int a, int m, const void* d_cells, uint8_t* d_payload, uint64_t run_bound,
                                      uint64_t* d_offsets, uint32_t* d_kept)>;
using RoundTrip = std::function<int(int a, int m, const uint8_t* d_payload, const uint64_t* d_offsets)>;
// wc_levelshost.cpp: the round trip of the level modes, wc_inverse_levels + wc_rmse
RoundTrip levels_round_trip(wc_ctx* c, int dtype, const wc_unit* units, const int32_t* levels);
// rmse: c->h_out (the round trip's cells) and c->h_rmse (double per unit, global index) are the driver's
int forward_serial(wc_ctx* c, const void* cells, int dtype, const wc_unit* units, int n, uint8_t* payload, uint64_t cap,
                   uint64_t* offsets, uint32_t* kept, double* rmse, const ForwardStep& step, const RoundTrip& trip,
                   std::vector<UnitResult> results);
// the device call of run [a, a + m) on the uploaded bytes (readable below bytes_cap) into c->h_out
using PayloadStep =
    std::function<int(int a, int m, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t bytes_cap)>;
struct SerialOut {
    uint64_t shift = 0, slack = 16;  // a run's bytes upload at shift + (their start & 7); c->h_payload has slack bytes more
    // either the boxes of out_units back from c->h_out (of out_bytes); checked: synchronize and
    // check_kernel_errors after each run's device call, before that run's cells cross back
    const wc_unit* out_units = nullptr;
    float* out = nullptr;
    uint64_t out_bytes = 0;
    bool checked = false;
    // or (payload set) c->h_out holds the run's slots in wc_forward's layout: forward_serial's packed tail
    uint8_t* payload = nullptr;
    uint64_t cap = 0;
    uint64_t* out_offsets = nullptr;
    uint32_t* kept = nullptr;
    std::vector<UnitResult> results;
    // the layers' second stream (wc_layershost.cpp); both unset for every other caller.
    // A second packed output (a split's rest; payload set too): the step left the run's slots, wc_forward's
    // layout, in c->h_second (of the run's wc_payload_bound) and their counts in c->h_second_cnt.
    uint8_t* payload2 = nullptr;
    uint64_t cap2 = 0;
    uint64_t* out_offsets2 = nullptr;
    uint32_t* kept2 = nullptr;
    // A second input (a merge's b): unit u's bytes [offsets2[u], end2[u]) of bytes2 go up with the run, to
    // c->h_second at the same shift rule, their rebased offsets to c->h_second_off.
    const uint8_t* bytes2 = nullptr;
    const uint64_t* offsets2 = nullptr;
    const uint64_t* end2 = nullptr;
};
// unit u's bytes are [offsets[u], end[u]); runs are split by the cells of units
int payload_serial(wc_ctx* c, const uint8_t* bytes, const uint64_t* offsets, const uint64_t* end, const wc_unit* units,
                   int n, const PayloadStep& step, const SerialOut& o);

// wc_maxerrhost.cpp: a bound per unit, each >= 0 (not NaN), and the units wc_forward_levels_tol accepts
int validate_maxerr(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const double* maxerr);

// wc_budgethost.cpp
int validate_budget(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels);

// wc_coarsehost.cpp
int validate_coarse(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                    const wc_unit* out_units);
uint64_t rows_magic(int32_t d);

// wc_regionhost.cpp (reduce NULL = all 0)
int validate_region(wc_ctx* c, const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                    const wc_region* regions, const wc_unit* out_units);
// wc_inverse_coarse_host (regions NULL) and wc_inverse_region_host after their null checks
int inverse_compact_host(wc_ctx* c, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                         const wc_unit* out_units, float* out);

// wc_packhost.cpp: no unit above WC_PACK_MAX_CELLS (the device calls over packed units)
int validate_pack(wc_ctx* c, const wc_unit* units, int n);

// wc_capi.cpp: wc_thin_budget (max_pairs) and wc_thin_thresh (thresh) after their null checks.
// full_slots: the budget form with wc_forward's slot layout (cap_u = N_u), for launch_pack.
int thin_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_out,
                uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key);

// wc_capi.cpp: wc_split_budget / wc_split_thresh and wc_merge after their null checks (thin_device's
// conventions; full_slots: the base in wc_forward's slot layout).
struct SplitOut {  // the rest's side of a split
    uint8_t* d_rest;
    uint64_t capacity;
    uint64_t* d_offsets;
    uint32_t* d_pairs;
};
int split_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                 const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_base,
                 uint64_t base_capacity, uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest,
                 float* d_thresh, uint32_t* d_key);
int merge_device(wc_ctx* c, const uint8_t* d_a, const uint64_t* d_a_offsets, const uint8_t* d_b,
                 const uint64_t* d_b_offsets, const wc_unit* units, int n, const int32_t* levels, uint8_t* d_out,
                 uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_pairs);
// wc_capi.cpp: wc_thin_tol / wc_split_tol after their null checks (the slots are wc_forward's: cap_u = N_u)
int thin_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const double* tol, uint8_t* d_out, uint64_t out_capacity,
                    uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound);
int split_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                     const int32_t* levels, const double* tol, uint8_t* d_base, uint64_t base_capacity,
                     uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest, float* d_thresh,
                     double* d_bound);

// Bracket one launch with events when profiling is on.
struct StageTimer {
    wc_ctx* c;
    int stage;
    hipEvent_t a = nullptr;
    StageTimer(wc_ctx* c_, int s) : c(c_), stage(s) {
        if (c->prof) {
            a = take_event(c);
            (void)hipEventRecord(a, c->stream);
        }
    }
    ~StageTimer() {
        if (c->prof && a) {
            hipEvent_t b = take_event(c);
            (void)hipEventRecord(b, c->stream);
            c->marks.push_back({stage, a, b});
        }
    }
};

}  // namespace wc
