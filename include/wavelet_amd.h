/*
 * wavelet_amd.h — C-ABI of the MI355X (gfx950) wavelet codec.
 *
 * This is the drop-in boundary for the reference's per-box hot path
 * (carsonmw3/wavelet-compression @ 2025-07-04).  The reference calls its codec
 * through C++ functions; the C++ mirror in include/wavelet_amd/ keeps those
 * exact signatures and forwards to the entry points below.  Each entry point
 * names the reference routine(s) it replaces:
 *
 *   wc_forward         compress() minus the xz write      src/compressor.h:9-15,
 *                      = wavelet_decompose + threshold     src/compressor.cpp:192-248
 *                        + rle_encode + serialize          src/compressor.cpp:24-80
 *   wc_decompose       wavelet_decompose                   src/compressor.cpp:85-185
 *   wc_inverse         decompress() minus the xz read      src/decompressor.h:6-10
 *                      = rle_decode + inverse transform    src/decompressor.cpp:14-30,238-255
 *   wc_inverse_flat    inverse_wavelet_decompose           src/decompressor.h:18, .cpp:79-159
 *   wc_rmse            calc_rmse_per_box (one component)   src/calc-loss.h:6-8, .cpp:12-43
 *
 * Conventions
 *   - Plain C types only; every function returns WC_OK (0) or a WC_ERR_* code,
 *     and wc_last_error() describes the last failure on that context.
 *   - A "unit" is one Box3D component (one (time, level, box, component) tuple
 *     of the reference's AMRIterator loop, src/modes.cpp:100-103): W x H x D
 *     cells, x fastest (src/grid.h:15-19).  Batches of units run in one call.
 *   - Functions without a _host suffix take DEVICE pointers (HBM-resident data)
 *     and are asynchronous on the context's stream.  _host variants take host
 *     pointers, copy through pinned staging, and return when results are ready.
 *   - Device buffers of cells, payloads, coefficients and reconstructions must
 *     be 16-byte aligned (hipMalloc and torch allocations are); offsets,
 *     kept counts, row indexes and RMSE outputs need their element alignment;
 *     both inputs of wc_rmse (the original cells and the reconstruction) and
 *     the original cells of the fused calls, any element alignment (wc_rmse
 *     only reads them).  Otherwise WC_ERR_INVALID.
 *   - One context per device per host thread.  The context owns its stream and
 *     its scratch memory; the caller owns every buffer it passes.
 *
 * Payload layout: unit u's serialized bytes, IDENTICAL to the reference's
 * serialize_compressed_wavelet output (src/compressor.cpp:55-80)
 *     int32 W, H, D; int32 ncoeff = W*H*D; int32 nrle; nrle x {int32 run, float32 value}
 * (ncoeff = -L in the opt-in multi-level mode, wc_forward_levels)
 * start at payload + offsets[u] and are 20 + 8*kept[u] bytes long.  Every
 * offsets[u] is == 4 (mod 8), so each pair is 8-byte aligned.
 *   - wc_forward (device): offsets[u] is unit u's fixed SLOT, the prefix of the
 *     worst-case sizes 24 + 8*W*H*D of the units before it (starting at 4), so
 *     no unit waits for another's kept count; offsets[n] = end of the last
 *     unit's bytes.  The buffer between units is not written.
 *   - wc_forward_host: the slots are packed densely (each unit 24 + 8*kept[u]
 *     bytes apart) before the copy back; offsets[] describe the packed buffer.
 *   - wc_inverse / wc_inverse_host accept any offsets that are multiples of 4.
 */
#ifndef WAVELET_AMD_H
#define WAVELET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WC_OK 0
#define WC_ERR_INVALID 1  /* bad argument (null pointer, negative dims, capacity too small) */
#define WC_ERR_HIP 2      /* a HIP runtime call failed */
#define WC_ERR_NOMEM 3    /* device or pinned allocation failed */
#define WC_ERR_FORMAT 4   /* a payload header disagrees with its unit, or a run is negative */

#define WC_F32 0          /* cells are float32 (Box3D, src/box-structs.h:7) */
#define WC_F64 1          /* cells are float64 (plotfile FAB), narrowed in-kernel (src/preprocess.cpp:78) */

typedef struct wc_unit {
    uint64_t cell_offset; /* element offset of the unit's first cell in the cell buffer */
    int32_t nx;           /* Grid3D width  (x, fastest) */
    int32_t ny;           /* Grid3D height (y) */
    int32_t nz;           /* Grid3D depth  (z, slowest) */
    int32_t reserved;     /* must be 0 */
} wc_unit;

typedef struct wc_ctx wc_ctx;

/* Context lifetime.  `device` is a HIP device ordinal. */
int wc_device_count(void);  /* HIP devices visible to this process (0 without a GPU) */
int wc_ctx_create(int device, wc_ctx** out);
void wc_ctx_destroy(wc_ctx* ctx);
const char* wc_last_error(const wc_ctx* ctx);

/* Run on an external hipStream_t (e.g. a torch stream); NULL restores the
 * context's own stream.  Switching drains the previous stream first (kernels
 * queued there may still read the plan and scratch that later calls reuse), so
 * a caller must switch away from its stream BEFORE destroying it.  The switch
 * takes effect even when that drain fails (the error is still returned). */
int wc_set_stream(wc_ctx* ctx, void* hip_stream);
int wc_synchronize(wc_ctx* ctx);  /* also reports (and clears) kernel-side errors of earlier async calls */

/* Tuning switches (wc_set_option).
 * WC_OPT_SPARSE (default 1): the forward's transform stores only the
 *   16/32-coefficient flat segments that hold some |c| > (tile max) * (1 - keep)
 *   and flags them; the emit loads only flagged segments.  Same bytes out;
 *   0 = dense staging of every coefficient.
 * WC_OPT_RIX_XCD (default 0): the row-indexed inverse's tiles dealt to the XCDs
 *   in contiguous runs (neighbouring tiles share payload lines at their range
 *   ends).  Same cells.
 * WC_OPT_INV_GROUPS (default 1): the row-indexed inverse runs in this many
 *   unit groups, pipelined: the row index of group g + 1 (latency-bound) runs
 *   beside the reconstruction of group g on a second stream of the context;
 *   the call stays ordered on the context's stream.  Same cells.  Measured
 *   slower on MI355X (C2: 0.53 ms at 1 group, 0.62 at 2, 0.59 at 4), kept as
 *   an option for workloads whose row index dominates.
 * WC_OPT_ORDERED (default 1): the look-back kernels (forward emit, inverse
 *   row index and decode) take each block's tile index from the launch order
 *   (no atomic per block); 0 takes it from a per-unit ticket atomic instead.
 *   Same bytes out either way, and neither form depends on the order in which
 *   the hardware dispatches workgroups or on other kernels sharing the device:
 *   a block that has waited its bound (WC_OPT_SPIN_LIMIT) for a predecessor
 *   tile to publish derives that tile's count from the tile's own inputs and
 *   goes on (DESIGN.md §Forward progress).  Several contexts or processes may
 *   share a GPU in either form.  wc_get_option(WC_OPT_ORDERED) returns the form
 *   the next launch takes.
 * WC_OPT_TICKETS (default 0): 1 = this context uses the ticket form whatever
 *   WC_OPT_ORDERED says.
 * WC_OPT_SPIN_LIMIT (default 0 = 64 polls, about 0.1 ms): unanswered polls of
 *   an unpublished predecessor before a waiting block derives it itself.  Any
 *   value gives the same bytes; 1 makes nearly every wait take that path
 *   (tests).
 * WC_OPT_REVERSE_TILES (default 0; test hook): the launch-order form with each
 *   unit's tile indices reversed, so that every look-back waits on blocks
 *   dispatched after it (the worst dispatch order).  Same bytes, slower.
 * WC_OPT_INVERSE_ROWS (default 1): the inverse of even-dims units (W, H even,
 *   D % 8 == 0) indexes the payload's pairs by flat row and reconstructs each
 *   tile straight from the payload; 0 decodes every unit into a dense fp32
 *   coefficient scratch first (4 B/cell written and read back).  Same cells.
 * WC_OPT_RIX_LDS (default 9216), WC_OPT_RIX_TX (default 4): tile shape of the
 *   row-indexed inverse: LDS floats per workgroup (1024..16384) and log2 of the
 *   tile's blocks along x (0..5); y takes the rest of the budget.  A unit
 *   whose one-block tile needs more than the budget, 4 * D + 80 floats (D > 236
 *   at 1024, D > 2284 at the default), decodes densely, as with
 *   WC_OPT_INVERSE_ROWS 0.  The largest budget is a 64 KB tile, which
 *   launches as it is.  Same cells.
 * WC_OPT_RIX_BLOCKED (default 0): each workgroup of the row-indexed inverse
 *   runs a contiguous run of tiles (0: tiles b, b + grid, ...).  Same cells.
 * WC_OPT_HOST_CHUNK (default 2^25 cells): wc_forward_host splits a batch of
 *   more than two such chunks into contiguous unit runs of about this many
 *   cells (at most 16 runs) and pipelines them: the cells of run r+1 upload
 *   while run r computes and run r-1's packed payloads download.  Same bytes
 *   and offsets out; 0 = one run.  wc_inverse_host runs the same way (run
 *   r+1's payload bytes upload while run r decodes and run r-1's boxes
 *   download).
 * WC_OPT_HOST_THREADS (default: OMP_NUM_THREADS, else the cores, at most 16):
 *   wc_forward_host / wc_inverse_host make the pages of each destination span
 *   of the caller's host buffer resident (MADV_POPULATE_WRITE, no byte
 *   changed) from this many threads just before the device-to-host copy into
 *   it: a copy into never-touched pageable memory otherwise takes the page
 *   faults on its own thread (C2 payloads: 12-20 GB/s instead of the link's
 *   57).  0 = leave the faults to the copy.  Whole pages inside a span only.
 * WC_OPT_HOST_THP (default 0): 1 = also advise transparent huge pages
 *   (MADV_HUGEPAGE) on the 2-MiB-aligned interior of those spans first.  Off
 *   by default: the advice splits the caller's mappings and changes their
 *   huge-page policy for the life of the mapping (the caller owns its memory).
 * WC_OPT_TOL_SOLO_TILES (default 64): the RMSE-tolerance mode (wc_forward_tol)
 *   bins a unit of up to this many flat tiles (4096 coefficients each) in ONE
 *   workgroup (LDS bins only); a larger unit is split over several workgroups
 *   that add their bins to 16 KB of global bins of the unit.  Same thresholds
 *   and bytes either way; 1 splits every unit of two or more tiles (tests).
 *   From 63 up (the default included) the global bins take at most 1/64 of
 *   the split units' coefficient scratch.
 */
#define WC_OPT_SPARSE 12
#define WC_OPT_ORDERED 13
#define WC_OPT_INVERSE_ROWS 14
#define WC_OPT_RIX_LDS 15
#define WC_OPT_RIX_TX 16
#define WC_OPT_RIX_BLOCKED 17
#define WC_OPT_HOST_CHUNK 18
#define WC_OPT_SPIN_LIMIT 19
#define WC_OPT_TICKETS 20
#define WC_OPT_REVERSE_TILES 29
#define WC_OPT_RIX_XCD 22
#define WC_OPT_INV_GROUPS 23
/* 24, 25: retired (the round-4 cohort forward, removed: slower than the
 * two-kernel forward in every measured shape) */
#define WC_OPT_HOST_THREADS 27
#define WC_OPT_HOST_THP 28
#define WC_OPT_TOL_SOLO_TILES 30
int wc_set_option(wc_ctx* ctx, int option, int64_t value);
int wc_get_option(const wc_ctx* ctx, int option, int64_t* value);

/* Host-side helpers (no device work). */
uint64_t wc_payload_bound(const wc_unit* units, int n);  /* worst case: every coefficient kept */
uint64_t wc_cell_count(const wc_unit* units, int n);

/* Forward path for a batch: fp64/fp32 cells -> serialized payloads.
 * keep: the reference's `keep` (a float widened to double, src/argparse.h:13).
 * d_offsets: n+1 uint64, d_kept: n uint32 (both device).  payload_capacity must
 * be >= wc_payload_bound(units, n). */
int wc_forward(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
               double keep, uint8_t* d_payload, uint64_t payload_capacity,
               uint64_t* d_offsets, uint32_t* d_kept);

int wc_forward_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                    double keep, uint8_t* payload, uint64_t payload_capacity,
                    uint64_t* offsets, uint32_t* kept);

/* wc_forward_host with unit u's W*H*D cells at its own host pointer cells[u]
 * (units[u].cell_offset is ignored): the C++ mirror's compress() hands over
 * the Box3D components it was given (src/compressor.h:9-15) without packing
 * them into one buffer first.  Same payload, offsets and kept counts as
 * wc_forward_host of the packed components. */
int wc_forward_host_units(wc_ctx* ctx, const void* const* cells, int dtype, const wc_unit* units, int n,
                          double keep, uint8_t* payload, uint64_t payload_capacity,
                          uint64_t* offsets, uint32_t* kept);

/* The reference's -estimate round trip on host buffers (src/modes.cpp:236-291:
 * compress the boxes, decompress them again, calc_rmse_per_box against the
 * originals, src/calc-loss.cpp:12-43): wc_forward_host's outputs (packed
 * payloads, offsets, kept counts), plus rmse[u] = the RMSE of unit u's
 * reconstruction against its cells.  The payloads are decoded again on the
 * device with the forward's row index (wc_forward_rows / wc_inverse_rows) and
 * compared there with the cells already uploaded for the forward: the cells
 * cross PCIe once and the reconstruction never does.  RMSE identical to
 * wc_rmse_host of the decoded reconstruction. */
int wc_round_trip_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n, double keep,
                       uint8_t* payload, uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept,
                       double* rmse);

/* Opt-in global-threshold mode (NOT the reference's rule; BASELINE north_star's
 * "keep-percentile histogram + RCCL all-reduce").  The reference thresholds each
 * box at its own max * (1 - keep) (src/compressor.cpp:212-216); this mode picks
 * ONE fp32 threshold for a whole run from the coefficient-magnitude histogram
 * summed over every unit on every rank.  Payload format and decoder unchanged.
 *
 *   wc_forward_stage: transform a batch into the context's coefficient scratch
 *     (the first half of wc_forward) and, when d_hist is not null, ADD the
 *     batch's magnitude histogram to d_hist (WC_HIST_BINS uint64 on the device;
 *     bin = fp32 bits of |c| >> WC_HIST_SHIFT, NaN not counted).  The bins are
 *     counted as the transform stages the coefficients (no second pass over them).
 *   (caller: all-reduce d_hist over ranks, e.g. RCCL sum of 4096 uint64)
 *   wc_hist_threshold: host-only; the fp32 threshold that keeps every
 *     coefficient whose bin is >= the highest bin b at which the count of
 *     coefficients in bins >= b reaches N - floor(quantile * N), N = the total
 *     count (retained >= (1 - quantile) N, by less than one bin's population).
 *     *retained receives that count (may be null).
 *   wc_forward_emit: threshold + pack the staged batch; thresh = NULL applies
 *     the reference per-unit rule with `keep` (so stage + emit == wc_forward),
 *     else every coefficient with |c| > *thresh is kept.  Needs the staged
 *     coefficients of the same units: any other compute call on the context in
 *     between invalidates them (WC_ERR_INVALID). */
#define WC_HIST_BINS 4096
#define WC_HIST_SHIFT 19
int wc_forward_stage(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                     uint64_t* d_hist);
int wc_hist_threshold(const uint64_t* hist, double quantile, float* thresh, uint64_t* retained);
int wc_forward_emit(wc_ctx* ctx, const wc_unit* units, int n, double keep, const float* thresh,
                    uint8_t* d_payload, uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept);

/* Opt-in RMSE-tolerance mode (NOT the reference's rule): the caller states the
 * tolerated RMSE of each unit and the library finds the unit's threshold.  The
 * reference's only quality control is `keep` (threshold = the box's own max *
 * (1 - keep)), so the error of a box follows from its largest coefficient and
 * its -estimate mode exists to guess `keep` by trial.  Payload format and
 * decoder unchanged; only the threshold differs.
 *
 * With W, H and D all even the one-level transform (avg = (a+b)/2, diff =
 * (a-b)/2 per axis) is orthogonal and every basis vector has squared norm 8:
 * dropping the coefficient set S costs SSE = 8 * sum_S c^2, RMSE^2 = SSE / N.
 * A unit with an odd dimension has no such bound (the reference's inverse does
 * not restore the trailing plane of an odd axis) and is rejected.
 *
 * The selection rule, on one unit's N = W*H*D coefficients and its tolerance
 * tol (a double >= 0, +inf allowed; NaN or negative: WC_ERR_INVALID):
 *   cnt[b]  = coefficients with fp32 bits of |c| >> WC_HIST_SHIFT == b (the
 *             WC_HIST_BINS bins of the global-threshold mode; NaN not counted)
 *   hi_b    = (double) the float with bits (b + 1) << 19 for b < 0xFEF, +inf
 *             from there on: every |c| of bin b is < hi_b
 *   budget  = (tol * tol) * (double)N
 *   S = 0; for b = 0, 1, ... over the non-empty bins:
 *       t = S + (double)cnt[b] * (8.0 * (hi_b * hi_b));
 *       if !(t <= budget) stop: b* = b;  else S = t      (no stop: b* = 4096)
 *   thresh  = 0.0f if b* == 0 (every non-zero coefficient kept), FLT_MAX if
 *             b* >= 0xFF0 (only +-inf kept), else the float with bits
 *             (b* << 19) - 1: the emit's strict |c| > thresh keeps exactly the
 *             bins >= b*
 *   bound   = sqrt(S / N) (0 when N == 0): the guaranteed model RMSE of the
 *             choice, bound <= tol
 * in IEEE double with separately rounded multiplies and adds.  Only integer
 * counts enter: the result is the same bits on the host and the device and in
 * every run.  Conservative by less than one bin step (upper bin edges
 * overestimate the dropped energy by at most (17/16)^2).  The actual RMSE adds
 * the fp32 rounding of the round trip to the model's.
 *
 *   wc_tol_threshold: host-only; the rule on one unit's counts.
 *   wc_forward_tol: wc_forward with per-unit tolerances in place of keep.
 *     tol: n doubles on the HOST, consumed before the call returns.  d_thresh
 *     (n floats) and d_bound (n doubles): device, nullable.  The coefficients
 *     are staged densely (the threshold is not known when the transform runs)
 *     and read once more for the bins.  A unit with cells and an odd W, H or D:
 *     WC_ERR_INVALID, nothing launched.  A unit without cells keeps nothing.
 *   wc_forward_emit_tol: the staged form, after wc_forward_stage(..., NULL);
 *     may be repeated with other tolerances on the same staged batch.
 *   wc_forward_tol_host: host buffers; payloads packed as wc_forward_host;
 *     thresh, bound, rmse (n each, host, nullable); rmse = the ACTUAL RMSE of
 *     each unit's round trip, taken on the device (wc_inverse_rmse).  The unit
 *     runs (WC_OPT_HOST_CHUNK) go one after another. */
int wc_tol_threshold(const uint64_t* counts, uint64_t ncoeff, double tol, float* thresh, double* bound);
int wc_forward_tol(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n, const double* tol,
                   uint8_t* d_payload, uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept,
                   float* d_thresh, double* d_bound);
int wc_forward_emit_tol(wc_ctx* ctx, const wc_unit* units, int n, const double* tol, uint8_t* d_payload,
                        uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh,
                        double* d_bound);
int wc_forward_tol_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n, const double* tol,
                        uint8_t* payload, uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept,
                        float* thresh, double* bound, double* rmse);

/* Opt-in multi-level transform (NOT the reference's codec, which transforms
 * each box once): a unit with L >= 2 levels repeats the one-level transform on
 * the low-pass corner of its coefficient array, the Mallat pyramid in the
 * unit's own index space.  With one level the 1/8 low-pass octant holds values
 * of the data's own magnitude, every sensible threshold keeps all of it, and a
 * unit cannot shrink below about 1/4 of its fp32 cells; further levels shrink
 * that corner by 8 each.  levels = 1 is the existing codec, byte for byte.
 *
 * Definition.  Each unit has L in 1..WC_MAX_LEVELS.  A unit with cells and
 * L >= 2 needs W, H and D each divisible by 2^L.  A is the unit's flat array
 * in the x-slowest order (I*H + J)*D + K after the one-level transform
 * (wc_decompose).  For l = 2..L, with (w, h, d) = (W, H, D) >> (l-1):
 *   take the sub-box S(x, y, z) = A[(x*H + y)*D + z], x < w, y < h, z < d;
 *   apply the reference's one-level wavelet_decompose to S as a w x h x d box
 *     (Z, then Y, then X sweeps; low at m, high at n/2 + m; low = (a + b) * 0.5f,
 *     high = (a - b) * 0.5f in fp32), giving T in its flat order (I*h + J)*d + K;
 *   write it back: A[(I*H + J)*D + K] = T[(I*h + J)*d + K].
 * Threshold, mask, run lengths and serialisation then run on the final A
 * exactly as for one level: the keep rule's threshold is (1 - keep) * the
 * signed value at the FIRST flat index of the largest |c| of the final array;
 * a caller's explicit threshold is the alternative.  The inverse mirrors it:
 * decode to the dense A; for l = L..2 apply inverse_wavelet_decompose (X, Y, Z;
 * avg + diff, avg - diff) to the sub-box in place by the same index map; then
 * the one-level inverse.
 *
 * Header.  L = 1 writes the reference's header (ncoeff = W*H*D).  L >= 2
 * writes ncoeff = -L in that int32 field (W*H*D is redundant with W, H, D), so
 * every one-level decoder, the reference's included, refuses such a payload
 * instead of decoding garbage, and a payload or .xz file describes itself.
 * Slot offsets, pair layout and wc_payload_bound do not change.
 *
 * wc_forward_tol is one-level only: with L >= 2 the basis vectors of level l
 * have squared norm 8^l, so the rule needs per-level weights.  The _tol form of
 * these calls is wc_forward_levels_tol below, with one threshold per level.
 *
 *   wc_levels_for: host-only; the largest L <= min(want, WC_MAX_LEVELS) with
 *     2^L dividing nx, ny and nz; 1 if none does or the box has no cells.
 *   wc_payload_levels: host-only; L of a payload from its 20-byte header.
 *     WC_ERR_FORMAT for negative dims, an ncoeff that is neither W*H*D nor
 *     -2..-WC_MAX_LEVELS, or dims that 2^L does not divide; WC_ERR_INVALID for
 *     null pointers or len < 20.
 *   wc_forward_levels: wc_forward with levels[u] per unit (n int32 on the
 *     HOST, consumed before the call returns) and, as wc_forward_emit, thresh
 *     = NULL for the keep rule or a host pointer to one fp32 threshold (|c| >
 *     *thresh kept in every unit).  The coefficients are staged densely.  It
 *     leaves nothing staged: a following wc_forward_emit / _emit_tol returns
 *     WC_ERR_INVALID.
 *   wc_decompose_levels / wc_inverse_flat_levels: the transforms alone
 *     (wc_decompose / wc_inverse_flat with levels).
 *   wc_inverse_levels: wc_inverse of such payloads.  Every unit decodes through
 *     the dense coefficient scratch.  Unit u's header must carry levels[u], else
 *     WC_ERR_FORMAT at the next wc_synchronize as for other malformed headers;
 *     nothing past a mismatching header is read and the unit's cells in d_out
 *     stay untouched (the other units of the batch decode as usual).
 *   wc_forward_levels_host / wc_inverse_levels_host: host buffers; payloads
 *     packed as wc_forward_host; the unit runs (WC_OPT_HOST_CHUNK) go one after
 *     another.  wc_inverse_levels_host takes levels = NULL to read each L from
 *     its header on the host.
 * A level outside 1..WC_MAX_LEVELS, or a dimension that 2^L does not divide on
 * a unit with cells: WC_ERR_INVALID naming the unit, before anything is
 * launched; outputs stay untouched. */
#define WC_MAX_LEVELS 4
int wc_levels_for(int nx, int ny, int nz, int want);
int wc_payload_levels(const uint8_t* header, size_t len, int* levels);
int wc_forward_levels(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                      const int32_t* levels, double keep, const float* thresh, uint8_t* d_payload,
                      uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept);
int wc_decompose_levels(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                        const int32_t* levels, float* d_flat);
int wc_inverse_flat_levels(wc_ctx* ctx, const float* d_flat, const wc_unit* units, int n, const int32_t* levels,
                           float* d_out);
int wc_inverse_levels(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, float* d_out);
int wc_forward_levels_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                           const int32_t* levels, double keep, const float* thresh, uint8_t* payload,
                           uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept);
int wc_inverse_levels_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, float* out);

/* Opt-in RMSE tolerance on the multi-level transform (NOT the reference's
 * rule): the tolerated RMSE of each unit, as wc_forward_tol, on the final array
 * of wc_forward_levels, with one threshold per level.
 *
 * Setting.  A unit W x H x D with cells and L levels, 1 <= L <= WC_MAX_LEVELS;
 * 2^L divides W, H and D (for L = 1: even dimensions, as wc_forward_tol
 * demands).  A is the final flat array of wc_forward_levels in the x-slowest
 * order (I*H + J)*D + K, N = W*H*D.
 *
 * Level of a coefficient.  j* is the largest j in 0..L-1 with I < W>>j,
 * J < H>>j and K < D>>j; lvl(I, J, K) = j* + 1 (the low-pass corner has level
 * L).  The basis vectors of level l have squared norm 8^l: dropping the set S
 * costs SSE = sum_S 8^lvl * c^2, exact for the real-number transform;
 * RMSE^2 = SSE / N.
 *
 * The selection rule, on the unit's tolerance tol (a double >= 0, +inf
 * allowed; NaN or negative: WC_ERR_INVALID):
 *   cnt[l][b] = coefficients of level l with fp32 bits of |c| >> WC_HIST_SHIFT
 *               == b (the WC_HIST_BINS bins; NaN not counted)
 *   hi_b      = as in wc_tol_threshold
 *   budget    = (tol * tol) * (double)N
 *   S = 0; visit the pairs (s, l) in lexicographic order, s = 0 .. 4095 +
 *   WC_LTOL_SHIFT*(L-1), then l = 1..L, with b = s - WC_LTOL_SHIFT*(l-1)
 *   (WC_LTOL_SHIFT = 24 bins = 1.5 octaves of 16 bins, about the factor sqrt(8)
 *   between the levels' weights); a pair whose b is outside 0..4095 or whose
 *   cnt[l][b] == 0 is skipped; at each visited pair
 *       t = S + (double)cnt[l][b] * ((double)8^l * (hi_b * hi_b));
 *       if !(t <= budget) stop at (s*, l*);  else S = t
 *   bstar_l   = clamp(s* + (l < l* ? 1 : 0) - WC_LTOL_SHIFT*(l-1), 0, 4096), the
 *               first kept bin of level l (no stop: 4096 for every level)
 *   thresh_l  = from bstar_l as wc_tol_threshold's thresh from b*: 0.0f at 0,
 *               FLT_MAX from 0xFF0 up, else the float with bits
 *               (bstar_l << 19) - 1
 *   bound     = sqrt(S / N) (0 when N == 0), bound <= tol
 * in IEEE double, every multiply and add rounded on its own; 8^l is an exact
 * double.  Only integer counts enter: the host, the device and every run give
 * the same bits.  With L = 1 the rule is wc_tol_threshold operation for
 * operation, and an L = 1 unit gets the bits and bytes of wc_forward_tol.
 *
 * Payload.  The pairs of exactly the coefficients with |c| > thresh_lvl
 * (strict: NaN is never kept), in flat order, with the reference's run-length
 * rule and serialisation and the header of wc_forward_levels (ncoeff = -L for
 * L >= 2).  The format does not change: wc_inverse_levels, wc_inverse_coarse
 * and their _host forms decode these payloads as they are.
 *
 *   wc_tol_levels_threshold: host-only; the rule on one unit's counts
 *     (levels x WC_HIST_BINS uint64, level-major); thresh receives `levels`
 *     floats, bound is nullable.  WC_ERR_INVALID for null pointers, a NaN or
 *     negative tol, or levels outside 1..WC_MAX_LEVELS.
 *   wc_forward_levels_tol: wc_forward_levels with per-unit tolerances in place
 *     of keep / thresh.  levels (n int32) and tol (n doubles): HOST, consumed
 *     before the call returns.  d_thresh: n x WC_MAX_LEVELS floats on the
 *     device, nullable; unit u's level l at u*WC_MAX_LEVELS + l - 1, entries
 *     past levels[u] written 0.0f.  d_bound: n doubles on the device, nullable.
 *     Slots, offsets and wc_payload_bound as in wc_forward_levels.  The
 *     coefficients are staged densely, read once for the bins and masked in
 *     place by the per-level thresholds before the emit.  It leaves nothing
 *     staged (there is no _emit form).  A unit without cells keeps nothing.
 *   wc_forward_levels_tol_host: host buffers; payloads packed as
 *     wc_forward_host; thresh (n x WC_MAX_LEVELS), bound, rmse (n each): host,
 *     nullable; rmse = the ACTUAL RMSE of each unit's round trip, taken on the
 *     device (wc_inverse_levels + wc_rmse).  The unit runs (WC_OPT_HOST_CHUNK)
 *     go one after another.
 * What wc_forward_levels refuses (a level outside 1..WC_MAX_LEVELS, a dimension
 * that 2^L does not divide) and what wc_forward_tol refuses (a NaN or negative
 * tolerance, a unit with cells and an odd dimension, which here can only be an
 * L = 1 unit): WC_ERR_INVALID naming the unit, before anything is launched;
 * outputs stay untouched. */
#define WC_LTOL_SHIFT 24
int wc_tol_levels_threshold(const uint64_t* counts, int levels, uint64_t ncoeff, double tol, float* thresh,
                            double* bound);
int wc_forward_levels_tol(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                          const int32_t* levels, const double* tol, uint8_t* d_payload, uint64_t payload_capacity,
                          uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound);
int wc_forward_levels_tol_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                               const int32_t* levels, const double* tol, uint8_t* payload, uint64_t payload_capacity,
                               uint64_t* offsets, uint32_t* kept, float* thresh, double* bound, double* rmse);

/* Opt-in size budget on the multi-level transform (NOT the reference's rule):
 * each unit keeps its max_pairs largest weighted coefficients and never more,
 * so its payload is at most 20 + 8 * max_pairs bytes (a pair is one kept
 * coefficient: a byte budget is a pair budget).  The selection is exact, by a
 * three-digit radix select on a 32-bit integer key.
 *
 * Setting, as for wc_forward_levels_tol.  A unit W x H x D with cells and L
 * levels, 1 <= L <= WC_MAX_LEVELS; 2^L divides W, H and D (for L = 1: even
 * dimensions).  A is the final flat array of wc_forward_levels, N = W*H*D;
 * lvl(I, J, K) as defined above.  The caller gives max_pairs[u] = K, a uint32.
 *
 * Candidates.  For a coefficient c, m = the fp32 bits of |c| (bits &
 * 0x7FFFFFFF).  c is a candidate iff 1 <= m <= 0x7F800000: +-0 and NaN are
 * never kept, +-inf is a candidate.
 * Key.  key(c) = m + ((WC_LTOL_SHIFT * (lvl - 1)) << WC_HIST_SHIFT): the
 * magnitude's bit pattern moved up by 24 bins (1.5 octaves, about sqrt(8)) per
 * level, the weighting wc_forward_levels_tol uses between levels.  The largest
 * key is 0x7F800000 + (72 << 19) = 0x81C00000.
 * Selection.  With at most K candidates T = 0.  Otherwise T = the (K + 1)-th
 * largest key, counted with multiplicity.  Kept = the candidates with key > T:
 * kept <= K always, and with more than K candidates kept + #{key == T} >=
 * K + 1.  Candidates whose key EQUALS T (the same magnitude bits at the same
 * level, or a coincidence across levels) are ALL dropped: there is no
 * positional tie-break, so a unit with ties at the boundary keeps fewer than K
 * (a constant box with a budget below its candidate count keeps nothing).
 * Per-level thresholds.  d = T - ((WC_LTOL_SHIFT * (l - 1)) << WC_HIST_SHIFT)
 * as a signed 64-bit value; thresh_l = the float with bits 0 if d <= 0,
 * 0x7F800000 (+inf) if d >= 0x7F800000, d otherwise.  "|c| > thresh_l"
 * (strict, false for NaN) is then exactly "candidate and key > T".
 * Only integers enter: the host, the device and every run give the same bits.
 *
 * Payload.  The pairs of exactly those coefficients, in flat order, with the
 * header of wc_forward_levels (ncoeff = -L for L >= 2); 20 + 8 * kept bytes.
 * Slots, offsets and wc_payload_bound as in wc_forward_levels.  K >= the
 * candidate count gives the bytes of wc_forward_levels with the explicit
 * threshold 0.0f.  The decoders need no change.  A unit without cells keeps
 * nothing.
 *
 *   wc_budget_thresholds: host-only; T -> thresh_1..levels.
 *   wc_budget_select: host-only; the rule on one unit's final flat array
 *     (nx * ny * nz floats, x slowest).  key receives T; thresh (levels floats)
 *     and kept (#{key > T}) are nullable.
 *   wc_forward_levels_budget: wc_forward_levels with per-unit pair budgets in
 *     place of keep / thresh.  levels (n int32, NULL = all 1) and max_pairs (n
 *     uint32): HOST, consumed before the call returns.  d_thresh (n x
 *     WC_MAX_LEVELS floats, entries past levels[u] written 0.0f) and d_key (n
 *     uint32, unit u's T): device, nullable.  Asynchronous on the context's
 *     stream; nothing is read back between its passes.  It leaves nothing
 *     staged.
 *   wc_forward_levels_budget_host: host buffers; payloads packed as
 *     wc_forward_host; thresh (n x WC_MAX_LEVELS), key, rmse (n each): host,
 *     nullable; rmse = the ACTUAL RMSE of each unit's round trip, taken on the
 *     device (wc_inverse_levels + wc_rmse).  The unit runs (WC_OPT_HOST_CHUNK)
 *     go one after another.
 * A level outside 1..WC_MAX_LEVELS, a dimension that 2^L does not divide on a
 * unit with cells (for L = 1: an odd dimension) or a null required buffer:
 * WC_ERR_INVALID naming the unit, before anything is launched; outputs stay
 * untouched. */
int wc_budget_thresholds(uint32_t key, int levels, float* thresh);
int wc_budget_select(const float* flat, int32_t nx, int32_t ny, int32_t nz, int levels, uint32_t max_pairs,
                     uint32_t* key, float* thresh, uint32_t* kept);
int wc_forward_levels_budget(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                             const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_payload,
                             uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh,
                             uint32_t* d_key);
int wc_forward_levels_budget_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                                  const int32_t* levels, const uint32_t* max_pairs, uint8_t* payload,
                                  uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept, float* thresh,
                                  uint32_t* key, double* rmse);

/* Opt-in pointwise (max-abs) error bound on the multi-level transform (NOT the
 * reference's rule): the caller states E per unit and no cell of the unit's
 * reconstruction is further than E from the original.  An RMSE tolerance says
 * nothing about the worst cell.  The Haar model gives only the analytic bound
 * T <= E / (7L + 1) (a cell depends on 7 detail coefficients per level plus one
 * low-pass value, each with weight +-1), which is 3 to 6 times below what the
 * data allows; this mode VERIFIES candidate thresholds on the device instead,
 * by the round trip itself.
 *
 * Setting.  A unit W x H x D with cells and L levels, 1 <= L <= WC_MAX_LEVELS;
 * 2^L divides W, H and D (for L = 1: even dimensions), exactly what
 * wc_forward_levels_tol accepts.  x = the caller's cells in the caller's dtype
 * (fp64 cells before narrowing).  A = the final flat array of
 * wc_forward_levels.  E = the unit's bound, a double >= 0, +inf allowed; NaN or
 * negative: WC_ERR_INVALID naming the unit, before anything is launched.
 *
 * Definitions.
 *   thr(b)  for b in 0..4095, wc_tol_threshold's threshold from a first kept
 *           bin: 0.0f at b = 0, FLT_MAX from 0xFF0 up, else the float with bits
 *           (b << WC_HIST_SHIFT) - 1
 *   R_b     wc_inverse_flat_levels of A with every coefficient that is not
 *           |c| > thr(b) replaced by +0.0f (strict: NaN is dropped); bit for
 *           bit what wc_inverse_levels returns for the payload written at that
 *           threshold
 *   err(b)  the max over the cells of |(double)x - (double)R_b|, taken over the
 *           differences that are not NaN; 0.0 if there are none.  A max does
 *           not depend on order: the host, the device and every run give the
 *           same bits.
 *
 * Search (radix 16, three passes; fixed, so that the result is defined).
 *   lo = 0
 *   for stride = 256, 16, 1:
 *       j* = the largest j in 0..15 such that err(lo + i*stride) <= E for
 *            every i in 1..j;  lo += j* * stride
 *   b* = lo, thresh = thr(b*), err = err(b*)
 * err <= E holds whenever b* > 0.  b* = 0 is accepted unverified: it keeps
 * every non-zero coefficient, its err is the fp32 rounding of the round trip
 * and may exceed a tiny E; the caller sees that in err.  err(b) is NOT monotone
 * in b (dropped coefficients cancel: of 400 random 4x4x4 boxes of integers in
 * -8..8 at L = 2, 380 show a decreasing step), so the leading run above is the
 * definition and "the largest b with err(b) <= E" is not.  In L-inf every level
 * weighs +-1, so one threshold for all levels is the natural rule.
 *
 * Payload.  Byte for byte what wc_forward_levels writes for that unit with the
 * explicit threshold thr(b*).  The format does not change: every decoder,
 * wc_pack, the thinning, split and merge read it as any payload.  A unit
 * without cells keeps nothing, with thresh 0.0f and err 0.0.
 *
 *   wc_maxerr_select: host-only; the rule on one unit in plain C++ (flat: the
 *     final array, nx * ny * nz floats, x slowest; cells: the unit's cells in
 *     dtype, x fastest).  thresh, err and bstar are nullable.
 *   wc_forward_levels_maxerr: wc_forward_levels with per-unit bounds in place
 *     of keep / thresh.  levels (n int32, NULL = all 1) and maxerr (n doubles):
 *     HOST, consumed before the call returns.  d_thresh (n floats, ONE per
 *     unit) and d_err (n doubles): device, nullable.  Asynchronous on the
 *     context's stream; nothing is read back between its passes (46 probes per
 *     unit in three launches).  It leaves nothing staged.
 *   wc_forward_levels_maxerr_host: host buffers; payloads packed as
 *     wc_forward_host; thresh, err, rmse (n each): host, nullable; rmse = the
 *     RMSE of each unit's round trip, taken on the device (wc_inverse_levels +
 *     wc_rmse).  The unit runs (WC_OPT_HOST_CHUNK) go one after another.
 *   wc_maxerr / wc_maxerr_host: the L-inf sibling of wc_rmse: per unit the max
 *     of |(double)orig - (double)regen| over the non-NaN differences, 0.0 for a
 *     unit without cells.  Any reconstruction, the reference mode's included.
 * A level outside 1..WC_MAX_LEVELS, a dimension that 2^L does not divide on a
 * unit with cells (for L = 1: an odd dimension), a NaN or negative bound or a
 * null required buffer: WC_ERR_INVALID naming the unit, before anything is
 * launched; outputs stay untouched.
 *
 * Out of scope: a CLI option, a compressed-domain (wc_thin_*) form, the
 * global-threshold mode, and per-level thresholds. */
int wc_maxerr_select(const float* flat, const void* cells, int dtype, int32_t nx, int32_t ny, int32_t nz, int levels,
                     double maxerr, float* thresh, double* err, uint32_t* bstar);
int wc_forward_levels_maxerr(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                             const int32_t* levels, const double* maxerr, uint8_t* d_payload,
                             uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh,
                             double* d_err);
int wc_forward_levels_maxerr_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                                  const int32_t* levels, const double* maxerr, uint8_t* payload,
                                  uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept, float* thresh,
                                  double* err, double* rmse);
int wc_maxerr(wc_ctx* ctx, const void* d_orig, int dtype, const float* d_regen, const wc_unit* units, int n,
              double* d_err);
int wc_maxerr_host(wc_ctx* ctx, const void* orig, int dtype, const float* regen, const wc_unit* units, int n,
                   double* err);

/* Opt-in thinning in the compressed domain (not in the reference): a standard
 * payload becomes a smaller one under a tighter pair budget or under per-level
 * thresholds, without its cells or its dense coefficients ever existing.  The
 * work follows the payload's pairs, not the box.
 *
 * The rule.  P is a standard payload of a unit W x H x D with L levels (L from
 * its header, as wc_payload_levels), N = W*H*D.  A(P) is the dense flat array
 * rle_decode gives: pair k sits at p_k = sum_{j<=k}(run_j + 1) - 1, a pair whose
 * position reaches N is dropped, everything else is 0.0f.
 *   thin_budget(P, K) = the bytes wc_forward_levels_budget's selection and emit
 *     give on A(P): candidates 1 <= m <= 0x7F800000, key = m + ((WC_LTOL_SHIFT *
 *     (lvl - 1)) << WC_HIST_SHIFT), T = the (K + 1)-th largest key or 0 with at
 *     most K candidates, kept = key > T (ties at T are all dropped), the header of
 *     wc_forward_levels and the reference's run rule on the kept set.
 *   thin_thresh(P, t_1..t_L) keeps exactly the entries with |c| > t_lvl (strict:
 *     NaN is never kept).  Each t_l is a float >= 0, +inf allowed; a NaN or
 *     negative threshold is WC_ERR_INVALID.
 * Consequences: a pair with value +-0 or NaN, or past N, is never in the output;
 * kept <= min(K, pairs); the output is never longer than the input; thinning is
 * idempotent at the same K or thresholds; thinning a thresh = t0 payload at
 * per-level thresholds all equal to t1 >= t0 gives the bytes of wc_forward_levels
 * with the explicit threshold t1; thinning a thresh = 0.0f payload with budget K
 * gives the bytes of wc_forward_levels_budget with K whenever the payload holds
 * every candidate.  Unit shapes: those wc_forward_levels accepts.  A packed unit
 * is refused (WC_ERR_FORMAT): wc_unpack first.
 *
 *   wc_thin_unit: host-only, no device; the rule on one payload of `len` bytes.
 *     Exactly one of max_pairs (K) and thresh (levels floats) is non-NULL.  out
 *     receives at most `cap` bytes, *written their count.  key (T; 0 for the
 *     threshold form) and thresh_out (levels floats) are nullable.  A header that
 *     is not a standard one, or a negative run: WC_ERR_FORMAT, nothing written.
 *   wc_thin_bound: the output extent of the device forms.  Unit u's slot is the
 *     prefix, starting at 4, of 24 + 8 * cap_u; cap_u = min(max_pairs[u], N_u), or
 *     N_u with max_pairs NULL (the threshold form: wc_payload_bound).
 *   wc_thin_budget / wc_thin_thresh: payloads at d_payload + d_offsets[u]
 *     (multiples of 4) -> slots in d_out (16-B aligned).  levels, max_pairs and
 *     thresh (n x WC_MAX_LEVELS, unit u's level l at u*WC_MAX_LEVELS + l - 1):
 *     HOST, consumed before the call returns.  d_out_offsets (n + 1; [n] = the end
 *     of the last unit's bytes), d_kept (n): device.  d_thresh and d_key: device,
 *     nullable, as in wc_forward_levels_budget.  Asynchronous on the context's
 *     stream; nothing is read back between the passes; nothing is left staged.
 *     out_capacity < wc_thin_bound, or d_payload inside the output's extent:
 *     WC_ERR_INVALID.  The outputs must not overlap the input.
 *     A header that disagrees with the unit (box, levels, a packed tag) raises
 *     WC_ERR_FORMAT at the next wc_synchronize; that unit's slot stays untouched
 *     and its d_kept is 0; the other units are thinned.  A negative run raises
 *     the same error; that unit's output is unspecified but inside its slot.
 *     Scratch of the context: 12 B per coefficient the units can hold, rounded up
 *     to tiles of 4096 (the pair count of a payload is not known to the host).
 *   wc_thin_budget_host / wc_thin_thresh_host: host buffers; the results packed
 *     densely as wc_forward_host's (out_capacity >= wc_thin_bound(units, n,
 *     max_pairs); out_offsets n + 1).  levels NULL reads the headers.  A header
 *     that disagrees fails the call (WC_ERR_FORMAT) before anything runs.  The
 *     unit runs (WC_OPT_HOST_CHUNK) go one after another. */
int wc_thin_unit(const uint8_t* payload, size_t len, const uint32_t* max_pairs, const float* thresh, uint8_t* out,
                 size_t cap, size_t* written, uint32_t* key, float* thresh_out);
uint64_t wc_thin_bound(const wc_unit* units, int n, const uint32_t* max_pairs);
int wc_thin_budget(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_out, uint64_t out_capacity,
                   uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key);
int wc_thin_thresh(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const float* thresh, uint8_t* d_out, uint64_t out_capacity,
                   uint64_t* d_out_offsets, uint32_t* d_kept);
int wc_thin_budget_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                        const int32_t* levels, const uint32_t* max_pairs, uint8_t* out, uint64_t out_capacity,
                        uint64_t* out_offsets, uint32_t* kept, float* thresh, uint32_t* key);
int wc_thin_thresh_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                        const int32_t* levels, const float* thresh, uint8_t* out, uint64_t out_capacity,
                        uint64_t* out_offsets, uint32_t* kept);

/* Thinning and splitting to an RMSE tolerance in the compressed domain (not in the
 * reference): the third selection rule of the thinning above.  The caller states
 * an error per unit, as for wc_forward_levels_tol, and the rule of that mode runs
 * on the payload's pairs: no cell and no dense coefficient exists.
 *
 * The rule.  P, W x H x D, L, N and A(P) as in the thinning rule above; lvl and
 * the selection rule as in wc_forward_levels_tol's section.
 *   thin_tol(P, tol):
 *   1. cnt[l][b] = the counts wc_forward_levels_tol's rule takes on A(P), from the
 *      pairs alone: a pair below N at level l with magnitude bits m <= 0x7F800000
 *      counts in bin m >> WC_HIST_SHIFT; a NaN pair below N counts nowhere; bin 0
 *      of level l additionally gets N_l - (pairs of level l below N, NaN
 *      included), the exact zeros of A(P); N_l = the positions of level l =
 *      prod(dims >> (l-1)) - prod(dims >> l) for l < L, prod(dims >> (L-1)) for
 *      l = L.
 *   2. (thresh_1..L, bound) = wc_tol_levels_threshold(cnt, L, N, tol), operation
 *      for operation.
 *   3. The output is thin_thresh(P, thresh_1..L).
 *   split_tol(P, tol) = (base, rest): base = thin_tol(P, tol), rest = its
 *   complement in canon(P), exactly as in split_thresh (canon, split and merge:
 *   the progressive layers' section below).
 * Units: those wc_forward_levels_tol accepts (even dimensions at L = 1, 2^L
 * dividing the box otherwise); a unit without cells keeps nothing, bound 0.
 * Consequences: on a NaN-free payload that holds every candidate (a thresh = 0.0f
 * payload), thin_tol(P, tol) is byte for byte wc_forward_levels_tol at tol,
 * thresholds and bound included (a NaN coefficient is "not counted" by the forward
 * but a zero of A(P): NaN-bearing units are outside this equality only);
 * tol = 0 gives canon(P); tol = +inf drops every finite pair (thresh_l = FLT_MAX:
 * a +-inf pair stays, as in the forward); merge(split_tol(P, tol)) == canon(P);
 * bound <= tol; bound is the RMSE this thinning adds for the real-number
 * transform, and the sets successive thinnings drop are disjoint, so the squares
 * of their bounds add: a payload written at tol0 and thinned with bound1 is
 * within sqrt(tol0^2 + bound1^2) of the original.
 *
 *   wc_thin_tol_unit / wc_split_tol_unit: host-only, no device; the rule on one
 *     payload, on wc_thin_unit / wc_split_unit.  thresh_out (levels floats) and
 *     bound are nullable.  A NaN or negative tol, or a box the mode does not
 *     accept: WC_ERR_INVALID; otherwise as wc_thin_unit / wc_split_unit.
 *   wc_thin_tol / wc_split_tol: the arguments of wc_thin_thresh / wc_split_thresh
 *     with tol (n doubles, HOST, consumed before the call returns) in place of
 *     thresh, and d_thresh (n x WC_MAX_LEVELS floats, entries past levels[u]
 *     written 0.0f) and d_bound (n doubles): device, nullable.  Capacities:
 *     wc_thin_bound(units, n, NULL) and wc_split_bound(units, n, NULL, ..).
 *     Asynchronous on the context's stream; nothing is read back between the
 *     passes; nothing is left staged.  A NaN or negative tolerance, or a unit
 *     with cells and an odd dimension (an L = 1 unit): WC_ERR_INVALID naming the
 *     unit, before anything is launched; outputs stay untouched.  A packed unit
 *     or a header that disagrees with its unit: as in wc_thin_thresh (its slot
 *     untouched, its counts 0; its d_thresh and d_bound entries are written 0).
 *     Scratch: the thinning's 12 B (the split's 16 B) per coefficient, and 64 KiB
 *     of bins per unit of more than WC_OPT_TOL_SOLO_TILES pair tiles.
 *   wc_thin_tol_host / wc_split_tol_host: host buffers, as wc_thin_thresh_host /
 *     wc_split_thresh_host; thresh (n x WC_MAX_LEVELS) and bound (n): host,
 *     nullable. */
int wc_thin_tol_unit(const uint8_t* payload, size_t len, double tol, uint8_t* out, size_t cap, size_t* written,
                     float* thresh_out, double* bound);
int wc_split_tol_unit(const uint8_t* payload, size_t len, double tol, uint8_t* base, size_t base_cap, size_t* base_len,
                      uint8_t* rest, size_t rest_cap, size_t* rest_len, float* thresh_out, double* bound);
int wc_thin_tol(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const double* tol, uint8_t* d_out, uint64_t out_capacity,
                uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound);
int wc_split_tol(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                 const int32_t* levels, const double* tol, uint8_t* d_base, uint64_t base_capacity,
                 uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                 uint64_t* d_rest_offsets, uint32_t* d_rest_pairs, float* d_thresh, double* d_bound);
int wc_thin_tol_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                     const int32_t* levels, const double* tol, uint8_t* out, uint64_t out_capacity,
                     uint64_t* out_offsets, uint32_t* kept, float* thresh, double* bound);
int wc_split_tol_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                      const int32_t* levels, const double* tol, uint8_t* base, uint64_t base_capacity,
                      uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                      uint64_t* rest_offsets, uint32_t* rest_pairs, float* thresh, double* bound);

/* Opt-in progressive layers in the compressed domain (not in the reference): the
 * complement of a thinning, and the union of payloads.  A payload becomes a stack
 * of layers; any prefix of the stack, merged, is a standard payload every decoder
 * reads unchanged.  No cell and no dense coefficient exists for either call.
 *
 * The rule.  P is a standard payload of a unit W x H x D with L levels, N = W*H*D.
 * A(P) and the positions p_k are the thinning rule's above: exact 64-bit sums, a
 * pair at or past N is dropped.
 *   canon(P) = thin_thresh(P, 0, .., 0): the pairs of P below N whose magnitude
 *     bits m satisfy 1 <= m <= 0x7F800000 (no +-0, no NaN), runs recomputed.  Every
 *     payload an encoder of this project emits is its own canonical form.
 *   split_budget(P, K) = (base, rest), split_thresh(P, t_1..t_L) = (base, rest):
 *     two standard payloads with P's header fields (W, H, D, ncoeff / -L).
 *     base is exactly thin_budget(P, K), respectively thin_thresh(P, t): the same
 *     bytes, kept count, T and per-level thresholds.  rest holds the pairs of
 *     canon(P) that are not in base, in position order, runs recomputed by the
 *     reference's run rule: in the budget form the candidates with key <= T (ties
 *     at T included), in the threshold form the candidates with |c| <= t_lvl.
 *   Consequences: the positions of base and rest are disjoint; pairs(base) +
 *     pairs(rest) = pairs(canon(P)); split(rest, K2) yields the next layer; the
 *     first j layers together are the candidates with key above the j-th T.
 *   merge(a, b), a and b standard payloads of the same unit and the same L: the
 *     standard payload with that header whose pairs are all pairs of a and of b at
 *     positions below N, in position order, value bits verbatim (nothing is
 *     dropped for being +-0 or NaN), runs recomputed.  A pair of a and a pair of
 *     b at the same position below N: the unit is refused (WC_ERR_FORMAT); layers
 *     are disjoint by construction, there is no override or sum semantic.
 *   Consequences: A(merge(a, b)) = A(a) + A(b) exactly; merge is commutative and
 *     associative; merge(a, empty) = a without its pairs past N;
 *     merge(split(P)) == canon(P) byte for byte, hence == P for every P an encoder
 *     emitted; merge(a, b) has at most 20 + 8 min(N, pairs(a) + pairs(b)) bytes.
 * Packed units are refused (WC_ERR_FORMAT): wc_unpack first.  Unit shapes: those
 * wc_forward_levels accepts.
 *
 *   wc_split_unit / wc_merge_unit: host-only, no device; the rule on one unit.
 *     wc_split_unit takes exactly one of max_pairs (K) and thresh (levels floats);
 *     key and thresh_out are nullable, as in wc_thin_unit.  A header that is not a
 *     standard one, a negative run, headers of a and b that differ (box or L), or
 *     an overlap: WC_ERR_FORMAT.  A short input or output buffer: WC_ERR_INVALID.
 *     Nothing is written on either.
 *   wc_split_bound: the output extents of the split's device forms.  The base's
 *     is wc_thin_bound's; unit u's rest slot is the prefix, starting at 4, of
 *     24 + 8 N_u (wc_payload_bound's layout: the pair count of a payload is not
 *     known to the host).  wc_merge_bound = wc_payload_bound.
 *   wc_split_budget / wc_split_thresh: payloads at d_payload + d_offsets[u]
 *     (multiples of 4) -> slots in d_base and d_rest (16-B aligned); d_base_offsets
 *     and d_rest_offsets (n + 1), d_kept and d_rest_pairs (n): device.  d_thresh,
 *     d_key: device, nullable.  levels, max_pairs, thresh: HOST, consumed before
 *     the call returns.  Asynchronous on the context's stream; nothing is read back
 *     between the passes; nothing is left staged.  The outputs must not overlap
 *     the input or each other.  Scratch of the context: 16 B per coefficient the
 *     units can hold, in tiles of 4096 (the thinning's 12 B and the rest's
 *     positions).
 *   wc_merge: payloads at d_a + d_a_offsets[u] and d_b + d_b_offsets[u] -> slots
 *     in d_out, d_out_offsets (n + 1), d_pairs (n).  d_a and d_b may be the same
 *     buffer with different offsets; the output must not overlap either input.
 *     Scratch: 8 B per coefficient the units can hold, in tiles of 4096.
 *   Errors of the device forms.  A capacity below the bound, or an output that
 *     starts inside an input's or another output's extent: WC_ERR_INVALID, nothing
 *     launched.  A header that disagrees with the unit (box, levels, a packed tag,
 *     an offset that is no multiple of 4; for wc_merge either input's, so headers
 *     of a and b that differ): WC_ERR_FORMAT at the next wc_synchronize, that
 *     unit's slots stay untouched and its counts are 0, the other units are
 *     processed.  A negative run: as in thinning.  An overlap in wc_merge:
 *     WC_ERR_FORMAT at the next wc_synchronize, that unit's output is a header with
 *     0 pairs and d_pairs[u] = 0, bytes past the header are unspecified but inside
 *     its slot, the other units are merged.
 *   _host forms: host buffers, results packed densely as wc_forward_host's
 *     (capacities >= the bounds), levels NULL reads the headers, a header (for
 *     wc_merge_host a header pair) that disagrees fails the call (WC_ERR_FORMAT)
 *     before anything runs.  The unit runs (WC_OPT_HOST_CHUNK) go one after
 *     another. */
int wc_split_unit(const uint8_t* payload, size_t len, const uint32_t* max_pairs, const float* thresh, uint8_t* base,
                  size_t base_cap, size_t* base_len, uint8_t* rest, size_t rest_cap, size_t* rest_len, uint32_t* key,
                  float* thresh_out);
int wc_merge_unit(const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint8_t* out, size_t cap,
                  size_t* written);
int wc_split_bound(const wc_unit* units, int n, const uint32_t* max_pairs, uint64_t* base_bytes, uint64_t* rest_bytes);
uint64_t wc_merge_bound(const wc_unit* units, int n);
int wc_split_budget(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_base, uint64_t base_capacity,
                    uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                    uint64_t* d_rest_offsets, uint32_t* d_rest_pairs, float* d_thresh, uint32_t* d_key);
int wc_split_thresh(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const float* thresh, uint8_t* d_base, uint64_t base_capacity,
                    uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                    uint64_t* d_rest_offsets, uint32_t* d_rest_pairs);
int wc_merge(wc_ctx* ctx, const uint8_t* d_a, const uint64_t* d_a_offsets, const uint8_t* d_b,
             const uint64_t* d_b_offsets, const wc_unit* units, int n, const int32_t* levels, uint8_t* d_out,
             uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_pairs);
int wc_split_budget_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const uint32_t* max_pairs, uint8_t* base, uint64_t base_capacity,
                         uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                         uint64_t* rest_offsets, uint32_t* rest_pairs, float* thresh, uint32_t* key);
int wc_split_thresh_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                         const int32_t* levels, const float* thresh, uint8_t* base, uint64_t base_capacity,
                         uint64_t* base_offsets, uint32_t* kept, uint8_t* rest, uint64_t rest_capacity,
                         uint64_t* rest_offsets, uint32_t* rest_pairs);
int wc_merge_host(wc_ctx* ctx, const uint8_t* a, const uint64_t* a_offsets, const uint8_t* b, const uint64_t* b_offsets,
                  const wc_unit* units, int n, const int32_t* levels, uint8_t* out, uint64_t out_capacity,
                  uint64_t* out_offsets, uint32_t* pairs);

/* Opt-in reduced-resolution decode (not in the reference): the box at 1/2^r
 * resolution straight from a payload, without the work of the full resolution.
 * The low-pass corner of the coefficient array after undoing levels L..r+1 is
 * that box; because the low-pass is (a + b) * 0.5f per axis, each of its cells
 * is the mean of a 2^r x 2^r x 2^r block of the full reconstruction up to fp32
 * rounding (the "average down" of AMR codes).  It works on one-level payloads
 * too, the reference's own file format: r = 1 of an even-sized box.
 *
 * Definition.  A unit is W x H x D with L levels; its payload is as
 * wc_forward_levels writes it (ncoeff = W*H*D for L = 1, -L for L >= 2).  The
 * unit has a reduction r, 0 <= r <= L; for r >= 1 on a unit with cells 2^r must
 * divide W, H and D (for L >= 2 the levels rule guarantees it; for L = 1, r = 1
 * it means even dimensions).  Write (w, h, d) = (W, H, D) >> r.
 *   1. A is the dense flat array of the payload in x-slowest order
 *      (I*H + J)*D + K: rle_decode, pairs at or past W*H*D dropped.
 *   2. Take the corner C(I, J, K) = A[(I*H + J)*D + K], I < w, J < h, K < d,
 *      stored compactly as C[(I*h + J)*d + K].
 *   3. r = L: the result is C read as a Box3D, out[x + w*(y + h*z)] = C(x, y, z);
 *      no arithmetic runs.  r < L: the result is the multi-level inverse
 *      (wc_inverse_flat_levels) of the flat array C of a w x h x d unit with
 *      L - r levels; with L - r = 1 that is the plain inverse_wavelet_decompose.
 *   4. r = 0 is wc_inverse_levels bit for bit.
 * Step 3 is exact, not an approximation: the synthesis of level l touches only
 * the corner (W, H, D) >> (l-1), so levels L..r+1 of the full inverse act on C
 * exactly as levels L-r..1 act on a w x h x d unit.
 * Property (finite data): every output cell differs from the mean of its
 * 2^r-cube of the full reconstruction by at most 3*r * 2^-23 * max|full
 * reconstruction| (one rounding of at most 2^-24 of a block mean per synthesis
 * step, 3 axis steps per level, r levels, a factor 2 of margin).
 *
 *   wc_coarse_units: host-only; out[u] = units[u] with dims >> reduce[u], cell
 *     offsets packed back to back, each start rounded up to 4 elements; *extent
 *     = elements the output needs.  WC_ERR_INVALID for null pointers, negative
 *     dims or a reduce outside 0..WC_MAX_LEVELS.
 *   wc_inverse_coarse: units describe the payloads at full size (their
 *     cell_offset is ignored); levels (HOST, NULL = all 1) and reduce (HOST)
 *     are consumed before the call returns.  out_units[u] must carry exactly the
 *     dims >> reduce[u]; its cell_offset is the caller's choice (any element
 *     alignment; d_out itself 16-byte aligned).  A unit without cells keeps its
 *     shifted dims and writes nothing.  For a unit with r >= 1 nothing of size
 *     W*H*D is written or read: the pairs go straight to the compact corner in
 *     context scratch, and pair tiles past the corner's end leave at once.  A
 *     batch whose reduces are all 0 is wc_inverse_levels (wc_inverse when the
 *     levels are all 1 too) on out_units.  Asynchronous; malformed payloads as
 *     in wc_inverse_levels: a header that disagrees with (W, H, D, L) raises
 *     WC_ERR_FORMAT at the next wc_synchronize, nothing past it is read and the
 *     unit's output cells stay untouched while the other units decode; a
 *     negative run raises the same error and writes nothing outside the unit's
 *     own corner scratch and output range.
 *   wc_inverse_coarse_host: host buffers; levels = NULL reads each L from its
 *     header, as wc_inverse_levels_host does; the unit runs go one after another.
 * A reduce outside 0..levels[u], a dimension that 2^r does not divide on a unit
 * with cells, an out_units entry with other dims or reserved != 0, or a null
 * buffer: WC_ERR_INVALID naming the unit, before anything is launched; outputs
 * stay untouched. */
int wc_coarse_units(const wc_unit* units, const int32_t* reduce, int n, wc_unit* out, uint64_t* extent);
int wc_inverse_coarse(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* d_out);
int wc_inverse_coarse_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* out);

/* Opt-in sub-box decode (not in the reference): the cells of a region of a box
 * straight from its payload, reading only the coefficients the region depends
 * on.  The transform is Haar on every level: a synthesis step writes cells 2m
 * and 2m + 1 of a line from the low and the high coefficient m of that line and
 * from nothing else, so a region aligned to 2^L depends on a small, exactly
 * known subset of the coefficient array, and decoding that subset alone gives
 * the bits of the full decode's crop.  It composes with the reduced-resolution
 * decode: a region at 1/2^r resolution.
 *
 * Definition.  A unit W x H x D has L levels (its payload as wc_forward_levels
 * writes it), a reduction r, 0 <= r <= L, and a region R in full-resolution
 * cells.  For a unit with cells: 2^L divides W, H and D (for L = 1: even
 * dimensions); 2^L divides every origin and extent of R; 0 <= x0 and x0 + nx <=
 * W, likewise for y and z.  A region with a zero extent writes nothing.  A unit
 * without cells needs an all-zero region.
 * Result: a Box3D of (nx, ny, nz) >> r cells (w, h, d) with
 *   out[x + w*(y + h*z)] = F_r((x0 >> r) + x, (y0 >> r) + y, (z0 >> r) + z),
 * F_r being what wc_inverse_coarse gives at reduction r (F_0: wc_inverse_levels,
 * or wc_inverse at L = 1), bit for bit.
 * How: nothing of size W*H*D is written or read.  Write (W', H', D') =
 * (W, H, D) >> r, L' = L - r, o = (x0, y0, z0) >> r, s = (nx, ny, nz) >> r.
 * For the pair at flat position p < W*H*D, (I, J, K) from p = (I*H + J)*D + K:
 *   1. Drop the pair unless I < W', J < H' and K < D' (the corner filter of the
 *      reduced-resolution decode).
 *   2. lvl = 0 if L' = 0; otherwise lvl = j* + 1, j* the largest j in 0..L'-1
 *      with I < W' >> j, J < H' >> j and K < D' >> j.
 *   3. Per axis, with n the axis' primed dimension, c its coordinate, o and s
 *      its origin and extent: if lvl >= 1 and c >= n >> lvl (high band),
 *      q = c - (n >> lvl) - (o >> lvl) and i = q + (s >> lvl); otherwise
 *      q = c - (o >> lvl) and i = q.  Keep the pair iff 0 <= q < s >> lvl on all
 *      three axes.
 *   4. Store the value at C[(i_x*s_y + i_y)*s_z + i_z] of a zeroed compact array.
 * C is the flat array of an s_x x s_y x s_z unit with L' levels: for L' >= 1
 * the result is its multi-level inverse, for L' = 0 C read as a Box3D.  No kept
 * pair sits at or past `end`, one past the flat position of the largest needed
 * (I, J, K); per axis that coordinate is (n >> 1) + (o >> 1) + (s >> 1) - 1 for
 * L' >= 1 and o + s - 1 for L' = 0.  Pair tiles past `end` leave at once.
 * Equalities: R = the whole box gives wc_inverse_coarse bit for bit (with r = 0
 * wc_inverse_levels); any R gives the crop of those.
 *
 *   wc_region_align: host-only; *aligned = the smallest region aligned to
 *     2^levels that contains *want inside the box nx x ny x nz (an axis of zero
 *     extent stays empty, at its origin rounded down).  WC_ERR_INVALID for null
 *     pointers, a region not inside the box, levels outside 1..WC_MAX_LEVELS or
 *     a box with cells whose dimensions 2^levels does not divide.
 *   wc_region_units: host-only; out[u] carries regions[u]'s extents >>
 *     reduce[u] (reduce NULL = all 0), packed as wc_coarse_units packs.  `units`
 *     is not read beyond the null check.  WC_ERR_INVALID for null pointers,
 *     negative extents or a reduce outside 0..WC_MAX_LEVELS.
 *   wc_inverse_region: units describe the payloads at full size (cell_offset
 *     ignored); levels (NULL = all 1), reduce (NULL = all 0) and regions are on
 *     the HOST and consumed before the call returns.  out_units[u] must carry
 *     exactly the extents >> reduce[u]; its cell_offset is the caller's choice
 *     (any element alignment; d_out itself 16-byte aligned).  Asynchronous;
 *     malformed payloads as in wc_inverse_coarse: a header that disagrees raises
 *     WC_ERR_FORMAT at the next wc_synchronize, the unit's output cells stay
 *     untouched and the other units decode; a negative run raises the same error
 *     and writes nothing outside the unit's own scratch and output range.  A
 *     unit whose region has no cells reads nothing, its header included.
 *   wc_inverse_region_host: host buffers; levels = NULL reads each L from its
 *     header; the unit runs go one after another; only the regions' cells cross
 *     back.
 * A reduce outside 0..levels[u], a region that is not inside the box or not
 * aligned to 2^L, a dimension 2^L does not divide, an out_units entry with other
 * dims or reserved != 0, or a null buffer: WC_ERR_INVALID naming the unit,
 * before anything is launched; outputs stay untouched. */
typedef struct wc_region { int32_t x0, y0, z0, nx, ny, nz; } wc_region;  /* full-resolution cells */
int wc_region_align(int32_t nx, int32_t ny, int32_t nz, int levels, const wc_region* want, wc_region* aligned);
int wc_region_units(const wc_unit* units, const wc_region* regions, const int32_t* reduce, int n, wc_unit* out,
                    uint64_t* extent);
int wc_inverse_region(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_region* regions, const wc_unit* out_units,
                      float* d_out);
int wc_inverse_region_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n,
                           const int32_t* levels, const int32_t* reduce, const wc_region* regions,
                           const wc_unit* out_units, float* out);

/* Opt-in packed payloads (NOT a reference format): a smaller way to STORE a
 * payload's kept coefficients.  A standard payload spends 8 bytes per pair, an
 * int32 run and an fp32 value; a packed unit stores each chunk of 64 pairs as
 * bit planes of the runs at the chunk's own width and as the top 2, 3 or 4 bytes
 * of the values in byte planes.  wc_unpack restores standard payloads, which
 * every decoder reads unchanged; wc_inverse_packed, wc_inverse_packed_coarse and
 * wc_inverse_packed_region (below) decode packed units directly.  Every other
 * entry point rejects a packed unit (WC_ERR_FORMAT), its ncoeff field being
 * neither W*H*D nor -2..-4.
 *
 * Format of one unit (integers little-endian).  V = value bytes, 2..4; L = the
 * source payload's levels, 1..WC_MAX_LEVELS; n = its nrle; nch = ceil(n / 64);
 * m_c = the pairs of chunk c, 64 for every chunk but the last, n - 64 (nch - 1)
 * for the last; pad8 rounds up to a multiple of 8.
 *   1. Header, 20 bytes: int32 W, H, D, tag, n with tag = -(16 V + L), -33..-68.
 *   2. Width table, nch bytes: w_c = bit_length(OR of the chunk's runs), 0..31;
 *      zero-padded to pad8(nch) bytes (readers ignore the pad).
 *   3. The chunks in order, each a run area and a value area.  Run area: w_c
 *      planes of ceil(m_c / 8) bytes; bit j % 8 of byte j / 8 of plane b is bit b
 *      of run j, unused bits 0 (a full chunk's plane is a wave64 ballot).  Value
 *      area: V planes of m_c bytes; byte j of plane p is byte 3 - p of the uint32
 *      q(value j): plane 0 is the sign-and-exponent byte.
 *   4. A unit starts at an offset == 4 (mod 8), as payload slots do; every full
 *      chunk then starts 8-byte aligned.
 *   5. The packed length, 20 + pad8(nch) + sum_c (w_c ceil(m_c / 8) + V m_c),
 *      follows from the header and the table alone (wc_packed_size).
 * Value rule q (integers only: host, device and numpy give the same bits).
 * s = 8 (4 - V); b = the value's bits, m = b & 0x7FFFFFFF, sign = b & 0x80000000.
 *   V = 4: q = b.  NaN (m > 0x7F800000): q = (b | 0x00400000) with the low s
 *   bits cleared (still a NaN).  inf: unchanged.  Otherwise r = (m + (1 << (s-1))
 *   - 1 + ((m >> s) & 1)) with the low s bits cleared: round to nearest even, a
 *   carry into the exponent wanted; if r >= 0x7F800000, r = m with the low s bits
 *   cleared (a finite value stays finite); q = sign | r.  A subnormal may round
 *   to +-0; the pair stays, with value +-0.  q(q(x)) = q(x).
 * Error: the level-l basis vectors are orthogonal with squared norm 8^l and
 * |q(v) - v| <= 2^(s-24) |v|, so for finite values
 *   || decode(q(p)) - decode(p) ||_2 <= 2^(s-24) || decode(p) ||_2
 * up to the decoder's own fp32 rounding: 2^-8 of the box's norm at V = 2, 2^-16 at
 * V = 3, nothing at V = 4.
 * Slots: the worst-case packed unit of N cells is S(N) = 20 + pad8(ceil(N / 64))
 * + 31 ceil(N / 8) + V N; unit u's slot is the prefix of pad8(S(N) + 4) of the
 * units before it, starting at 4 (the forward's scheme); wc_packed_bound gives
 * the capacity.
 *
 * Host-only rule (plain C++, no device):
 *   wc_pack_value: q.  vbytes outside 2..4: the bits unchanged.
 *   wc_packed_tag: the tag; 0 for levels or vbytes out of range.
 *   wc_payload_packed: *levels and *vbytes of a 20-byte header; *vbytes = 0 for a
 *     standard or multi-level header (then as wc_payload_levels).  WC_ERR_FORMAT
 *     for any other header.
 *   wc_packed_size: *bytes = the length of the packed unit at `unit`, of which
 *     `avail` bytes may be read: WC_ERR_INVALID if that is less than the header
 *     and the padded table; WC_ERR_FORMAT for a header that is not a packed one,
 *     n above the cell count or a width above 31.
 *   wc_pack_unit / wc_unpack_unit: one unit between the two forms.  WC_ERR_FORMAT
 *     for what the device calls refuse (below); WC_ERR_INVALID for null or short
 *     buffers or vbytes outside 2..4; nothing is written then.
 * Device calls, asynchronous on the context's stream, nothing read back:
 *   wc_pack: standard payloads at d_payload + d_offsets[u] (any multiple of 4;
 *     the layout of wc_forward or of the _host forms) -> packed units in their
 *     slots.  d_packed_offsets: n + 1 uint64, unit u's slot and, at n, the end of
 *     the last unit's bytes; d_packed_bytes: n uint64, each unit's exact length
 *     (0 for a refused unit).  packed_capacity >= wc_packed_bound.  Nothing is
 *     written outside a unit's exact length.
 *   wc_unpack: packed units at d_packed + d_packed_offsets[u] (each == 4 mod 8;
 *     slots or the dense layout of wc_pack_host) -> standard payloads in the
 *     forward's slot layout (payload_capacity >= wc_payload_bound; d_offsets n + 1,
 *     d_kept n, as wc_forward writes them).  Values are q(v), runs unchanged, the
 *     header's ncoeff is W*H*D again, or -L for L >= 2.  At V = 4 the payload is
 *     byte for byte the source.  Nothing at or past packed_capacity is read.
 *   Both take units of at most WC_PACK_MAX_CELLS cells: a workgroup finds its
 *   place by summing the width table before it, which no workgroup has to wait
 *   for but costs n^2 / 2^18 table bytes on a unit of n pairs.
 * Refusals.  On the device (WC_ERR_FORMAT at the next wc_synchronize; the other
 * units of the call are transcoded, nothing is written outside the refused
 * unit's slot): in wc_pack a source header that is not a standard or multi-level
 * header of its unit, nrle above the cell count, a negative run; in wc_unpack an
 * offset that is not 4 (mod 8), a header or tag that is not a packed one of its
 * unit, n above the cell count, a width above 31, a unit whose length from
 * header and table would pass packed_capacity.  Before anything is launched
 * (WC_ERR_INVALID, outputs untouched): null buffers, a capacity below its bound,
 * vbytes outside 2..4, a unit above WC_PACK_MAX_CELLS cells.
 *   wc_pack_host / wc_unpack_host: host buffers; one upload, the device call, the
 *     slots packed densely on the device as wc_forward_host does, one download.
 *     They are NOT pipelined over WC_OPT_HOST_CHUNK runs, and they cost one more
 *     crossing of the payload bytes than a forward that packed before its
 *     download would.  wc_pack_host: packed_offsets (n + 1; each == 4 mod 8,
 *     unit u + 1 at pad8 of unit u's length after unit u; [n] = the end of the
 *     last unit's bytes) and packed_bytes (n); packed_capacity >= packed_offsets[n],
 *     at most wc_packed_bound.  wc_unpack_host: payload, offsets and kept as
 *     wc_forward_host returns them.  A refused unit fails the call
 *     (WC_ERR_FORMAT) and leaves the outputs untouched. */
#define WC_PACK_MAX_CELLS (1 << 21)
uint32_t wc_pack_value(uint32_t bits, int vbytes);
int32_t wc_packed_tag(int levels, int vbytes);
int wc_payload_packed(const uint8_t* header, size_t len, int* levels, int* vbytes);
int wc_packed_size(const uint8_t* unit, size_t avail, uint64_t* bytes);
int wc_pack_unit(const uint8_t* payload, size_t len, int vbytes, uint8_t* out, size_t cap, size_t* written);
int wc_unpack_unit(const uint8_t* packed, size_t len, uint8_t* out, size_t cap, size_t* written);
int wc_packed_bound(const wc_unit* units, int n, int vbytes, uint64_t* bytes);
int wc_pack(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n, int vbytes,
            uint8_t* d_packed, uint64_t packed_capacity, uint64_t* d_packed_offsets, uint64_t* d_packed_bytes);
int wc_unpack(wc_ctx* ctx, const uint8_t* d_packed, const uint64_t* d_packed_offsets, uint64_t packed_capacity,
              const wc_unit* units, int n, uint8_t* d_payload, uint64_t payload_capacity, uint64_t* d_offsets,
              uint32_t* d_kept);
int wc_pack_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets, const wc_unit* units, int n, int vbytes,
                 uint8_t* packed, uint64_t packed_capacity, uint64_t* packed_offsets, uint64_t* packed_bytes);
int wc_unpack_host(wc_ctx* ctx, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units, int n,
                   uint8_t* payload, uint64_t payload_capacity, uint64_t* offsets, uint32_t* kept);

/* Decoding packed units directly: the dense decode (wc_inverse_levels), the
 * reduced-resolution decode (wc_inverse_coarse) and the sub-box decode
 * (wc_inverse_region) with packed units as their source.  Each call gives, bit
 * for bit (NaN payload bits included), what wc_unpack followed by its standard
 * twin gives on the same units: the same kernels run the same scan, scatter and
 * synthesis, and only the load of a tile's pairs differs (a decode tile is 64
 * chunks; a workgroup places its chunks from the width table as wc_unpack does).
 * No standard payload is written and nothing is sized by wc_payload_bound; the
 * coarse and the sub-box decode keep their "only the pair tiles before `end`"
 * property, and read of those tiles only the table, the planes and the values.
 *   wc_inverse_packed: EVERY unit of the call is a packed unit at d_packed +
 *     d_packed_offsets[u] (each == 4 mod 8; the slots of wc_pack or the dense
 *     layout of wc_pack_host; d_packed 8-byte aligned); a mixed batch is the
 *     caller's to split.  levels (HOST, consumed before return; NULL = all 1) as
 *     in wc_inverse_levels.  Every unit decodes densely, for every L, L = 1 units
 *     of any dimensions included (the row-indexed inverse reads pairs at random
 *     from a standard payload and has no packed form).  Books WC_STAGE_DECODE,
 *     WC_STAGE_LEVELS and WC_STAGE_INVERSE like wc_inverse_levels.
 *   wc_inverse_packed_coarse / wc_inverse_packed_region: levels, reduce, regions
 *     and out_units exactly as in wc_inverse_coarse / wc_inverse_region.
 *   Nothing at or past packed_capacity is read.  Refusals on the device
 *   (WC_ERR_FORMAT at the next wc_synchronize; the other units decode): an offset
 *   that is not 4 (mod 8), a header that is not a packed one of its unit with the
 *   expected L, n above the cell count, a table whose end would pass the capacity:
 *   the unit's output cells stay untouched, as in the standard decoders; a width
 *   above 31 or a chunk whose end would pass the capacity: the unit's cells are
 *   unspecified, and nothing is written outside the unit's own scratch and output
 *   range.  A packed run has at most 31 bits, so no negative run can arise.  A
 *   unit whose region has no cells reads nothing, its header included.  Before
 *   anything is launched (WC_ERR_INVALID, outputs untouched): what the standard
 *   twin refuses, null buffers, a unit above WC_PACK_MAX_CELLS cells.
 *   _host forms: host buffers; levels = NULL reads each L from its unit's tag;
 *     the packed bytes are uploaded (not standard payloads), the unit runs
 *     (WC_OPT_HOST_CHUNK) go one after another, only the result cells cross back.
 *     Every unit is checked on the host first (wc_packed_size): a unit the device
 *     would refuse fails the call (WC_ERR_FORMAT) and leaves the outputs untouched.
 * Measured at C2 (profiles/r17/packed_decode.json, DESIGN.md "Packed decode"). */
int wc_inverse_packed(wc_ctx* ctx, const uint8_t* d_packed, const uint64_t* d_packed_offsets, uint64_t packed_capacity,
                      const wc_unit* units, int n, const int32_t* levels, float* d_out);
int wc_inverse_packed_coarse(wc_ctx* ctx, const uint8_t* d_packed, const uint64_t* d_packed_offsets,
                             uint64_t packed_capacity, const wc_unit* units, int n, const int32_t* levels,
                             const int32_t* reduce, const wc_unit* out_units, float* d_out);
int wc_inverse_packed_region(wc_ctx* ctx, const uint8_t* d_packed, const uint64_t* d_packed_offsets,
                             uint64_t packed_capacity, const wc_unit* units, int n, const int32_t* levels,
                             const int32_t* reduce, const wc_region* regions, const wc_unit* out_units, float* d_out);
int wc_inverse_packed_host(wc_ctx* ctx, const uint8_t* packed, const uint64_t* packed_offsets, const wc_unit* units,
                           int n, const int32_t* levels, float* out);
int wc_inverse_packed_coarse_host(wc_ctx* ctx, const uint8_t* packed, const uint64_t* packed_offsets,
                                  const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                                  const wc_unit* out_units, float* out);
int wc_inverse_packed_region_host(wc_ctx* ctx, const uint8_t* packed, const uint64_t* packed_offsets,
                                  const wc_unit* units, int n, const int32_t* levels, const int32_t* reduce,
                                  const wc_region* regions, const wc_unit* out_units, float* out);

/* Transform only: cells -> flat fp32 coefficients (x-slowest order), written
 * at the same element offsets as the cells (d_flat has the cell buffer's extent). */
int wc_decompose(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n,
                 float* d_flat);

/* Inverse path for a batch: payloads -> fp32 Box3D cells at units[u].cell_offset.
 * Asynchronous on the context's stream.  Each payload header must match its unit
 * (W,H,D, ncoeff) and no run may be negative, else the next wc_synchronize (or the
 * _host variant itself) returns WC_ERR_FORMAT (the reference exits,
 * src/decompressor.cpp:228-231). */
int wc_inverse(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets,
               const wc_unit* units, int n, float* d_out);

int wc_inverse_host(wc_ctx* ctx, const uint8_t* payload, const uint64_t* offsets,
                    const wc_unit* units, int n, float* out);

/* Inverse transform only: flat coefficients -> fp32 Box3D cells. */
int wc_inverse_flat(wc_ctx* ctx, const float* d_flat, const wc_unit* units, int n, float* d_out);
int wc_inverse_flat_host(wc_ctx* ctx, const float* flat, const wc_unit* units, int n, float* out);

/* Per-unit RMSE between original cells (fp64 narrowed, or fp32) and fp32
 * reconstructions; d_rmse: n doubles (device).  d_orig and d_regen at any
 * element alignment (vector loads where both bases allow them). */
int wc_rmse(wc_ctx* ctx, const void* d_orig, int dtype, const float* d_regen,
            const wc_unit* units, int n, double* d_rmse);
int wc_rmse_host(wc_ctx* ctx, const void* orig, int dtype, const float* regen,
                 const wc_unit* units, int n, double* rmse);

/* wc_inverse then wc_rmse of the reconstruction against d_orig, fused: the
 * row-indexed inverse adds each tile's squared differences right after
 * writing it (the reconstruction is not re-read from HBM).  Same d_out; RMSE
 * equal to wc_rmse's up to the order of the double sum (a batch with a unit
 * on the dense decode path runs the two calls).  Replaces the decompress ->
 * calc_rmse_per_box pair of the reference's -estimate / round-trip
 * (src/modes.cpp:209-327, src/calc-loss.cpp:12-43). */
int wc_inverse_rmse(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets,
                    const wc_unit* units, int n, const void* d_orig, int dtype, float* d_out,
                    double* d_rmse);

/* Round trips in one process (the reference's -estimate: compress, then
 * decompress the same boxes and calc_rmse_per_box, src/modes.cpp:236-291).
 * The forward knows, as it packs the pairs, where every flat row of a unit
 * starts in the payload; wc_forward_rows writes that ROW INDEX beside the
 * payloads, and wc_inverse_rows reads it instead of re-deriving it from the
 * payloads (the row index kernel of wc_inverse, a third of its time).
 *
 *   Row index layout (caller-owned device buffer, wc_rowindex_bytes): unit u
 *   owns W*H + 1 entries of 8 bytes (none when it has no cells), after the
 *   entries of units 0..u-1.  Entry
 *   r < W*H of flat row r = I*H + J (the D coefficients r*D .. r*D + D - 1 of
 *   the reference's flat order, src/compressor.cpp:178-181) is {uint32 k,
 *   uint32 p_k - r*D}: k the first pair whose flat position p_k is >= r*D;
 *   entry W*H and the rows after the last pair hold {nrle, ncoeff - r*D}.
 *   Written for the units of the row-indexed shape (W and H even, D % 8 ==
 *   0, cells > 0); the entries of other units are not written (their inverse
 *   decodes from the payload).
 *
 *   wc_forward_rows: wc_forward (same payloads, offsets, kept counts) that
 *     also writes the row index (rowinfo_capacity >= wc_rowindex_bytes).
 *   wc_inverse_rows: wc_inverse (d_orig = d_rmse = NULL) or wc_inverse_rmse
 *     (both set) of payloads whose row index d_rowinfo came from
 *     wc_forward_rows of the same payloads and units (NULL: derived from the
 *     payloads, = wc_inverse / wc_inverse_rmse; rowinfo_capacity is then
 *     ignored, else it must be >= wc_rowindex_bytes).  Pair indices read from
 *     the row index are clamped to each payload's pair count, so a row index
 *     that belongs to other payloads gives wrong cells but never an access
 *     outside the payloads; headers are checked against the units
 *     (WC_ERR_FORMAT at the next wc_synchronize). */
uint64_t wc_rowindex_bytes(const wc_unit* units, int n);
int wc_forward_rows(wc_ctx* ctx, const void* d_cells, int dtype, const wc_unit* units, int n, double keep,
                    uint8_t* d_payload, uint64_t payload_capacity, uint64_t* d_offsets, uint32_t* d_kept,
                    void* d_rowinfo, uint64_t rowinfo_capacity);
int wc_inverse_rows(wc_ctx* ctx, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const void* d_rowinfo, uint64_t rowinfo_capacity, const void* d_orig, int dtype, float* d_out,
                    double* d_rmse);

/* Transform only, host pointers (the reference's static wavelet_decompose). */
int wc_decompose_host(wc_ctx* ctx, const void* cells, int dtype, const wc_unit* units, int n,
                      float* flat);

/* Per-kernel timing with hipEvents recorded on the context stream around each
 * launch (used by bench.py for the live roofline figure).  Stage ids below;
 * wc_profile_read() returns the summed milliseconds and launch counts since
 * the previous read, then resets. */
#define WC_STAGE_TRANSFORM 0  /* K1  transform (+ dense re-staging fallback) */
#define WC_STAGE_EMIT 1       /* K2  threshold + ordered pack (k_emit) */
#define WC_STAGE_DECODE 2     /* K5  rle_decode */
#define WC_STAGE_INVERSE 3    /* K6  inverse transform */
#define WC_STAGE_RMSE 4       /* K7; also wc_maxerr */
#define WC_STAGE_HIST 5       /* histogram pass of generic units (wc_forward_stage with d_hist; the fast
                                 units' bins are counted inside the transform stage) */
#define WC_STAGE_PAIRS 6      /* header check + pair counts of wc_inverse_rows with a caller row index */
#define WC_STAGE_TOL 7        /* per-unit bins + threshold pick of the RMSE-tolerance mode (wc_forward_tol); per-level bins, pick
                                 and mask pass of wc_forward_levels_tol; radix select and mask pass of
                                 wc_forward_levels_budget; probe passes, pick and mask pass of
                                 wc_forward_levels_maxerr; every pass of wc_thin_budget / wc_thin_thresh, of
                                 wc_split_budget / wc_split_thresh and of wc_merge */
#define WC_STAGE_LEVELS 8    /* level passes, key pass and header patch of the multi-level mode (wc_forward_levels,
                                 wc_inverse_levels) */
#define WC_STAGE_PACK 9      /* packed payloads: k_pack_widths + k_pack_body (wc_pack), k_unpack (wc_unpack) */
#define WC_NUM_STAGES 10
int wc_profile_enable(wc_ctx* ctx, int on);
int wc_profile_read(wc_ctx* ctx, double* total_ms, uint32_t* launches, int nstages);

/* Version string of the library build (arch, flags). */
const char* wc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WAVELET_AMD_H */
