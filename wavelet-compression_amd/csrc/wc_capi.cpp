// wc_capi.cpp — the extern "C" boundary (include/wavelet_amd.h): context
// lifetime, options and the device-pointer entry points.
//
// The context (wc_ctx.h) owns the stream, grow-only scratch in HBM and the
// cached batch plans (wc_plan.cpp), and turns a batch of units into kernel
// launches.  No CPU fallback exists: every computing entry point launches HIP
// kernels and fails with WC_ERR_HIP if the device or code object is absent.
// The _host entry points are in wc_hostpipe.cpp; those of the opt-in modes are
// calls of the two serial drivers of wc_hostserial.cpp (wc_forward_tol_host and
// the host-only wc_tol_threshold: wc_tolhost.cpp; wc_forward_levels_tol_host:
// wc_leveltolhost.cpp; the host-only wc_tol_levels_threshold: wc_leveltolrule.cpp;
// wc_forward_levels_budget_host: wc_budgethost.cpp; the host-only wc_budget_select
// and wc_budget_thresholds: wc_budgetrule.cpp; wc_forward_levels_maxerr_host and
// wc_maxerr_host: wc_maxerrhost.cpp; the host-only wc_maxerr_select: wc_maxerrrule.cpp; wc_pack, wc_unpack and their _host
// forms: wc_packhost.cpp; the packed format's host-only rule: wc_packrule.cpp;
// the packed decoders' _host forms: wc_packdecodehost.cpp;
// wc_forward_levels_host and wc_inverse_levels_host: wc_levelshost.cpp; the
// host-only wc_levels_for and wc_payload_levels: wc_levelsrule.cpp;
// wc_inverse_coarse_host and wc_coarse_units: wc_coarsehost.cpp;
// wc_inverse_region_host and the checks it shares with wc_inverse_coarse_host:
// wc_regionhost.cpp; wc_region_align and wc_region_units: wc_regionrule.cpp;
// wc_thin_budget_host and wc_thin_thresh_host: wc_thinhost.cpp).
//
// Forward path per batch (wc_forward), every unit shape: K1 k_transform{,_fast}
// -> flat coefficients in HBM scratch (sparse staging: only the flagged
// segments) + per-unit max keys -> k_transform_fallback (units whose thresh
// is < 0 re-staged densely) -> K2 k_emit (threshold + decoupled look-back +
// ordered pack), writing unit u's serialized bytes at its fixed slot
// offsets[u] (and with wc_forward_rows the payloads' row index).  Inverse:
// K5 k_rowindex (or the caller's row index) -> K6r k_inverse_rows from the
// payloads; units that are not row-indexable: k_decode -> dense flat scratch
// -> K6 k_inverse{,_fast}.
#include "wc_ctx.h"
#include "wc_regionmap.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace wc;

namespace {

// While one lives, get_plan builds dense plans (WC_OPT_INVERSE_ROWS = 0: every unit's pair tiles in
// dtiles).  The plan's key holds the option, so such a plan is cached beside the batch's default one.
struct DensePlans {
    wc_ctx* c;
    bool rows;
    explicit DensePlans(wc_ctx* c_) : c(c_), rows(c_->opt_inv_rows) { c->opt_inv_rows = false; }
    ~DensePlans() { c->opt_inv_rows = rows; }
};
// The dense plan of these units; strip_offsets: without their cell offsets (the passes over payloads
// ignore them, so the key carries none).
int dense_plan(wc_ctx* c, const wc_unit* units, int n, bool strip_offsets) {
    DensePlans dense(c);
    if (!strip_offsets) return get_plan(c, units, n);
    std::vector<wc_unit> full(units, units + n);
    for (wc_unit& u : full) u.cell_offset = 0;
    return get_plan(c, full.data(), n);
}

// Staged forward, first half: K1 transform into the flat coefficient
// scratch + per-unit max keys (zeroed state).
int stage_transform(wc_ctx* c, const void* d_cells, int dtype, double keep, bool sparse) {
    Plan& P = c->plan;
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const XTile* dxt = (const XTile*)P.d_xtiles.p;
    hipError_t e = hipSuccess;
    if ((e = hipMemsetAsync(c->state.p, 0, P.state_bytes, c->stream)) != hipSuccess)
        return hip_fail(c, e, "memset state");
    unsigned long long* key = (unsigned long long*)((uint8_t*)c->state.p + 16);
    const size_t n = P.units.size();
    uint32_t* spos = (uint32_t*)((uint8_t*)c->state.p + 16 + 12 * n);
    float* coef = (float*)c->coef.p;
    uint8_t* flags = sparse && P.any_sparse ? (uint8_t*)c->flags.p : nullptr;
    {
        StageTimer t(c, WC_STAGE_TRANSFORM);
        e = launch_transform(c->stream, d_cells, dtype, du, dxt, P.ngen, P.lds_gen, coef, 0, key);
        if (e == hipSuccess)
            e = launch_transform_fast(c->stream, d_cells, dtype, du, dxt + P.ngen, P.nfast, P.lds_fast, coef, 0,
                                      key, flags, spos, keep, persistent_grid(c, 0, P.lds_fast));
        // units whose thresh came out < 0 need every coefficient (rare: negative signed max)
        if (e == hipSuccess && flags)
            e = launch_transform_fallback(c->stream, d_cells, dtype, du, (int)P.units.size(), dxt, P.lds_fast, coef,
                                          key, spos, keep);
    }
    c->sparse_staged = flags != nullptr;
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "transform launch");
}

// Second half: K2 threshold + ordered pack of the staged coefficients
// (gthresh: the global-threshold mode's fp32 threshold, or null).  Uses the
// unit keys and the zeroed tickets / look-back granules of the per-call state.
int stage_emit(wc_ctx* c, int n, double keep, const float* gthresh, uint8_t* d_payload, uint64_t* d_offsets,
               uint32_t* d_kept, uint2* d_rows = nullptr, const float* d_uthresh = nullptr) {
    Plan& P = c->plan;
    uint8_t* st = (uint8_t*)c->state.p;
    EmitParams p{};
    p.units = (const UnitDev*)P.d_units.p;
    p.edesc = (const EmitDesc*)P.d_edesc.p;
    p.n = n;
    p.ordered = (uint32_t)tile_order(c);
    p.key = (const unsigned long long*)(st + 16);
    p.tickets = (uint32_t*)(st + 16 + 8ull * n);
    p.status = (unsigned long long*)(st + round_up(16 + 20ull * n, 8));
    p.payload = d_payload;
    p.offsets = d_offsets;
    p.kept = d_kept;
    p.err = (uint32_t*)c->errflag.p;
    p.keep = keep;
    if (gthresh) {
        p.use_gthresh = 1;
        p.gthresh = *gthresh;
    }
    p.flags = (c->sparse_staged && !gthresh && !d_uthresh) ? (const uint8_t*)c->flags.p : nullptr;
    p.rowinfo = d_rows;
    p.uthresh = d_uthresh;
    StageTimer t(c, WC_STAGE_EMIT);
    hipError_t e = launch_emit(c->stream, p, (const float*)c->coef.p, P.nedesc_small,
                               (uint32_t)P.edesc.size() - P.nedesc_small);
    if (e != hipSuccess) return hip_fail(c, e, "emit launch");
    return WC_OK;
}

int forward_staged(wc_ctx* c, const void* d_cells, int dtype, int n, double keep, uint8_t* d_payload,
                   uint64_t* d_offsets, uint32_t* d_kept, uint2* d_rows = nullptr) {
    int rc = stage_transform(c, d_cells, dtype, keep, c->opt_sparse);
    return rc ? rc : stage_emit(c, n, keep, nullptr, d_payload, d_offsets, d_kept, d_rows);
}

// A call's small host arrays (tolerances, levels, work lists) reach the device
// through the context's pinned block, so the caller's arrays are consumed before
// the call returns.  pin_begin: the block, at least in_bytes long and no longer
// read by the previous call's copy, and tol_in of dev_bytes; pin_upload: the
// block's first in_bytes to tol_in on the stream.
int pin_begin(wc_ctx* c, size_t in_bytes, size_t dev_bytes, uint8_t** pin) {
    int rc;
    hipError_t e;
    if ((rc = ensure(c, c->tol_in, dev_bytes))) return rc;
    if (!c->tol_ev && (e = hipEventCreateWithFlags(&c->tol_ev, hipEventDisableTiming)) != hipSuccess)
        return hip_fail(c, e, "event");
    // the previous call's copy out of the pinned block has finished
    if (c->tol_ev_live && (e = hipEventSynchronize(c->tol_ev)) != hipSuccess) return hip_fail(c, e, "pinned upload");
    c->tol_ev_live = false;
    if (c->tol_pin_bytes < in_bytes) {
        if (c->tol_pin) (void)hipHostFree(c->tol_pin);
        c->tol_pin = nullptr;
        c->tol_pin_bytes = 0;
        const size_t want = std::max(in_bytes, size_t(4096));
        if ((e = hipHostMalloc(&c->tol_pin, want, hipHostMallocDefault)) != hipSuccess) {
            c->tol_pin = nullptr;
            return fail(c, WC_ERR_NOMEM, std::string("pinned block: ") + hipGetErrorString(e));
        }
        c->tol_pin_bytes = want;
    }
    *pin = (uint8_t*)c->tol_pin;
    return WC_OK;
}

int pin_upload(wc_ctx* c, size_t in_bytes) {
    hipError_t e;
    if ((e = hipMemcpyAsync(c->tol_in.p, c->tol_pin, in_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipEventRecord(c->tol_ev, c->stream)) != hipSuccess)
        return hip_fail(c, e, "pinned upload");
    c->tol_ev_live = true;
    return WC_OK;
}

// RMSE-tolerance mode, between the dense staging and the emit: unit u's
// threshold (and model bound) from its own magnitude bins (wc_tol.hip).  The
// tolerances and the solo / split layout of this call go through the context's
// pinned block (the caller's array is consumed here).  *uthresh: the device
// thresholds for the emit (d_thresh, or context scratch when that is null).
int stage_tol(wc_ctx* c, int n, const double* tol, float* d_thresh, double* d_bound, const float** uthresh) {
    const Plan& P = c->plan;
    // A unit of more than opt_tol_solo flat tiles is split into runs of `chunk`
    // tiles, one workgroup each.
    const uint32_t solo = (uint32_t)c->opt_tol_solo;
    const uint32_t chunk = std::min<uint32_t>(solo, 8);
    std::vector<uint32_t> slot(n), split;
    std::vector<uint2> items;
    for (int u = 0; u < n; ++u) {
        const uint32_t nt = P.units[u].nftiles;
        if (nt <= solo) {
            slot[u] = 0xffffffffu;
            continue;
        }
        slot[u] = (uint32_t)split.size();
        split.push_back((uint32_t)u);
        for (uint32_t t = 0; t < nt; t += chunk) items.push_back(make_uint2((uint32_t)u, t));
    }
    const size_t nsplit = split.size(), nitems = items.size();
    // tol[n] | items[nitems] | slot[n] | split_units[nsplit] (8-B members first) | thresh[n]
    const size_t o_items = sizeof(double) * n, o_slot = o_items + sizeof(uint2) * nitems, o_split = o_slot + 4ull * n,
                 in_bytes = o_split + 4 * nsplit, o_thresh = round_up(in_bytes, 8);
    int rc;
    hipError_t e;
    uint8_t* pin = nullptr;
    if ((nsplit && (rc = ensure(c, c->tol_bins, sizeof(uint32_t) * WC_HIST_BINS * nsplit))) ||
        (rc = pin_begin(c, in_bytes, o_thresh + sizeof(float) * n, &pin)))
        return rc;
    std::memcpy(pin, tol, sizeof(double) * n);
    if (nitems) std::memcpy(pin + o_items, items.data(), sizeof(uint2) * nitems);
    std::memcpy(pin + o_slot, slot.data(), 4ull * n);
    if (nsplit) std::memcpy(pin + o_split, split.data(), 4 * nsplit);
    if ((rc = pin_upload(c, in_bytes))) return rc;
    uint8_t* d = (uint8_t*)c->tol_in.p;
    if (nsplit && (e = hipMemsetAsync(c->tol_bins.p, 0, sizeof(uint32_t) * WC_HIST_BINS * nsplit, c->stream)) !=
                      hipSuccess)
        return hip_fail(c, e, "memset bins");
    float* th = d_thresh ? d_thresh : (float*)(d + o_thresh);
    StageTimer t(c, WC_STAGE_TOL);
    e = launch_tol(c->stream, (const UnitDev*)P.d_units.p, n, (const uint32_t*)(d + o_slot),
                   (const uint2*)(d + o_items), (uint32_t)nitems, chunk, (const uint32_t*)(d + o_split),
                   (uint32_t)nsplit, (const float*)c->coef.p, (uint32_t*)c->tol_bins.p, (const double*)d, th, d_bound);
    if (e != hipSuccess) return hip_fail(c, e, "tolerance launch");
    *uthresh = th;
    return WC_OK;
}

// Multi-level mode (wc_levels.hip).  The levels and the work lists of one call,
// on the device (in tol_in, uploaded through the pinned block): the levels are
// not part of the cached plan, which is keyed by the units alone.
struct LevelWork {
    const int32_t* levels = nullptr;  // [n]
    const uint2* hdr = nullptr;       // (unit, L) of the units with L >= 2
    const uint2* key = nullptr;       // (unit, first flat tile) runs of kLevelKeyChunk tiles of those units
    const uint2* lv[WC_MAX_LEVELS - 1] = {};  // level l's (unit, chunk) items at lv[l - 2]
    uint32_t nhdr = 0, nkey = 0, nlv[WC_MAX_LEVELS - 1] = {};
    int maxl = 1;
};
constexpr uint32_t kLevelKeyChunk = 8;  // flat tiles per workgroup of the key pass

// extra: a blob of the caller's that rides along (8-B aligned on the device, *d_extra).
int upload_levels(wc_ctx* c, int n, const int32_t* levels, LevelWork* w, const void* extra = nullptr,
                  size_t extra_bytes = 0, const void** d_extra = nullptr) {
    const Plan& P = c->plan;
    std::vector<uint2> hdr, key, lv[WC_MAX_LEVELS - 1];
    const uint32_t cb = level_chunk_blocks();
    for (int u = 0; u < n; ++u) {
        const int L = levels[u];
        if (L < 2) continue;
        w->maxl = std::max(w->maxl, L);
        hdr.push_back(make_uint2((uint32_t)u, (uint32_t)L));
        const UnitDev& d = P.units[u];
        for (uint32_t t = 0; t < d.nftiles; t += kLevelKeyChunk) key.push_back(make_uint2((uint32_t)u, t));
        for (int l = 2; l <= L; ++l) {
            const uint64_t nblk = d.ncells >> (3 * l);  // 2x2x2 blocks of the level's sub-box
            for (uint64_t b = 0; b < nblk; b += cb) lv[l - 2].push_back(make_uint2((uint32_t)u, (uint32_t)(b / cb)));
        }
    }
    size_t items = hdr.size() + key.size();
    for (const auto& v : lv) items += v.size();
    const size_t o_levels = sizeof(uint2) * items, o_extra = round_up(o_levels + sizeof(int32_t) * n, 8),
                 in_bytes = extra_bytes ? o_extra + extra_bytes : o_levels + sizeof(int32_t) * n;
    int rc;
    uint8_t* pin = nullptr;
    if ((rc = pin_begin(c, in_bytes, in_bytes, &pin))) return rc;
    const uint8_t* d = (const uint8_t*)c->tol_in.p;
    size_t o = 0;
    auto put = [&](const std::vector<uint2>& v, const uint2** dev, uint32_t* count) {
        if (!v.empty()) std::memcpy(pin + o, v.data(), sizeof(uint2) * v.size());
        *dev = (const uint2*)(d + o);
        *count = (uint32_t)v.size();
        o += sizeof(uint2) * v.size();
    };
    put(hdr, &w->hdr, &w->nhdr);
    put(key, &w->key, &w->nkey);
    for (int i = 0; i < WC_MAX_LEVELS - 1; ++i) put(lv[i], &w->lv[i], &w->nlv[i]);
    std::memcpy(pin + o_levels, levels, sizeof(int32_t) * n);
    w->levels = (const int32_t*)(d + o_levels);
    if (extra_bytes) {
        std::memcpy(pin + o_extra, extra, extra_bytes);
        *d_extra = d + o_extra;
    }
    if ((rc = ensure(c, c->lv_side, sizeof(float) * (P.coef_extent / 8 + 64)))) return rc;
    return pin_upload(c, in_bytes);
}

// The level passes on the coefficient scratch: analysis l = 2..L after the
// one-level transform (with_key: then the units' max keys of the final array,
// for the keep rule), or synthesis l = L..2 before the one-level inverse.
// bad (inverse of payloads): per-unit words the decode set for a header that disagrees.
int run_levels(wc_ctx* c, const LevelWork& w, bool fwd, bool with_key, const uint32_t* bad = nullptr) {
    const UnitDev* du = (const UnitDev*)c->plan.d_units.p;
    float* coef = (float*)c->coef.p;
    float* side = (float*)c->lv_side.p;
    unsigned long long* key = (unsigned long long*)((uint8_t*)c->state.p + 16);
    StageTimer t(c, WC_STAGE_LEVELS);
    hipError_t e = hipSuccess;
    if (fwd) {
        for (int l = 2; l <= w.maxl && e == hipSuccess; ++l)
            e = launch_level(c->stream, true, du, w.lv[l - 2], w.nlv[l - 2], l - 1, coef, side,
                             with_key && l == 2 ? key : nullptr, nullptr);
        if (e == hipSuccess && with_key) e = launch_level_key(c->stream, du, w.key, w.nkey, kLevelKeyChunk, coef, key);
    } else {
        for (int l = w.maxl; l >= 2 && e == hipSuccess; --l)
            e = launch_level(c->stream, false, du, w.lv[l - 2], w.nlv[l - 2], l - 1, coef, side, nullptr, bad);
    }
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "level pass launch");
}

// RMSE tolerance on the multi-level transform (wc_leveltol.hip).  The call's
// per-unit descriptors and its solo / split layout ride along with the level
// work lists (upload_levels' extra blob):
//   LtUnit[n] | items[nitems] | split_units[nsplit] | thresh[n * WC_MAX_LEVELS]
// (8-B members first; the thresholds only when the caller passes no d_thresh).
struct LevelTolWork {
    std::vector<uint8_t> blob;
    size_t o_items = 0, o_split = 0, o_thresh = 0, o_tail = 0;
    uint32_t nitems = 0, nsplit = 0, chunk = 0;
};

// tol NULL: the descriptors' tolerances are 0 (the size-budget mode has none);
// tail: bytes per unit and per split unit that a mode appends at o_tail (8-B aligned, zeroed).
void build_leveltol(const wc_ctx* c, int n, const int32_t* levels, const double* tol, bool own_thresh,
                    LevelTolWork* t, size_t tail_unit = 0, size_t tail_split = 0) {
    const Plan& P = c->plan;
    // as stage_tol: a unit of more than opt_tol_solo flat tiles is split into runs of `chunk` tiles
    const uint32_t solo = (uint32_t)c->opt_tol_solo;
    t->chunk = std::min<uint32_t>(solo, 8);
    std::vector<LtUnit> lt(n);
    std::vector<uint32_t> split;
    std::vector<uint2> items;
    for (int u = 0; u < n; ++u) {
        const UnitDev& d = P.units[u];
        lt[u] = {d.ncells ? rows_magic(d.nz) : 0, d.ncells ? rows_magic(d.ny) : 0, tol ? tol[u] : 0.0,
                 (uint32_t)levels[u], kLtSolo};
        if (d.nftiles <= solo) continue;
        lt[u].slot = (uint32_t)split.size();
        split.push_back((uint32_t)u);
        for (uint32_t f = 0; f < d.nftiles; f += t->chunk) items.push_back(make_uint2((uint32_t)u, f));
    }
    t->nitems = (uint32_t)items.size();
    t->nsplit = (uint32_t)split.size();
    t->o_items = sizeof(LtUnit) * n;
    t->o_split = t->o_items + sizeof(uint2) * items.size();
    t->o_thresh = t->o_split + 4 * split.size();
    t->o_tail = round_up(t->o_thresh + (own_thresh ? sizeof(float) * WC_MAX_LEVELS * n : 0), 8);
    const size_t tail = tail_unit * n + tail_split * split.size();
    t->blob.assign(tail ? t->o_tail + tail : t->o_thresh + (own_thresh ? sizeof(float) * WC_MAX_LEVELS * n : 0), 0);
    std::memcpy(t->blob.data(), lt.data(), sizeof(LtUnit) * n);
    if (!items.empty()) std::memcpy(t->blob.data() + t->o_items, items.data(), sizeof(uint2) * items.size());
    if (!split.empty()) std::memcpy(t->blob.data() + t->o_split, split.data(), 4 * split.size());
}

// Between the level passes and the emit: the per-level bins and the pick of
// every unit, then the mask pass that zeroes what the thresholds drop.
int stage_leveltol(wc_ctx* c, int n, int maxl, const LevelTolWork& t, const uint8_t* d_blob, float* d_thresh,
                   double* d_bound) {
    const Plan& P = c->plan;
    int rc;
    hipError_t e;
    const size_t bin_bytes = sizeof(uint32_t) * WC_HIST_BINS * (size_t)maxl * t.nsplit;
    if (t.nsplit) {
        if ((rc = ensure(c, c->tol_bins, bin_bytes))) return rc;
        if ((e = hipMemsetAsync(c->tol_bins.p, 0, bin_bytes, c->stream)) != hipSuccess)
            return hip_fail(c, e, "memset bins");
    }
    float* th = d_thresh ? d_thresh : (float*)const_cast<uint8_t*>(d_blob + t.o_thresh);
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const LtUnit* lt = (const LtUnit*)d_blob;
    StageTimer timer(c, WC_STAGE_TOL);
    e = launch_leveltol(c->stream, du, n, lt, (const uint2*)(d_blob + t.o_items), t.nitems, t.chunk,
                        (const uint32_t*)(d_blob + t.o_split), t.nsplit, maxl, (const float*)c->coef.p,
                        (uint32_t*)c->tol_bins.p, th, d_bound);
    if (e == hipSuccess)
        e = launch_leveltol_mask(c->stream, du, lt, (const FTile*)P.d_ftiles.p, (uint32_t)P.ftiles.size(),
                                 (float*)c->coef.p, th);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "level tolerance launch");
}

// Size-budget mode, between the level passes and the emit: the radix select of
// every unit (wc_budget.hip), then the mask pass of the tolerance mode with the
// thresholds it found.  The tail of the blob: state[nsplit] | max_pairs[n].
int stage_budget(wc_ctx* c, int n, int maxl, const LevelTolWork& t, const uint8_t* d_blob, float* d_thresh,
                 uint32_t* d_key) {
    const Plan& P = c->plan;
    int rc;
    if (t.nsplit && (rc = ensure(c, c->tol_bins, sizeof(uint32_t) * WC_HIST_BINS * (size_t)maxl * t.nsplit))) return rc;
    float* th = d_thresh ? d_thresh : (float*)const_cast<uint8_t*>(d_blob + t.o_thresh);
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const LtUnit* lt = (const LtUnit*)d_blob;
    BudgetState* state = (BudgetState*)const_cast<uint8_t*>(d_blob + t.o_tail);
    const uint32_t* maxp = (const uint32_t*)(d_blob + t.o_tail + sizeof(BudgetState) * t.nsplit);
    StageTimer timer(c, WC_STAGE_TOL);
    hipError_t e = launch_budget(c->stream, du, n, lt, maxp, (const uint2*)(d_blob + t.o_items), t.nitems, t.chunk,
                                 (const uint32_t*)(d_blob + t.o_split), t.nsplit, maxl, (const float*)c->coef.p,
                                 (uint32_t*)c->tol_bins.p, state, th, d_key);
    if (e == hipSuccess)
        e = launch_leveltol_mask(c->stream, du, lt, (const FTile*)P.d_ftiles.p, (uint32_t)P.ftiles.size(),
                                 (float*)c->coef.p, th);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "size budget launch");
}

// Max-error mode, between the level passes and the emit: the three probe passes
// and the pick of every unit (wc_maxerr.hip), then the mask pass of the
// tolerance mode with the one threshold per unit in its slots.  The tail of the
// blob: state[3][n][16] (zeroed) | prefix[n + 1], the units' first probe tiles.
constexpr size_t kMaxerrStateUnit = 3 * 16 * sizeof(uint64_t);
int stage_maxerr(wc_ctx* c, int n, int maxl, const LevelTolWork& t, const uint8_t* d_blob, const void* d_cells,
                 int dtype, uint32_t ntiles, float* d_thresh, double* d_err) {
    const Plan& P = c->plan;
    float* slots = (float*)const_cast<uint8_t*>(d_blob + t.o_thresh);
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const LtUnit* lt = (const LtUnit*)d_blob;
    unsigned long long* state = (unsigned long long*)const_cast<uint8_t*>(d_blob + t.o_tail);
    const uint32_t* prefix = (const uint32_t*)(d_blob + t.o_tail + kMaxerrStateUnit * n);
    StageTimer timer(c, WC_STAGE_TOL);
    hipError_t e = launch_maxerr_select(c->stream, du, n, lt, prefix, ntiles, maxl, d_cells, dtype,
                                        (const float*)c->coef.p, state, slots, d_thresh, d_err);
    if (e == hipSuccess)
        e = launch_leveltol_mask(c->stream, du, lt, (const FTile*)P.d_ftiles.p, (uint32_t)P.ftiles.size(),
                                 (float*)c->coef.p, slots);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "max-error launch");
}

bool single_level(const int32_t* levels, int n) {
    for (int i = 0; i < n; ++i)
        if (levels[i] != 1) return false;
    return true;
}

// What wc_forward_levels, _tol and _budget begin with, in the order that decides
// which error a caller sees first: units, dtype, n == 0, null buffers (own_ok:
// the mode's own buffers are there), the mode's `validate`, the capacity, the
// alignments (`more`: the mode's own outputs), then the device, the plan and
// the scratch.  *run = false: the call ends here with the value returned (an
// error, or WC_OK for n == 0).
struct AlignedArg {
    const void* p;
    const char* what;
    uintptr_t align;
};
template <class Validate>
int forward_levels_begin(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const void* d_payload,
                         uint64_t cap, const void* d_offsets, const void* d_kept, bool own_ok, Validate validate,
                         std::initializer_list<AlignedArg> more, bool* run) {
    *run = false;
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_payload || !d_offsets || !d_kept || !own_ok) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate())) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_payload, "payload")) ||
        (rc = check_aligned(c, d_offsets, "offsets", 8)) || (rc = check_aligned(c, d_kept, "kept", 4)))
        return rc;
    for (const AlignedArg& a : more)
        if ((rc = check_aligned(c, a.p, a.what, a.align))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n)) || (rc = ensure_scratch(c))) return rc;
    *run = true;
    return WC_OK;
}

// ... and end with: ncoeff = -L into the headers of the units with L >= 2.
int patch_level_headers(wc_ctx* c, const LevelWork& w, uint8_t* d_payload) {
    StageTimer t(c, WC_STAGE_LEVELS);
    hipError_t e = launch_level_headers(c->stream, (const UnitDev*)c->plan.d_units.p, w.hdr, w.nhdr, d_payload);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "level header launch");
}

// wc_forward_emit and _tol after their argument checks: these units' plan must
// be the one whose coefficients are staged (staged: as the mode needs them);
// then the per-unit tile tickets (tdone) and the look-back status words, which
// are per call: everything after the unit keys is zeroed.
int restage(wc_ctx* c, const wc_unit* units, int n, bool staged, const char* who) {
    const uint64_t gen = c->plan_gen;
    int rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    // get_plan keeps the cached plan (and so the staged scratch) only for the same units
    if (!staged || gen != c->plan_gen)
        return fail(c, WC_ERR_INVALID, std::string(who) + ": no staged coefficients for these units (wc_forward_stage)");
    const size_t st_off = 16 + 8ull * n;
    hipError_t e = hipMemsetAsync((uint8_t*)c->state.p + st_off, 0, c->plan.state_bytes - st_off, c->stream);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "memset status");
}

}  // namespace

extern "C" {

const char* wc_version(void) { return "wavelet_amd 0.2 (gfx950; fp-contract=off, no denormal flush)"; }

int wc_device_count(void) {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess ? ndev : 0;
}

int wc_ctx_create(int device, wc_ctx** out) {
    if (!out) return WC_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return WC_ERR_HIP;
    if (device < 0 || device >= ndev) return WC_ERR_INVALID;
    wc_ctx* c = new wc_ctx();
    c->device = device;
    if (set_device(c) != WC_OK) {
        delete c;
        return WC_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return WC_ERR_HIP;
    }
    c->stream = c->own;
    // the persistent error word (check_kernel_errors reads and clears it)
    if (ensure(c, c->errflag, 16) != WC_OK || hipMemset(c->errflag.p, 0, 16) != hipSuccess) {
        wc_ctx_destroy(c);
        return WC_ERR_NOMEM;
    }
    *out = c;
    return WC_OK;
}

void wc_ctx_destroy(wc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    DevBuf* bufs[] = {&c->coef,          &c->part,           &c->errflag,        &c->state,
                      &c->flags,         &c->h_cells,        &c->h_payload,      &c->h_packed,
                      &c->h_offsets,     &c->h_poff,         &c->h_kept,         &c->h_out,
                      &c->h_rows,        &c->h_rmse,
                      &c->plan.d_units,  &c->plan.d_xtiles,  &c->plan.d_ftiles,  &c->plan.d_dtiles,
                      &c->plan.d_edesc, &c->plan.d_ixtiles, &c->plan.d_rtiles,
                      &c->plan.d_rdtiles, &c->rowinfo,    &c->istate,        &c->npairs,
                      &c->tol_in,        &c->tol_bins,       &c->h_thresh,       &c->h_bound,
                      &c->lv_side,       &c->pk_desc,        &c->pk_in,          &c->pk_out,
                      &c->pk_off,        &c->pk_bytes,       &c->thin,           &c->merge,
                      &c->h_second,      &c->h_second_off,   &c->h_second_cnt};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (Plan& P : c->plan_cache) free_plan(P);
    for (hipEvent_t e : c->hev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->iev) (void)hipEventDestroy(e);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->up) (void)hipStreamDestroy(c->up);
    if (c->down) (void)hipStreamDestroy(c->down);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->bounce) (void)hipHostFree(c->bounce);
    if (c->tol_pin) (void)hipHostFree(c->tol_pin);
    if (c->tol_ev) (void)hipEventDestroy(c->tol_ev);
    for (hipEvent_t e : c->bev) (void)hipEventDestroy(e);
    for (auto& m : c->marks) {
        c->ev_pool.push_back(m.a);
        c->ev_pool.push_back(m.b);
    }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

const char* wc_last_error(const wc_ctx* c) { return c ? c->err.c_str() : "null context"; }

int wc_set_stream(wc_ctx* c, void* s) {
    if (!c) return WC_ERR_INVALID;
    hipStream_t next = s ? (hipStream_t)s : c->own;
    // Kernels queued on the old stream may still read the plan's descriptors
    // and the scratch, which later calls rebuild or reuse in stream order on
    // the new stream: drain the old one first.
    // The switch happens even when the drain fails (a stale handle must not
    // stay the context's stream); the failure is still reported.
    hipError_t e = hipSuccess;
    if (next != c->stream) e = hipStreamSynchronize(c->stream);
    c->stream = next;
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "wc_set_stream: synchronize the previous stream");
}

int wc_set_option(wc_ctx* c, int option, int64_t value) {
    if (!c) return WC_ERR_INVALID;
    switch (option) {
        case WC_OPT_SPARSE:
            c->opt_sparse = value != 0;
            return WC_OK;
        case WC_OPT_RIX_XCD:
            c->opt_rix_xcd = value != 0;
            return WC_OK;
        case WC_OPT_INV_GROUPS:
            if (value < 1 || value > 16) return fail(c, WC_ERR_INVALID, "WC_OPT_INV_GROUPS: 1..16");
            c->opt_inv_groups = (int)value;
            return WC_OK;
        case WC_OPT_ORDERED:
            c->opt_ordered = value != 0;
            return WC_OK;
        case WC_OPT_INVERSE_ROWS:
            c->opt_inv_rows = value != 0;
            return WC_OK;
        case WC_OPT_RIX_LDS:
            if (value < 1024 || value > 16384) return fail(c, WC_ERR_INVALID, "WC_OPT_RIX_LDS: 1024..16384 floats");
            c->opt_rix_lds = (int)value;
            return WC_OK;
        case WC_OPT_RIX_BLOCKED:
            c->opt_rix_blocked = value != 0;
            return WC_OK;
        case WC_OPT_RIX_TX:
            if (value < 0 || value > 5) return fail(c, WC_ERR_INVALID, "WC_OPT_RIX_TX: log2 of 1..32 blocks");
            c->opt_rix_lx = (int)value;
            return WC_OK;
        case WC_OPT_HOST_CHUNK:
            if (value < 0) return fail(c, WC_ERR_INVALID, "WC_OPT_HOST_CHUNK: cells >= 0");
            c->opt_host_chunk = value;
            return WC_OK;
        case WC_OPT_SPIN_LIMIT: {
            if (value < 0 || value > 0xffffffffll) return fail(c, WC_ERR_INVALID, "WC_OPT_SPIN_LIMIT: 0..2^32-1 polls");
            hipError_t e;
            if ((e = hipSetDevice(c->device)) != hipSuccess ||
                (e = hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)c->errflag.p + 1), (int)(uint32_t)value, 1,
                                       c->stream)) != hipSuccess)
                return hip_fail(c, e, "WC_OPT_SPIN_LIMIT");
            c->opt_spin_limit = (uint32_t)value;
            return WC_OK;
        }
        case WC_OPT_TICKETS:
            c->force_tickets = value != 0;
            return WC_OK;
        case WC_OPT_REVERSE_TILES:
            c->opt_reverse = value != 0;
            return WC_OK;
        case WC_OPT_HOST_THREADS:
            if (value < -1 || value > 256) return fail(c, WC_ERR_INVALID, "WC_OPT_HOST_THREADS: -1..256");
            c->opt_host_threads = (int)value;
            return WC_OK;
        case WC_OPT_HOST_THP:
            c->opt_host_thp = value != 0;
            return WC_OK;
        case WC_OPT_TOL_SOLO_TILES:
            if (value < 1 || value > (int64_t(1) << 19))
                return fail(c, WC_ERR_INVALID, "WC_OPT_TOL_SOLO_TILES: 1..2^19 flat tiles");
            c->opt_tol_solo = (int)value;
            return WC_OK;
        default:
            return fail(c, WC_ERR_INVALID, "unknown option");
    }
}

int wc_get_option(const wc_ctx* c, int option, int64_t* value) {
    if (!c || !value) return WC_ERR_INVALID;
    switch (option) {
        case WC_OPT_SPARSE: *value = c->opt_sparse; return WC_OK;
        case WC_OPT_RIX_XCD: *value = c->opt_rix_xcd; return WC_OK;
        case WC_OPT_INV_GROUPS: *value = c->opt_inv_groups; return WC_OK;
        case WC_OPT_ORDERED: *value = use_ordered(c) ? 1 : 0; return WC_OK;  // the form the next launch takes
        case WC_OPT_INVERSE_ROWS: *value = c->opt_inv_rows; return WC_OK;
        case WC_OPT_RIX_LDS: *value = c->opt_rix_lds; return WC_OK;
        case WC_OPT_RIX_TX: *value = c->opt_rix_lx; return WC_OK;
        case WC_OPT_RIX_BLOCKED: *value = c->opt_rix_blocked; return WC_OK;
        case WC_OPT_HOST_CHUNK: *value = c->opt_host_chunk; return WC_OK;
        case WC_OPT_SPIN_LIMIT: *value = c->opt_spin_limit; return WC_OK;
        case WC_OPT_TICKETS: *value = c->force_tickets ? 1 : 0; return WC_OK;
        case WC_OPT_REVERSE_TILES: *value = c->opt_reverse ? 1 : 0; return WC_OK;
        case WC_OPT_HOST_THREADS:
            *value = c->opt_host_threads < 0 ? host_threads_default() : c->opt_host_threads;
            return WC_OK;
        case WC_OPT_HOST_THP: *value = c->opt_host_thp; return WC_OK;
        case WC_OPT_TOL_SOLO_TILES: *value = c->opt_tol_solo; return WC_OK;
        default: return WC_ERR_INVALID;
    }
}

int wc_synchronize(wc_ctx* c) {
    if (!c) return WC_ERR_INVALID;
    hipError_t e = hipStreamSynchronize(c->stream);
    // the pipelined inverse's second stream joins c->stream on success; drain it
    // too, so no queued work outlives a synchronize on any path
    if (e == hipSuccess && c->aux) e = hipStreamSynchronize(c->aux);
    if (e != hipSuccess) return hip_fail(c, e, "hipStreamSynchronize");
    return check_kernel_errors(c);
}

int wc_forward(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, double keep,
               uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_payload || !d_offsets || !d_kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_payload, "payload")) ||
        (rc = check_aligned(c, d_offsets, "offsets", 8)) || (rc = check_aligned(c, d_kept, "kept", 4)))
        return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    if ((rc = ensure_scratch(c))) return rc;
    return forward_staged(c, d_cells, dtype, n, keep, d_payload, d_offsets, d_kept);
}

int wc_forward_rows(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, double keep,
                    uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept, void* d_rowinfo,
                    uint64_t rowinfo_capacity) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_payload || !d_offsets || !d_kept || !d_rowinfo) return fail(c, WC_ERR_INVALID, "null buffer");
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if (rowinfo_capacity < wc_rowindex_bytes(units, n))
        return fail(c, WC_ERR_INVALID, "rowinfo_capacity < wc_rowindex_bytes");
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_payload, "payload")) ||
        (rc = check_aligned(c, d_offsets, "offsets", 8)) || (rc = check_aligned(c, d_kept, "kept", 4)) ||
        (rc = check_aligned(c, d_rowinfo, "rowinfo", 8)))
        return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    if (c->plan.rowinfo_entries > 0xffffffffull)  // the emit descriptors keep 32-bit row offsets
        return fail(c, WC_ERR_INVALID, "wc_forward_rows: more than 2^32 row-index entries in one batch");
    if ((rc = ensure_scratch(c))) return rc;
    return forward_staged(c, d_cells, dtype, n, keep, d_payload, d_offsets, d_kept, (uint2*)d_rowinfo);
}

int wc_forward_stage(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, uint64_t* d_hist) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = check_aligned(c, d_cells, "cells"))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    // dense staging: the histogram and any later threshold need every coefficient
    if ((rc = ensure_scratch(c))) return rc;
    if (!d_hist) {
        if ((rc = stage_transform(c, d_cells, dtype, 0.0, false))) return rc;
        c->staged = true;
        return WC_OK;
    }
    // The fast tiles bin their coefficients as K1 stages them (k_transform_hist:
    // no re-read of the staged coefficients); the generic ones (odd dims, D % 8
    // != 0) stage as usual and k_hist bins those units afterwards.
    Plan& P = c->plan;
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const XTile* dxt = (const XTile*)P.d_xtiles.p;
    unsigned long long* key = (unsigned long long*)((uint8_t*)c->state.p + 16);
    float* coef = (float*)c->coef.p;
    hipError_t e = hipMemsetAsync(c->state.p, 0, P.state_bytes, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "memset state");
    {
        StageTimer t(c, WC_STAGE_TRANSFORM);
        e = launch_transform(c->stream, d_cells, dtype, du, dxt, P.ngen, P.lds_gen, coef, 0, key);
        if (e == hipSuccess)
            e = launch_transform_hist(c->stream, d_cells, dtype, du, dxt + P.ngen, P.nfast, P.lds_fast, coef, key,
                                      (unsigned long long*)d_hist,
                                      persistent_grid(c, 2, transform_hist_lds_bytes(P.lds_fast)));
        if (e != hipSuccess) return hip_fail(c, e, "transform launch");
    }
    c->sparse_staged = false;
    if (P.ngen) {
        const uint32_t max_blocks = 2048;  // 8 workgroups per CU, 256 CUs
        StageTimer t(c, WC_STAGE_HIST);
        e = launch_hist(c->stream, du, (const FTile*)P.d_ftiles.p, (uint32_t)P.ftiles.size(), coef, max_blocks,
                        (unsigned long long*)d_hist, true);
        if (e != hipSuccess) return hip_fail(c, e, "histogram launch");
    }
    c->staged = true;
    return WC_OK;
}

int wc_hist_threshold(const uint64_t* hist, double quantile, float* thresh, uint64_t* retained) {
    if (!hist || !thresh || !(quantile >= 0.0 && quantile <= 1.0)) return WC_ERR_INVALID;
    uint64_t total = 0;
    for (int b = 0; b < WC_HIST_BINS; ++b) total += hist[b];
    const uint64_t drop = (uint64_t)std::floor(quantile * (double)total);
    const uint64_t target = total - std::min(drop, total);
    uint64_t cum = 0;
    int bstar = -1;  // -1: keep nothing
    if (target > 0)
        for (int b = WC_HIST_BINS - 1; b >= 0; --b) {
            cum += hist[b];
            if (cum >= target) {
                bstar = b;
                break;
            }
        }
    float t;
    if (bstar < 0) {
        t = __builtin_inff();  // |c| > inf never holds
        cum = 0;
    } else if (bstar == 0) {
        t = -1.0f;  // every non-NaN coefficient
    } else {
        const uint32_t bits = ((uint32_t)bstar << WC_HIST_SHIFT) - 1u;
        std::memcpy(&t, &bits, 4);
    }
    *thresh = t;
    if (retained) *retained = cum;
    return WC_OK;
}

int wc_forward_emit(wc_ctx* c, const wc_unit* units, int n, double keep, const float* thresh, uint8_t* d_payload,
                    uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !d_kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_payload, "payload")) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_kept, "kept", 4)))
        return rc;
    if ((rc = restage(c, units, n, c->staged, "wc_forward_emit"))) return rc;
    if ((rc = stage_emit(c, n, keep, thresh, d_payload, d_offsets, d_kept))) return rc;
    c->staged = true;  // the coefficients are still there: emit again with another threshold
    return WC_OK;
}

int wc_forward_tol(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const double* tol,
                   uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh,
                   double* d_bound) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_payload || !d_offsets || !d_kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_tol(c, units, n, tol))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_payload, "payload")) ||
        (rc = check_aligned(c, d_offsets, "offsets", 8)) || (rc = check_aligned(c, d_kept, "kept", 4)) ||
        (rc = check_aligned(c, d_thresh, "thresh", 4)) || (rc = check_aligned(c, d_bound, "bound", 8)))
        return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    if ((rc = ensure_scratch(c))) return rc;
    // dense staging: the threshold is not known when the transform runs
    const float* uth = nullptr;
    if ((rc = stage_transform(c, d_cells, dtype, 0.0, false)) || (rc = stage_tol(c, n, tol, d_thresh, d_bound, &uth)))
        return rc;
    return stage_emit(c, n, 0.0, nullptr, d_payload, d_offsets, d_kept, nullptr, uth);
}

int wc_forward_emit_tol(wc_ctx* c, const wc_unit* units, int n, const double* tol, uint8_t* d_payload, uint64_t cap,
                        uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !d_kept) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_tol(c, units, n, tol))) return rc;
    if (cap < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "payload_capacity < wc_payload_bound");
    if ((rc = check_aligned(c, d_payload, "payload")) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_kept, "kept", 4)) || (rc = check_aligned(c, d_thresh, "thresh", 4)) ||
        (rc = check_aligned(c, d_bound, "bound", 8)))
        return rc;
    // every coefficient is needed
    if ((rc = restage(c, units, n, c->staged && !c->sparse_staged, "wc_forward_emit_tol"))) return rc;
    const float* uth = nullptr;
    if ((rc = stage_tol(c, n, tol, d_thresh, d_bound, &uth)) ||
        (rc = stage_emit(c, n, 0.0, nullptr, d_payload, d_offsets, d_kept, nullptr, uth)))
        return rc;
    c->staged = true;  // the coefficients are still there: emit again with other tolerances
    return WC_OK;
}

int wc_decompose(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, float* d_flat) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_flat) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_flat, "flat"))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    Plan& P = c->plan;
    const UnitDev* du = (const UnitDev*)P.d_units.p;
    const XTile* dxt = (const XTile*)P.d_xtiles.p;
    StageTimer t(c, WC_STAGE_TRANSFORM);
    hipError_t e = launch_transform(c->stream, d_cells, dtype, du, dxt, P.ngen, P.lds_gen, d_flat, 1, nullptr);
    if (e == hipSuccess)
        e = launch_transform_fast(c->stream, d_cells, dtype, du, dxt + P.ngen, P.nfast, P.lds_fast, d_flat, 1,
                                  nullptr, nullptr, nullptr, 0.0, persistent_grid(c, 0, P.lds_fast));
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "transform launch");
}

}  // extern "C"

namespace {

// Per-call state of the pair-tile scans of a decode (wc_pairscan.h): ticket[n] |
// status[decode tiles] in c->state, `bytes` in all (decode_state_bytes of the
// plan whose decode tiles run), zeroed here; `ordered`: the kernels' tile-index
// argument.  dense: some unit's tiles look back over zeroed granules; without
// one the ordered form needs no state (the row index's granules carry the
// call's epoch) and the clear is skipped.
struct DecodeState {
    uint32_t* ticket;
    unsigned long long* status;
    int ordered;  // 0: tickets, 1: plan order, 2: reversed (WC_OPT_REVERSE_TILES)
};
hipError_t decode_state(wc_ctx* c, int n, size_t bytes, bool dense, DecodeState* s) {
    uint8_t* st = (uint8_t*)c->state.p;
    *s = {(uint32_t*)st, (unsigned long long*)(st + round_up(4ull * n, 8)), tile_order(c)};
    return dense || !s->ordered ? hipMemsetAsync(st, 0, bytes, c->stream) : hipSuccess;
}

// wc_inverse, and with orig != null also calc_rmse_per_box fused into the
// row-indexed inverse (every unit row-indexed; the caller checks).
// user_rows (wc_inverse_rows): the caller's row index of these payloads, as
// wc_forward_rows wrote it: K6r reads it and the row index kernel does not
// run; units that are not row-indexed still decode densely.
int inverse_impl(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, int n, float* d_out,
                 const void* d_orig, int dtype, double* d_rmse, const uint2* user_rows = nullptr) {
    Plan& P = c->plan;
    int rc = WC_OK;
    hipError_t e = hipSuccess;
    // The dense coefficient scratch is fully written by the decode (no memset).
    DecodeState ds;  // once: the clear and the launches must agree on the form
    if ((e = decode_state(c, n, decode_state_bytes(P), !P.dtiles.empty(), &ds)) != hipSuccess)
        return hip_fail(c, e, "memset");
    c->epoch = (c->epoch + 1) & kEpochMask;
    if (c->epoch == 0) {  // wrapped: granules of 2^30 calls ago could look current
        if ((e = hipMemsetAsync(c->istate.p, 0, c->istate.bytes, c->stream)) != hipSuccess)
            return hip_fail(c, e, "memset");
        c->epoch = 1;
    }
    const int ng = (int)P.ig_rd.size() - 1;  // row-indexed groups (0: none)
    const bool piped = ng > 1 && !c->prof && !user_rows;  // profiling times each kernel alone
    const uint2* rows_in = user_rows ? user_rows : (const uint2*)c->rowinfo.p;
    if (piped && (rc = inverse_stream(c, 2 * ng + 2))) return rc;
    auto rows = [&](int g, hipStream_t s) {  // K6r over group g's tiles
        const uint32_t t0 = P.ig_rt[g], nt = P.ig_rt[g + 1] - P.ig_rt[g];
        return launch_inverse_rows(s, (const RTile*)P.d_rtiles.p + t0, nt, P.lds_rows,
                                   nt ? persistent_grid(c, 1, P.lds_rows) : 1u, d_payload, d_offsets, rows_in, d_out,
                                   c->opt_rix_blocked ? 1 : 0, d_orig, dtype, (const UnitDev*)P.d_units.p, n,
                                   (double*)c->part.p, d_rmse, g == ng - 1, (const uint32_t*)c->npairs.p);
    };
    auto index = [&](int g, hipStream_t s) {  // K5 over group g's tiles (g = ng: the dense decode)
        const bool dense = g == ng;
        return launch_decode(s, (const UnitDev*)P.d_units.p, (const FTile*)P.d_dtiles.p,
                             dense ? (uint32_t)P.dtiles.size() : 0u, (const FTile*)P.d_rdtiles.p + (dense ? 0 : P.ig_rd[g]),
                             dense ? 0u : P.ig_rd[g + 1] - P.ig_rd[g], (unsigned long long*)c->istate.p, c->epoch,
                             d_payload, d_offsets, ds.ticket, ds.status, (float*)c->coef.p, (uint2*)c->rowinfo.p,
                             (uint32_t*)c->errflag.p, ds.ordered, (uint32_t*)c->npairs.p);
    };
    if (piped) {
        // K5 of group g + 1 on the context stream beside K6r of group g on the
        // aux stream: the latency-bound row index overlaps the streaming
        // reconstruction; the aux stream joins back before the call returns.
        hipEvent_t* ev = c->iev.data();
        if ((e = hipEventRecord(ev[0], c->stream)) != hipSuccess || (e = hipStreamWaitEvent(c->aux, ev[0], 0)) != hipSuccess)
            return hip_fail(c, e, "inverse pipeline");
        for (int g = 0; g < ng && e == hipSuccess; ++g) {
            e = index(g, c->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[1 + g], c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->aux, ev[1 + g], 0);
            if (e == hipSuccess) e = rows(g, c->aux);
        }
        if (e == hipSuccess && !P.dtiles.empty()) e = index(ng, c->stream);
        if (e == hipSuccess) e = hipEventRecord(ev[1 + ng], c->aux);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev[1 + ng], 0);
        if (e == hipSuccess)
            e = launch_inverse(c->stream, (const float*)c->coef.p, 0, (const UnitDev*)P.d_units.p,
                               (const XTile*)P.d_ixtiles.p, P.ign, P.lds_inverse, P.ifast, P.lds_fast, d_out);
        if (e != hipSuccess) {
            // K6r work already queued on the aux stream still reads the payload
            // and the row index: drain it before the scratch can be reused
            (void)hipStreamSynchronize(c->aux);
            return hip_fail(c, e, "inverse launch");
        }
        c->err_check_pending = true;
        return rc;
    }
    if (ng > 0 && user_rows) {  // the row index is the caller's: check the headers, count the pairs
        StageTimer t(c, WC_STAGE_PAIRS);
        e = launch_pair_counts(c->stream, (const UnitDev*)P.d_units.p, n, d_payload, d_offsets,
                               (uint32_t*)c->npairs.p, (uint32_t*)c->errflag.p);
        if (e != hipSuccess) return hip_fail(c, e, "pair count launch");
    }
    if ((ng > 0 && !user_rows) || !P.dtiles.empty()) {  // a decode stage only when something launches
        StageTimer t(c, WC_STAGE_DECODE);
        for (int g = 0; g <= ng && e == hipSuccess; ++g)
            if ((g < ng && !user_rows) || (g == ng && !P.dtiles.empty())) e = index(g, c->stream);
    }
    if (e != hipSuccess) return hip_fail(c, e, "decode launch");
    {
        StageTimer t(c, WC_STAGE_INVERSE);
        for (int g = 0; g < ng && e == hipSuccess; ++g) e = rows(g, c->stream);
        if (e == hipSuccess && ng == 0 && d_orig)  // every unit empty: the per-unit RMSE (0) only
            e = launch_inverse_rows(c->stream, nullptr, 0, 0, 1u, d_payload, d_offsets, rows_in, d_out, 0, d_orig,
                                    dtype, (const UnitDev*)P.d_units.p, n, (double*)c->part.p, d_rmse, true,
                                    (const uint32_t*)c->npairs.p);
        if (e == hipSuccess)
            e = launch_inverse(c->stream, (const float*)c->coef.p, 0, (const UnitDev*)P.d_units.p,
                               (const XTile*)P.d_ixtiles.p, P.ign, P.lds_inverse, P.ifast, P.lds_fast, d_out);
    }
    if (e != hipSuccess) return hip_fail(c, e, "inverse launch");
    // Malformed payloads surface at the next wc_synchronize (WC_ERR_FORMAT).
    c->err_check_pending = true;
    return rc;
}

// What wc_inverse_coarse and wc_inverse_region fill alike of a unit's descriptor
// (f: the full-size unit, o: its derived unit).  The origin and end stay 0, and
// with them a unit without cells: no tile reads more than the end of such a unit.
void compact_desc(RegionDesc& d, const wc_unit& f, const wc_unit& o, int L, int r) {
    d = RegionDesc{};
    d.L = (uint32_t)(L - r);
    d.direct = r == L ? 1u : 0u;
    d.out_off = o.cell_offset;
    d.W = f.nx;
    d.H = f.ny;
    d.D = f.nz;
    const uint64_t cells = (uint64_t)f.nx * f.ny * f.nz;
    d.want = L >= 2 ? -L : (int32_t)cells;
    if (!cells) return;
    d.w = (uint32_t)(f.nx >> r);
    d.h = (uint32_t)(f.ny >> r);
    d.d = (uint32_t)(f.nz >> r);
    d.sx = (uint32_t)o.nx;
    d.sy = (uint32_t)o.ny;
    d.sz = (uint32_t)o.nz;
    d.dmagic = rows_magic(f.nz);
    d.hmagic = rows_magic(f.ny);
}

// The reduced-resolution and the sub-box inverse, from the units' descriptors
// (dst_off and dt_begin are filled here, from the plans).  Two plans: the one of
// the full-size units gives the pair tiles of the decode and their look-back
// granules; the one of out_units (the derived units: the regions' extents >> r,
// with `whole` the boxes >> r) places each compact unit in the coefficient
// scratch and runs the remaining L - r levels and the one-level inverse on it,
// as wc_inverse_levels does on full arrays.  Both are dense plans
// (WC_OPT_INVERSE_ROWS = 0) and stay in the plan cache.
// packed_cap: d_payload holds packed units, read below *packed_cap (wc_inverse_packed_coarse / _region).
int inverse_compact(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const wc_unit* out_units, float* d_out, std::vector<RegionDesc>& desc, bool whole,
                    const uint64_t* packed_cap = nullptr) {
    int rc;
    if ((rc = check_aligned(c, d_payload, "payload", packed_cap ? 8 : 16)) ||  // packed: as wc_unpack
        (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_out, "out")))
        return rc;
    if ((rc = set_device(c))) return rc;
    std::vector<int32_t> rest(n);  // levels of the compact unit: L - r (1 for r == L, which runs nothing)
    bool any_direct = false, any_run = false;
    uint32_t maxt = 0;  // the batch's largest ceil(end / kFlatTile): no tile index at or past it has work
    for (int u = 0; u < n; ++u) {
        const RegionDesc& d = desc[u];
        rest[u] = std::max<int32_t>(1, (int32_t)d.L);
        if (!d.end) continue;  // a unit or a region without cells
        maxt = std::max(maxt, (d.end - 1) / (uint32_t)kFlatTile + 1);
        any_direct |= d.direct != 0;
        any_run |= d.direct == 0;
    }
    const FTile* dtiles = nullptr;
    uint32_t ndt = 0;
    size_t dstate = 0;
    {
        DensePlans dense(c);  // both plans, as wc_inverse_levels': the full units' (the decode's tiles), then the compact units'
        if ((rc = dense_plan(c, units, n, true)) == WC_OK) {
            const Plan& F = c->plan;
            dtiles = (const FTile*)F.d_dtiles.p;  // the plan moves into the cache below: its buffers stay
            dstate = decode_state_bytes(F);
            // dtiles is ordered by tile index, then unit: the tiles below maxt are a prefix of it
            for (int u = 0; u < n; ++u) {
                desc[u].dt_begin = F.units[u].dt_begin;
                ndt += std::min(F.units[u].ndt, maxt);
            }
            rc = get_plan(c, out_units, n);
        }
    }
    if (rc || (rc = ensure_scratch(c)) || (rc = ensure(c, c->state, dstate))) return rc;
    const Plan& P = c->plan;
    for (int u = 0; u < n; ++u) desc[u].dst_off = P.units[u].coef_off;
    LevelWork w;
    const void* d_desc = nullptr;
    if ((rc = upload_levels(c, n, rest.data(), &w, desc.data(), sizeof(RegionDesc) * n, &d_desc))) return rc;
    DecodeState ds;
    hipError_t e = decode_state(c, n, dstate, true, &ds);
    if (e != hipSuccess) return hip_fail(c, e, "memset");
    uint32_t* bad = (uint32_t*)c->npairs.p;  // per-unit "skip" words, as in wc_inverse_levels
    {
        StageTimer t(c, WC_STAGE_DECODE);
        // the compact units: positions without a pair must read as zeros
        if (P.coef_extent && (e = hipMemsetAsync(c->coef.p, 0, sizeof(float) * P.coef_extent, c->stream)) != hipSuccess)
            return hip_fail(c, e, "memset");
        e = launch_decode_region(c->stream, (const RegionDesc*)d_desc, dtiles, ndt, d_payload, d_offsets, ds.ticket,
                                 ds.status, (float*)c->coef.p, (uint32_t*)c->errflag.p, ds.ordered, bad, whole,
                                 packed_cap);
        // the units with r == L: their compact units are their cells
        if (e == hipSuccess && any_direct)
            e = launch_corner_box(c->stream, (const RegionDesc*)d_desc, (const FTile*)P.d_ftiles.p,
                                  (uint32_t)P.ftiles.size(), (const float*)c->coef.p, d_out, bad);
        if (e != hipSuccess) return hip_fail(c, e, "compact decode launch");
    }
    c->err_check_pending = true;  // malformed payloads surface at the next wc_synchronize
    if (w.maxl >= 2 && (rc = run_levels(c, w, false, false, bad))) return rc;
    if (!any_run) return WC_OK;  // every compact unit was its result, or no region had cells
    StageTimer t(c, WC_STAGE_INVERSE);
    e = launch_inverse(c->stream, (const float*)c->coef.p, 0, (const UnitDev*)P.d_units.p, (const XTile*)P.d_ixtiles.p,
                       P.ign, P.lds_inverse, P.ifast, P.lds_fast, d_out, bad);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "inverse launch");
}

int inverse_dense(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                  const int32_t* levels, float* d_out, const uint64_t* packed_cap);

}  // namespace

extern "C" {

int wc_inverse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
               float* d_out) {
    return wc_inverse_rows(c, d_payload, d_offsets, units, n, nullptr, 0, nullptr, WC_F32, d_out, nullptr);
}

int wc_inverse_rmse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const void* d_orig, int dtype, float* d_out, double* d_rmse) {
    if (!c) return WC_ERR_INVALID;
    if (n > 0 && (!d_orig || !d_rmse)) return fail(c, WC_ERR_INVALID, "null buffer");
    return wc_inverse_rows(c, d_payload, d_offsets, units, n, nullptr, 0, d_orig, dtype, d_out, d_rmse);
}

// wc_inverse / wc_inverse_rmse, and with d_rowinfo the caller's row index in
// place of the row index kernel (wc_forward_rows wrote it for these payloads).
int wc_inverse_rows(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const void* d_rowinfo, uint64_t rowinfo_capacity, const void* d_orig, int dtype, float* d_out,
                    double* d_rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (d_orig && dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !d_out || (!d_orig != !d_rmse)) return fail(c, WC_ERR_INVALID, "null buffer");
    if (d_rowinfo && rowinfo_capacity < wc_rowindex_bytes(units, n))
        return fail(c, WC_ERR_INVALID, "rowinfo_capacity < wc_rowindex_bytes");
    if ((rc = check_aligned(c, d_payload, "payload")) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_out, "out")) || (rc = check_aligned(c, d_rowinfo, "rowinfo", 8)) ||
        (rc = check_aligned(c, d_rmse, "rmse", 8)) ||
        (rc = check_aligned(c, d_orig, "orig", dtype == WC_F64 ? 8 : 4)))
        return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n)) || (rc = ensure_scratch(c))) return rc;
    const uint2* rows = (const uint2*)d_rowinfo;
    if (!d_orig) return inverse_impl(c, d_payload, d_offsets, n, d_out, nullptr, 0, nullptr, rows);
    const Plan& P = c->plan;
    bool all_rix = true;
    for (const UnitDev& d : P.units) all_rix &= d.rix != 0 || d.ncells == 0;
    if (!all_rix) {  // some units decode densely: the two calls, same results
        if ((rc = inverse_impl(c, d_payload, d_offsets, n, d_out, nullptr, 0, nullptr, rows))) return rc;
        return wc_rmse(c, d_orig, dtype, d_out, units, n, d_rmse);
    }
    return inverse_impl(c, d_payload, d_offsets, n, d_out, d_orig, dtype == WC_F64 ? 1 : 0, d_rmse, rows);
}

int wc_inverse_flat(wc_ctx* c, const float* d_flat, const wc_unit* units, int n, float* d_out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_flat || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = check_aligned(c, d_flat, "flat")) || (rc = check_aligned(c, d_out, "out"))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    Plan& P = c->plan;
    StageTimer t(c, WC_STAGE_INVERSE);
    hipError_t e = launch_inverse(c->stream, d_flat, 1, (const UnitDev*)P.d_units.p, (const XTile*)P.d_xtiles.p,
                                  P.ngen, P.lds_inverse, P.nfast, P.lds_fast, d_out);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "inverse launch");
}

// Multi-level forward: the one-level transform staged densely, the level
// passes, then the emit on the final array and ncoeff = -L into the headers of
// the units with L >= 2.  Leaves nothing staged.
int wc_forward_levels(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const int32_t* levels,
                      double keep, const float* thresh, uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets,
                      uint32_t* d_kept) {
    bool run;
    int rc = forward_levels_begin(c, d_cells, dtype, units, n, d_payload, cap, d_offsets, d_kept, true,
                                  [&] { return validate_levels(c, units, n, levels); }, {}, &run);
    if (!run) return rc;
    if (single_level(levels, n) && !thresh)  // wc_forward itself
        return forward_staged(c, d_cells, dtype, n, keep, d_payload, d_offsets, d_kept);
    LevelWork w;
    // dense staging: the level passes and the final threshold need every coefficient
    if ((rc = upload_levels(c, n, levels, &w)) || (rc = stage_transform(c, d_cells, dtype, 0.0, false)) ||
        (rc = run_levels(c, w, true, !thresh)) || (rc = stage_emit(c, n, keep, thresh, d_payload, d_offsets, d_kept)))
        return rc;
    return patch_level_headers(c, w, d_payload);
}

// Multi-level forward with per-unit RMSE tolerances: wc_forward_levels' staging
// and level passes, then the per-level bins, pick and mask pass on the final
// array, the unchanged emit with threshold 0.0f on what the mask left, and the
// header patch.  Leaves nothing staged.
int wc_forward_levels_tol(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n,
                          const int32_t* levels, const double* tol, uint8_t* d_payload, uint64_t cap,
                          uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    bool run;
    int rc = forward_levels_begin(
        c, d_cells, dtype, units, n, d_payload, cap, d_offsets, d_kept, true,
        [&] {  // an odd dimension passes validate_levels only at L = 1, where validate_tol refuses it
            const int v = validate_levels(c, units, n, levels);
            return v ? v : validate_tol(c, units, n, tol);
        },
        {{d_thresh, "thresh", 4}, {d_bound, "bound", 8}}, &run);
    if (!run) return rc;
    LevelWork w;
    LevelTolWork t;
    build_leveltol(c, n, levels, tol, !d_thresh, &t);
    const void* d_blob = nullptr;
    const float zero = 0.0f;  // the mask pass has applied the thresholds: the emit keeps every non-zero
    if ((rc = upload_levels(c, n, levels, &w, t.blob.data(), t.blob.size(), &d_blob)) ||
        (rc = stage_transform(c, d_cells, dtype, 0.0, false)) || (rc = run_levels(c, w, true, false)) ||
        (rc = stage_leveltol(c, n, w.maxl, t, (const uint8_t*)d_blob, d_thresh, d_bound)) ||
        (rc = stage_emit(c, n, 0.0, &zero, d_payload, d_offsets, d_kept)))
        return rc;
    return patch_level_headers(c, w, d_payload);
}

// Multi-level forward under a pair budget per unit: wc_forward_levels' staging
// and level passes, the radix select and the mask pass on the final array, the
// unchanged emit with threshold 0.0f, the header patch.  No device-to-host read
// anywhere: the select's state stays on the device.  Leaves nothing staged.
int wc_forward_levels_budget(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n,
                             const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_payload, uint64_t cap,
                             uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    std::vector<int32_t> ones;
    bool run;
    int rc = forward_levels_begin(
        c, d_cells, dtype, units, n, d_payload, cap, d_offsets, d_kept, max_pairs != nullptr,
        [&] {
            levels = levels_or_ones(levels, n, ones);
            return validate_budget(c, units, n, levels);
        },
        {{d_thresh, "thresh", 4}, {d_key, "key", 4}}, &run);
    if (!run) return rc;
    LevelWork w;
    LevelTolWork t;
    build_leveltol(c, n, levels, nullptr, !d_thresh, &t, sizeof(uint32_t), sizeof(BudgetState));
    std::memcpy(t.blob.data() + t.o_tail + sizeof(BudgetState) * t.nsplit, max_pairs, sizeof(uint32_t) * n);
    const void* d_blob = nullptr;
    const float zero = 0.0f;  // the mask pass has applied the thresholds: the emit keeps every non-zero
    if ((rc = upload_levels(c, n, levels, &w, t.blob.data(), t.blob.size(), &d_blob)) ||
        (rc = stage_transform(c, d_cells, dtype, 0.0, false)) || (rc = run_levels(c, w, true, false)) ||
        (rc = stage_budget(c, n, w.maxl, t, (const uint8_t*)d_blob, d_thresh, d_key)) ||
        (rc = stage_emit(c, n, 0.0, &zero, d_payload, d_offsets, d_kept)))
        return rc;
    return patch_level_headers(c, w, d_payload);
}

// Multi-level forward under a pointwise error bound per unit: wc_forward_levels'
// staging and level passes, the probe passes, the pick and the mask pass on the
// final array, the unchanged emit with threshold 0.0f, the header patch.  No
// device-to-host read anywhere: the search's state stays on the device.  Leaves
// nothing staged.
int wc_forward_levels_maxerr(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n,
                             const int32_t* levels, const double* maxerr, uint8_t* d_payload, uint64_t cap,
                             uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, double* d_err) {
    std::vector<int32_t> ones;
    bool run;
    int rc = forward_levels_begin(
        c, d_cells, dtype, units, n, d_payload, cap, d_offsets, d_kept, maxerr != nullptr,
        [&] {
            levels = levels_or_ones(levels, n, ones);
            return validate_maxerr(c, units, n, levels, maxerr);
        },
        {{d_thresh, "thresh", 4}, {d_err, "err", 8}}, &run);
    if (!run) return rc;
    LevelWork w;
    LevelTolWork t;
    // the mask pass's slots are always the call's own: d_thresh holds one float per unit
    build_leveltol(c, n, levels, maxerr, true, &t, kMaxerrStateUnit + 2 * sizeof(uint32_t));
    int maxl = 1;
    for (int u = 0; u < n; ++u) maxl = std::max(maxl, (int)levels[u]);
    std::vector<uint32_t> prefix(n + 1, 0u);
    for (int u = 0; u < n; ++u) {
        const UnitDev& d = c->plan.units[u];
        prefix[u + 1] = prefix[u] + (d.ncells ? maxerr_tiles(maxl, d.nx, d.ny, d.nz) : 0u);
    }
    std::memcpy(t.blob.data() + t.o_tail + kMaxerrStateUnit * n, prefix.data(), sizeof(uint32_t) * (n + 1));
    const void* d_blob = nullptr;
    const float zero = 0.0f;  // the mask pass has applied the thresholds: the emit keeps every non-zero
    if ((rc = upload_levels(c, n, levels, &w, t.blob.data(), t.blob.size(), &d_blob)) ||
        (rc = stage_transform(c, d_cells, dtype, 0.0, false)) || (rc = run_levels(c, w, true, false)) ||
        (rc = stage_maxerr(c, n, maxl, t, (const uint8_t*)d_blob, d_cells, dtype, prefix[n], d_thresh, d_err)) ||
        (rc = stage_emit(c, n, 0.0, &zero, d_payload, d_offsets, d_kept)))
        return rc;
    return patch_level_headers(c, w, d_payload);
}

int wc_decompose_levels(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const int32_t* levels,
                        float* d_flat) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_cells || !d_flat) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if (single_level(levels, n)) return wc_decompose(c, d_cells, dtype, units, n, d_flat);
    if ((rc = check_aligned(c, d_cells, "cells")) || (rc = check_aligned(c, d_flat, "flat"))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n)) || (rc = ensure_scratch(c))) return rc;
    // through the coefficient scratch (aligned units, the side scratch beside it), then out
    LevelWork w;
    if ((rc = upload_levels(c, n, levels, &w)) || (rc = stage_transform(c, d_cells, dtype, 0.0, false)) ||
        (rc = run_levels(c, w, true, false)))
        return rc;
    const Plan& P = c->plan;
    StageTimer t(c, WC_STAGE_LEVELS);
    hipError_t e = launch_level_flat(c->stream, (const UnitDev*)P.d_units.p, (const FTile*)P.d_ftiles.p,
                                     (uint32_t)P.ftiles.size(), (float*)c->coef.p, d_flat, 1);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "flat copy launch");
}

int wc_inverse_flat_levels(wc_ctx* c, const float* d_flat, const wc_unit* units, int n, const int32_t* levels,
                           float* d_out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_flat || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if (single_level(levels, n)) return wc_inverse_flat(c, d_flat, units, n, d_out);
    if ((rc = check_aligned(c, d_flat, "flat")) || (rc = check_aligned(c, d_out, "out"))) return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n)) || (rc = ensure_scratch(c))) return rc;
    LevelWork w;
    if ((rc = upload_levels(c, n, levels, &w))) return rc;
    const Plan& P = c->plan;
    hipError_t e;
    {
        StageTimer t(c, WC_STAGE_LEVELS);
        e = launch_level_flat(c->stream, (const UnitDev*)P.d_units.p, (const FTile*)P.d_ftiles.p,
                              (uint32_t)P.ftiles.size(), (float*)c->coef.p, const_cast<float*>(d_flat), 0);
        if (e != hipSuccess) return hip_fail(c, e, "flat copy launch");
    }
    if ((rc = run_levels(c, w, false, false))) return rc;
    StageTimer t(c, WC_STAGE_INVERSE);
    e = launch_inverse(c->stream, (const float*)c->coef.p, 0, (const UnitDev*)P.d_units.p, (const XTile*)P.d_xtiles.p,
                       P.ngen, P.lds_inverse, P.nfast, P.lds_fast, d_out);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "inverse launch");
}

// Multi-level inverse: every unit through the dense decode (the plan of
// WC_OPT_INVERSE_ROWS = 0), the synthesis passes on the coefficient scratch,
// then the one-level inverse of all units.
int wc_inverse_levels(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, float* d_out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    if (single_level(levels, n)) return wc_inverse(c, d_payload, d_offsets, units, n, d_out);
    return inverse_dense(c, d_payload, d_offsets, units, n, levels, d_out, nullptr);
}

}  // extern "C"

namespace {

// wc_inverse_levels after its checks, and wc_inverse_packed (packed_cap: d_payload
// holds packed units, read below *packed_cap; then also for batches of L = 1).
int inverse_dense(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                  const int32_t* levels, float* d_out, const uint64_t* packed_cap) {
    int rc;
    if ((rc = check_aligned(c, d_payload, "payload", packed_cap ? 8 : 16)) ||  // packed: as wc_unpack
        (rc = check_aligned(c, d_offsets, "offsets", 8)) || (rc = check_aligned(c, d_out, "out")))
        return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = dense_plan(c, units, n, false)) || (rc = ensure_scratch(c))) return rc;
    LevelWork w;
    if ((rc = upload_levels(c, n, levels, &w))) return rc;
    const Plan& P = c->plan;
    DecodeState ds;
    hipError_t e = decode_state(c, n, decode_state_bytes(P), true, &ds);
    if (e != hipSuccess) return hip_fail(c, e, "memset");
    // per-unit "header disagrees" words, written by each unit's first decode tile (a unit
    // without cells has neither decode nor inverse tiles); npairs is free: no unit is row-indexed
    uint32_t* bad = (uint32_t*)c->npairs.p;
    {
        StageTimer t(c, WC_STAGE_DECODE);
        e = packed_cap
                ? launch_decode_packed(c->stream, (const UnitDev*)P.d_units.p, (const FTile*)P.d_dtiles.p,
                                       (uint32_t)P.dtiles.size(), d_payload, d_offsets, *packed_cap, ds.ticket, ds.status,
                                       (float*)c->coef.p, (uint32_t*)c->errflag.p, ds.ordered, w.levels, bad)
                : launch_decode(c->stream, (const UnitDev*)P.d_units.p, (const FTile*)P.d_dtiles.p,
                                (uint32_t)P.dtiles.size(), nullptr, 0u, nullptr, 0u, d_payload, d_offsets, ds.ticket,
                                ds.status, (float*)c->coef.p, nullptr, (uint32_t*)c->errflag.p, ds.ordered, bad, w.levels);
        if (e != hipSuccess) return hip_fail(c, e, "decode launch");
    }
    c->err_check_pending = true;  // malformed payloads surface at the next wc_synchronize
    if ((rc = run_levels(c, w, false, false, bad))) return rc;
    StageTimer t(c, WC_STAGE_INVERSE);
    e = launch_inverse(c->stream, (const float*)c->coef.p, 0, (const UnitDev*)P.d_units.p, (const XTile*)P.d_ixtiles.p,
                       P.ign, P.lds_inverse, P.ifast, P.lds_fast, d_out, bad);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "inverse launch");
}

// wc_inverse_coarse (packed_cap NULL) and wc_inverse_packed_coarse.
int inverse_coarse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* d_out,
                   const uint64_t* packed_cap) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !reduce || !out_units || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if (packed_cap && (rc = validate_pack(c, units, n))) return rc;
    std::vector<int32_t> ones;
    levels = levels_or_ones(levels, n, ones);
    if ((rc = validate_levels(c, units, n, levels)) || (rc = validate_coarse(c, units, n, levels, reduce, out_units)))
        return rc;
    if (std::all_of(reduce, reduce + n, [](int32_t r) { return r == 0; }))
        return packed_cap ? inverse_dense(c, d_payload, d_offsets, out_units, n, levels, d_out, packed_cap)
                          : wc_inverse_levels(c, d_payload, d_offsets, out_units, n, levels, d_out);
    std::vector<RegionDesc>& desc = c->cdesc;
    desc.resize(n);
    for (int u = 0; u < n; ++u) {
        RegionDesc& d = desc[u];
        compact_desc(d, units[u], out_units[u], levels[u], reduce[u]);
        // valid for odd dimensions (L = 1, r = 0), which region_end is not; 0 for a unit without cells
        if (d.W && d.H && d.D) d.end = (uint32_t)((((uint64_t)d.w - 1) * d.H + ((uint64_t)d.h - 1)) * d.D + d.d);
    }
    return inverse_compact(c, d_payload, d_offsets, units, n, out_units, d_out, desc, true, packed_cap);
}

// wc_inverse_region (packed_cap NULL) and wc_inverse_packed_region.
int inverse_region(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const int32_t* reduce, const wc_region* regions, const wc_unit* out_units,
                   float* d_out, const uint64_t* packed_cap) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !regions || !out_units || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if (packed_cap && (rc = validate_pack(c, units, n))) return rc;
    std::vector<int32_t> ones, zeros;
    levels = levels_or_ones(levels, n, ones);
    if (!reduce) {
        zeros.assign(n, 0);
        reduce = zeros.data();
    }
    if ((rc = validate_levels(c, units, n, levels)) ||
        (rc = validate_region(c, units, n, levels, reduce, regions, out_units)))
        return rc;
    std::vector<RegionDesc>& desc = c->cdesc;
    desc.resize(n);
    for (int u = 0; u < n; ++u) {
        RegionDesc& d = desc[u];
        compact_desc(d, units[u], out_units[u], levels[u], reduce[u]);
        if (!(d.W && d.H && d.D)) continue;  // end = 0
        const wc_region& g = regions[u];
        const int r = reduce[u];
        d.ox = (uint32_t)(g.x0 >> r);
        d.oy = (uint32_t)(g.y0 >> r);
        d.oz = (uint32_t)(g.z0 >> r);
        d.end = (uint32_t)region_end(d.w, d.h, d.d, d.L, d.ox, d.oy, d.oz, d.sx, d.sy, d.sz, (uint32_t)d.H,
                                     (uint32_t)d.D);  // <= W*H*D < 2^31; 0: a region without cells
    }
    return inverse_compact(c, d_payload, d_offsets, units, n, out_units, d_out, desc, false, packed_cap);
}

}  // namespace

extern "C" {

// Reduced-resolution inverse: every unit's region is its whole primed box
// (inverse_compact, wc_region.hip).
int wc_inverse_coarse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* d_out) {
    return inverse_coarse(c, d_payload, d_offsets, units, n, levels, reduce, out_units, d_out, nullptr);
}

// Sub-box inverse (inverse_compact, wc_region.hip).
int wc_inverse_region(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_region* regions, const wc_unit* out_units,
                      float* d_out) {
    return inverse_region(c, d_payload, d_offsets, units, n, levels, reduce, regions, out_units, d_out, nullptr);
}

}  // extern "C"

namespace wc {

// What every pass over a unit's pairs needs of it (wc_thin.hip, wc_layers.hip): the box, the header's
// ncoeff field, N and L; its select is one workgroup's until the caller splits it.
static ThinDesc thin_desc(const wc_unit& f, int L) {
    const uint64_t N = (uint64_t)f.nx * f.ny * f.nz;
    ThinDesc d{};
    d.W = f.nx;
    d.H = f.ny;
    d.D = f.nz;
    d.want = L >= 2 ? -L : (int32_t)N;
    d.N = (uint32_t)N;
    d.L = (uint32_t)L;
    d.slot = kLtSolo;
    return d;
}

// Thinning in the compressed domain (wc_thin.hip).  The plan of the units (dense,
// without cell offsets: the one wc_inverse_region's decode uses) gives the pair
// tiles and their look-back granules; the call's descriptors and split layout go
// through the pinned block.  Everything of wc_ctx::thin is sized and grown here,
// before the first launch; the state words are cleared on the stream.
// With `so` the call is a split: the same descriptors, plan, scratch and launch, with the rest's slots
// (wc_forward's layout), its count words and 4 B per coefficient more for the rest's positions.
static int thin_or_split(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                         const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots,
                         uint8_t* d_out, uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_kept,
                         float* d_thresh, uint32_t* d_key, const SplitOut* so, const double* tol = nullptr,
                         double* d_bound = nullptr) {
    const bool budget = max_pairs != nullptr;
    int rc;
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    // the tolerance form: what wc_forward_levels_tol refuses (an odd dimension passes validate_levels only at L = 1)
    if (tol && (rc = validate_tol(c, units, n, tol))) return rc;
    int maxl = 1;
    std::vector<ThinDesc> desc(n);
    uint64_t cursor = 4, rcursor = 4;
    for (int u = 0; u < n; ++u) {
        const wc_unit& f = units[u];
        const int L = levels[u];
        ThinDesc& d = desc[u];
        d = thin_desc(f, L);
        const uint64_t N = d.N;
        if (so) {
            d.rest_off = rcursor;
            rcursor += 24 + 8 * N;
        }
        d.dmagic = N ? rows_magic(f.nz) : 0;
        d.hmagic = N ? rows_magic(f.ny) : 0;
        d.K = budget ? max_pairs[u] : 0u;
        d.cap = budget && !full_slots ? (uint32_t)std::min<uint64_t>(d.K, N) : (uint32_t)N;
        maxl = std::max(maxl, L);
        if (tol) d.tol = tol[u];
        for (int l = 0; l < L && !budget && !tol; ++l) {
            d.th[l] = thresh[(size_t)u * WC_MAX_LEVELS + l];
            if (!(d.th[l] >= 0.0f))
                return fail(c, WC_ERR_INVALID,
                            "unit " + std::to_string(u) + ": threshold of level " + std::to_string(l + 1) +
                                " is NaN or negative");
        }
        d.out_off = cursor;
        cursor += 24 + 8ull * d.cap;
    }
    if (out_capacity < cursor) return fail(c, WC_ERR_INVALID, "out_capacity < wc_thin_bound");
    if (so && so->capacity < rcursor) return fail(c, WC_ERR_INVALID, "rest_capacity < wc_split_bound");
    {  // the input's length is not known here: what can be seen is its start inside the output's extent
        const uintptr_t a0 = (uintptr_t)d_payload, a1 = a0 + 24, b0 = (uintptr_t)d_out, b1 = b0 + cursor;
        if (a0 < b1 && b0 < a1) return fail(c, WC_ERR_INVALID, "out overlaps the payload buffer");
        if (so) {
            const uintptr_t r0 = (uintptr_t)so->d_rest, r1 = r0 + rcursor;
            if (a0 < r1 && r0 < a1) return fail(c, WC_ERR_INVALID, "rest overlaps the payload buffer");
            if (b0 < r1 && r0 < b1) return fail(c, WC_ERR_INVALID, "base and rest overlap");
        }
    }
    if (so && ((rc = check_aligned(c, so->d_rest, "rest")) || (rc = check_aligned(c, so->d_offsets, "rest_offsets", 8)) ||
               (rc = check_aligned(c, so->d_pairs, "rest_pairs", 4))))
        return rc;
    if ((rc = check_aligned(c, d_payload, "payload")) || (rc = check_aligned(c, d_offsets, "offsets", 8)) ||
        (rc = check_aligned(c, d_out, "out")) || (rc = check_aligned(c, d_out_offsets, "out_offsets", 8)) ||
        (rc = check_aligned(c, d_kept, "kept", 4)) || (rc = check_aligned(c, d_thresh, "thresh", 4)) ||
        (rc = check_aligned(c, d_key, "key", 4)) || (rc = check_aligned(c, d_bound, "bound", 8)))
        return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = dense_plan(c, units, n, true))) return rc;  // every unit's pair tiles in dtiles
    const Plan& P = c->plan;
    // as build_leveltol: a unit of more than opt_tol_solo tiles is split into runs of `chunk` tiles
    const uint32_t solo = (uint32_t)c->opt_tol_solo, chunk = std::min<uint32_t>(solo, 8);
    std::vector<uint32_t> split;
    std::vector<uint2> items;
    uint64_t tiles = 0;
    for (int u = 0; u < n; ++u) {
        const UnitDev& d = P.units[u];
        desc[u].dt_begin = d.dt_begin;
        tiles += d.ndt;
        if (!(budget || tol) || d.ndt <= solo) continue;
        desc[u].slot = (uint32_t)split.size();
        split.push_back((uint32_t)u);
        for (uint32_t t = 0; t < d.ndt; t += chunk) items.push_back(make_uint2((uint32_t)u, t));
    }
    const size_t nsplit = split.size(), nitems = items.size();
    // the pinned blob: ThinDesc[n] | items[nitems] | split_units[nsplit]
    const size_t o_items = sizeof(ThinDesc) * n, o_split = o_items + sizeof(uint2) * nitems,
                 in_bytes = o_split + 4 * nsplit;
    // wc_ctx::thin: [ticket[2][n] | keptw[n] | keyw[n] | (a split) restw[n] | status[2][tiles]] (cleared) |
    //               state[nsplit] | thresh[n][4] | gbins[nsplit][4352, tolerance form: kThinTolBinStride] |
    //               s2[tiles * kFlatTile] | s1[tiles * kFlatTile] | (a split) s3[tiles * kFlatTile]
    const size_t o_status = round_up((so ? 20ull : 16ull) * n, 8), clear_bytes = o_status + 16ull * tiles,
                 o_state = round_up(clear_bytes, 16), o_th = o_state + sizeof(BudgetState) * nsplit,
                 o_bins = o_th + sizeof(float) * WC_MAX_LEVELS * n, o_s2 = o_bins + 4ull * (tol ? kThinTolBinStride : 4352) * nsplit,
                 o_s1 = round_up(o_s2 + 4ull * kFlatTile * tiles, 16), o_s3 = o_s1 + 8ull * kFlatTile * tiles,
                 total = o_s3 + (so ? 4ull * kFlatTile * tiles : 0);
    uint8_t* pin = nullptr;
    if ((rc = ensure(c, c->thin, total)) || (rc = pin_begin(c, in_bytes, in_bytes, &pin))) return rc;
    std::memcpy(pin, desc.data(), sizeof(ThinDesc) * n);
    if (nitems) std::memcpy(pin + o_items, items.data(), sizeof(uint2) * nitems);
    if (nsplit) std::memcpy(pin + o_split, split.data(), 4 * nsplit);
    if ((rc = pin_upload(c, in_bytes))) return rc;
    uint8_t* s = (uint8_t*)c->thin.p;
    const uint8_t* blob = (const uint8_t*)c->tol_in.p;
    hipError_t e = hipMemsetAsync(s, 0, clear_bytes, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "memset");
    ThinLaunch a{};
    a.desc = (const ThinDesc*)blob;
    a.n = n;
    a.tiles = (const FTile*)P.d_dtiles.p;
    a.ntiles = (uint32_t)P.dtiles.size();
    a.payload = d_payload;
    a.offsets = d_offsets;
    a.budget = budget;
    a.tol = tol != nullptr;
    a.maxl = maxl;
    a.bound = d_bound;
    a.ordered = tile_order(c);
    a.ticket[0] = (uint32_t*)s;
    a.ticket[1] = (uint32_t*)s + n;
    a.keptw = (uint32_t*)s + 2 * (size_t)n;
    a.keyw = (uint32_t*)s + 3 * (size_t)n;
    a.status[0] = (unsigned long long*)(s + o_status);
    a.status[1] = a.status[0] + tiles;
    a.state = (BudgetState*)(s + o_state);
    a.thresh = d_thresh ? d_thresh : (float*)(s + o_th);
    a.key_out = d_key;
    a.gbins = (uint32_t*)(s + o_bins);
    a.s2 = (uint32_t*)(s + o_s2);
    a.s1 = (uint2*)(s + o_s1);
    a.items = (const uint2*)(blob + o_items);
    a.nitems = (uint32_t)nitems;
    a.chunk = chunk;
    a.split_units = (const uint32_t*)(blob + o_split);
    a.nsplit = (uint32_t)nsplit;
    a.out = d_out;
    a.out_offsets = d_out_offsets;
    a.kept = d_kept;
    a.err = (uint32_t*)c->errflag.p;
    if (so) {
        a.rest = so->d_rest;
        a.rest_offsets = so->d_offsets;
        a.rest_pairs = so->d_pairs;
        a.s3 = (uint32_t*)(s + o_s3);
        a.restw = (uint32_t*)s + 4 * (size_t)n;
    }
    StageTimer t(c, WC_STAGE_TOL);
    if ((e = launch_thin(c->stream, a)) != hipSuccess) return hip_fail(c, e, so ? "split launch" : "thin launch");
    c->err_check_pending = true;  // malformed payloads surface at the next wc_synchronize
    return WC_OK;
}

int thin_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_out,
                uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    return thin_or_split(c, d_payload, d_offsets, units, n, levels, max_pairs, thresh, full_slots, d_out, out_capacity,
                         d_out_offsets, d_kept, d_thresh, d_key, nullptr);
}

int split_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                 const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_base,
                 uint64_t base_capacity, uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest,
                 float* d_thresh, uint32_t* d_key) {
    return thin_or_split(c, d_payload, d_offsets, units, n, levels, max_pairs, thresh, full_slots, d_base, base_capacity,
                         d_base_offsets, d_kept, d_thresh, d_key, &rest);
}

int thin_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const double* tol, uint8_t* d_out, uint64_t out_capacity,
                    uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    return thin_or_split(c, d_payload, d_offsets, units, n, levels, nullptr, nullptr, true, d_out, out_capacity,
                         d_out_offsets, d_kept, d_thresh, nullptr, nullptr, tol, d_bound);
}

int split_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                     const int32_t* levels, const double* tol, uint8_t* d_base, uint64_t base_capacity,
                     uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest, float* d_thresh,
                     double* d_bound) {
    return thin_or_split(c, d_payload, d_offsets, units, n, levels, nullptr, nullptr, true, d_base, base_capacity,
                         d_base_offsets, d_kept, d_thresh, nullptr, &rest, tol, d_bound);
}

// wc_merge (wc_layers.hip).  The dense plan of the units gives the pair tiles of either input; the
// descriptors go through the pinned block; wc_ctx::merge is sized and grown here, before the first launch.
int merge_device(wc_ctx* c, const uint8_t* d_a, const uint64_t* d_a_offsets, const uint8_t* d_b,
                 const uint64_t* d_b_offsets, const wc_unit* units, int n, const int32_t* levels, uint8_t* d_out,
                 uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_pairs) {
    int rc;
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    std::vector<ThinDesc> desc(n);
    uint64_t cursor = 4;
    for (int u = 0; u < n; ++u) {
        ThinDesc& d = desc[u];
        d = thin_desc(units[u], levels[u]);
        d.cap = d.N;
        d.out_off = cursor;
        cursor += 24 + 8ull * d.N;
    }
    if (out_capacity < cursor) return fail(c, WC_ERR_INVALID, "out_capacity < wc_merge_bound");
    for (const uint8_t* in : {d_a, d_b}) {  // an input's length is not known here: its start inside the output's extent
        const uintptr_t a0 = (uintptr_t)in, a1 = a0 + 24, b0 = (uintptr_t)d_out, b1 = b0 + cursor;
        if (a0 < b1 && b0 < a1) return fail(c, WC_ERR_INVALID, "out overlaps an input buffer");
    }
    if ((rc = check_aligned(c, d_a, "a")) || (rc = check_aligned(c, d_a_offsets, "a_offsets", 8)) ||
        (rc = check_aligned(c, d_b, "b")) || (rc = check_aligned(c, d_b_offsets, "b_offsets", 8)) ||
        (rc = check_aligned(c, d_out, "out")) || (rc = check_aligned(c, d_out_offsets, "out_offsets", 8)) ||
        (rc = check_aligned(c, d_pairs, "pairs", 4)))
        return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = dense_plan(c, units, n, true))) return rc;  // every unit's pair tiles in dtiles
    const Plan& P = c->plan;
    uint64_t tiles = 0;
    for (int u = 0; u < n; ++u) {
        desc[u].dt_begin = P.units[u].dt_begin;
        tiles += P.units[u].ndt;
    }
    // wc_ctx::merge: [ticket[2][n] | live[2][n] | overlap[n] | status[2][tiles]] (cleared) | pos[2][tiles * kFlatTile]
    const size_t o_status = round_up(20ull * n, 8), clear_bytes = round_up(o_status + 16ull * tiles, 16),
                 total = clear_bytes + 8ull * kFlatTile * tiles, in_bytes = sizeof(ThinDesc) * n;
    uint8_t* pin = nullptr;
    if ((rc = ensure(c, c->merge, total)) || (rc = pin_begin(c, in_bytes, in_bytes, &pin))) return rc;
    std::memcpy(pin, desc.data(), in_bytes);
    if ((rc = pin_upload(c, in_bytes))) return rc;
    uint8_t* s = (uint8_t*)c->merge.p;
    hipError_t e = hipMemsetAsync(s, 0, clear_bytes, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "memset");
    MergeLaunch a{};
    a.desc = (const ThinDesc*)c->tol_in.p;
    a.n = n;
    a.tiles = (const FTile*)P.d_dtiles.p;
    a.ntiles = (uint32_t)P.dtiles.size();
    a.pay[0] = d_a;
    a.pay[1] = d_b;
    a.off[0] = d_a_offsets;
    a.off[1] = d_b_offsets;
    a.ordered = tile_order(c);
    a.ticket[0] = (uint32_t*)s;
    a.ticket[1] = (uint32_t*)s + n;
    a.live = (uint32_t*)s + 2 * (size_t)n;
    a.overlap = (uint32_t*)s + 4 * (size_t)n;
    a.status[0] = (unsigned long long*)(s + o_status);
    a.status[1] = a.status[0] + tiles;
    a.pos[0] = (uint32_t*)(s + clear_bytes);
    a.pos[1] = a.pos[0] + (size_t)kFlatTile * tiles;
    a.out = d_out;
    a.out_offsets = d_out_offsets;
    a.pairs = d_pairs;
    a.err = (uint32_t*)c->errflag.p;
    StageTimer t(c, WC_STAGE_TOL);
    if ((e = launch_merge(c->stream, a)) != hipSuccess) return hip_fail(c, e, "merge launch");
    c->err_check_pending = true;  // malformed payloads and overlaps surface at the next wc_synchronize
    return WC_OK;
}

}  // namespace wc

extern "C" {

uint64_t wc_thin_bound(const wc_unit* units, int n, const uint32_t* max_pairs) {
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) {
        const uint64_t N = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        b += 24 + 8 * (max_pairs ? std::min<uint64_t>(max_pairs[i], N) : N);
    }
    return b;
}

int wc_thin_budget(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_out, uint64_t out_capacity,
                   uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !max_pairs || !d_out || !d_out_offsets || !d_kept)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return thin_device(c, d_payload, d_offsets, units, n, levels, max_pairs, nullptr, false, d_out, out_capacity,
                       d_out_offsets, d_kept, d_thresh, d_key);
}

// Progressive layers (wc_thin.hip's split, wc_layers.hip's merge): a payload into (base, rest), and two payloads into their union.
int wc_split_budget(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_base, uint64_t base_capacity,
                    uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                    uint64_t* d_rest_offsets, uint32_t* d_rest_pairs, float* d_thresh, uint32_t* d_key) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !max_pairs || !d_base || !d_base_offsets || !d_kept || !d_rest ||
        !d_rest_offsets || !d_rest_pairs)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return split_device(c, d_payload, d_offsets, units, n, levels, max_pairs, nullptr, false, d_base, base_capacity,
                        d_base_offsets, d_kept, SplitOut{d_rest, rest_capacity, d_rest_offsets, d_rest_pairs}, d_thresh,
                        d_key);
}

int wc_split_thresh(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const float* thresh, uint8_t* d_base, uint64_t base_capacity,
                    uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                    uint64_t* d_rest_offsets, uint32_t* d_rest_pairs) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !thresh || !d_base || !d_base_offsets || !d_kept || !d_rest ||
        !d_rest_offsets || !d_rest_pairs)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return split_device(c, d_payload, d_offsets, units, n, levels, nullptr, thresh, false, d_base, base_capacity,
                        d_base_offsets, d_kept, SplitOut{d_rest, rest_capacity, d_rest_offsets, d_rest_pairs}, nullptr,
                        nullptr);
}

int wc_merge(wc_ctx* c, const uint8_t* d_a, const uint64_t* d_a_offsets, const uint8_t* d_b, const uint64_t* d_b_offsets,
             const wc_unit* units, int n, const int32_t* levels, uint8_t* d_out, uint64_t out_capacity,
             uint64_t* d_out_offsets, uint32_t* d_pairs) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_a || !d_a_offsets || !d_b || !d_b_offsets || !levels || !d_out || !d_out_offsets || !d_pairs)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return merge_device(c, d_a, d_a_offsets, d_b, d_b_offsets, units, n, levels, d_out, out_capacity, d_out_offsets,
                        d_pairs);
}

int wc_thin_thresh(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                   const int32_t* levels, const float* thresh, uint8_t* d_out, uint64_t out_capacity,
                   uint64_t* d_out_offsets, uint32_t* d_kept) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !thresh || !d_out || !d_out_offsets || !d_kept)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return thin_device(c, d_payload, d_offsets, units, n, levels, nullptr, thresh, false, d_out, out_capacity,
                       d_out_offsets, d_kept, nullptr, nullptr);
}

// The tolerance forms of the thinning and of the split (wc_thin.hip): T from wc_forward_levels_tol's rule
// on the pairs' bins.
int wc_thin_tol(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const double* tol, uint8_t* d_out, uint64_t out_capacity,
                uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !tol || !d_out || !d_out_offsets || !d_kept)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return thin_tol_device(c, d_payload, d_offsets, units, n, levels, tol, d_out, out_capacity, d_out_offsets, d_kept,
                           d_thresh, d_bound);
}

int wc_split_tol(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                 const int32_t* levels, const double* tol, uint8_t* d_base, uint64_t base_capacity,
                 uint64_t* d_base_offsets, uint32_t* d_kept, uint8_t* d_rest, uint64_t rest_capacity,
                 uint64_t* d_rest_offsets, uint32_t* d_rest_pairs, float* d_thresh, double* d_bound) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_payload || !d_offsets || !levels || !tol || !d_base || !d_base_offsets || !d_kept || !d_rest ||
        !d_rest_offsets || !d_rest_pairs)
        return fail(c, WC_ERR_INVALID, "null buffer");
    return split_tol_device(c, d_payload, d_offsets, units, n, levels, tol, d_base, base_capacity, d_base_offsets, d_kept,
                            SplitOut{d_rest, rest_capacity, d_rest_offsets, d_rest_pairs}, d_thresh, d_bound);
}

// The decoders over packed units (wc_packsrc.h): wc_unpack followed by
// wc_inverse_levels / wc_inverse_coarse / wc_inverse_region, bit for bit, without
// the standard payloads in between.  The full decode takes the dense path for
// every L (the row-indexed inverse reads pairs at random from a standard payload).
int wc_inverse_packed(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_packed_offsets, uint64_t packed_capacity,
                      const wc_unit* units, int n, const int32_t* levels, float* d_out) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (n == 0) return WC_OK;
    if (!d_packed || !d_packed_offsets || !d_out) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = validate_pack(c, units, n))) return rc;
    std::vector<int32_t> ones;
    levels = levels_or_ones(levels, n, ones);
    if ((rc = validate_levels(c, units, n, levels))) return rc;
    return inverse_dense(c, d_packed, d_packed_offsets, units, n, levels, d_out, &packed_capacity);
}

int wc_inverse_packed_coarse(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_packed_offsets,
                             uint64_t packed_capacity, const wc_unit* units, int n, const int32_t* levels,
                             const int32_t* reduce, const wc_unit* out_units, float* d_out) {
    return inverse_coarse(c, d_packed, d_packed_offsets, units, n, levels, reduce, out_units, d_out, &packed_capacity);
}

int wc_inverse_packed_region(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_packed_offsets,
                             uint64_t packed_capacity, const wc_unit* units, int n, const int32_t* levels,
                             const int32_t* reduce, const wc_region* regions, const wc_unit* out_units, float* d_out) {
    return inverse_region(c, d_packed, d_packed_offsets, units, n, levels, reduce, regions, out_units, d_out,
                          &packed_capacity);
}

int wc_rmse(wc_ctx* c, const void* d_orig, int dtype, const float* d_regen, const wc_unit* units, int n,
            double* d_rmse) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_orig || !d_regen || !d_rmse) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n)) || (rc = ensure_scratch(c))) return rc;
    Plan& P = c->plan;
    StageTimer t(c, WC_STAGE_RMSE);
    hipError_t e = launch_rmse(c->stream, d_orig, dtype, d_regen, (const UnitDev*)P.d_units.p, n,
                               (const FTile*)P.d_ftiles.p, (uint32_t)P.ftiles.size(), (double*)c->part.p, d_rmse);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "rmse launch");
}

int wc_maxerr(wc_ctx* c, const void* d_orig, int dtype, const float* d_regen, const wc_unit* units, int n,
              double* d_err) {
    if (!c) return WC_ERR_INVALID;
    int rc;
    if ((rc = validate_units(c, units, n))) return rc;
    if (dtype != WC_F32 && dtype != WC_F64) return fail(c, WC_ERR_INVALID, "dtype");
    if (n == 0) return WC_OK;
    if (!d_orig || !d_regen || !d_err) return fail(c, WC_ERR_INVALID, "null buffer");
    if ((rc = check_aligned(c, d_orig, "orig", dtype == WC_F64 ? 8 : 4)) ||
        (rc = check_aligned(c, d_regen, "regen", 4)) || (rc = check_aligned(c, d_err, "err", 8)))
        return rc;
    if ((rc = set_device(c)) || (rc = get_plan(c, units, n))) return rc;
    Plan& P = c->plan;
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(double) * n, c->stream);  // the atomic max starts from +0.0
    if (e != hipSuccess) return hip_fail(c, e, "memset err");
    StageTimer t(c, WC_STAGE_RMSE);
    e = launch_maxerr(c->stream, d_orig, dtype, d_regen, (const UnitDev*)P.d_units.p, (const FTile*)P.d_ftiles.p,
                      (uint32_t)P.ftiles.size(), d_err);
    return e == hipSuccess ? WC_OK : hip_fail(c, e, "maxerr launch");
}

int wc_profile_enable(wc_ctx* c, int on) {
    if (!c) return WC_ERR_INVALID;
    c->prof = on != 0;
    return WC_OK;
}

int wc_profile_read(wc_ctx* c, double* total_ms, uint32_t* launches, int nstages) {
    if (!c || nstages < 0 || (nstages > 0 && (!total_ms || !launches))) return WC_ERR_INVALID;
    for (int i = 0; i < nstages; ++i) {
        total_ms[i] = 0.0;
        launches[i] = 0;
    }
    int rc = WC_OK;
    if (!c->marks.empty()) {
        hipError_t e = hipEventSynchronize(c->marks.back().b);
        if (e != hipSuccess) rc = hip_fail(c, e, "hipEventSynchronize");
    }
    for (auto& m : c->marks) {
        float ms = 0.f;
        if (rc == WC_OK && m.stage < nstages && hipEventElapsedTime(&ms, m.a, m.b) == hipSuccess) {
            total_ms[m.stage] += ms;
            launches[m.stage] += 1;
        }
        c->ev_pool.push_back(m.a);
        c->ev_pool.push_back(m.b);
    }
    c->marks.clear();
    return rc;
}

}  // extern "C"
