// test_hostserial.cpp — the two serial host drivers (wc_hostserial.cpp) and every _host
// entry point built on them, on the CPU, for the ASan + UBSan build (`make hostserialsan`,
// run by tests/test_hostserial_san.py) over the fake HIP runtime of tests/cpp/fake_device.cpp.
// No GPU and no kernel: the device entry points the drivers call are restated here on the
// fake's wc_forward / wc_inverse (a unit keeps its first kept_of(unit) cells), and write
// recognisable per-unit values (100 + the unit's index in the whole batch, ...) into their
// threshold, bound and key outputs, so that a wrong `+ a` or stride of a driver shows.
// Every caller buffer is a heap block of exactly its documented size.
//
//   modes     each entry point at WC_OPT_HOST_CHUNK 0 (one run), 512 (about a unit per run)
//             and 1500 (mixed): the expected outputs, byte-identical across the three; the
//             packed end in offsets[n]; per-unit results at the unit's index; cells no unit
//             owns keep their sentinel; capacity exactly at the bound, and one byte less
//   failures  at chunk 512, every H2D, D2H, hipStreamSynchronize, launch_pack and device
//             step of the call made to fail in turn (the first run's and the last run's
//             among them): the return code, no allocation left after the context is gone,
//             and no copy still pending when the call returns (fake::pending_copies)
//   verdict   a unit the device refuses in a packed decoder fails the call with that run's
//             and the later runs' cells untouched
//   refusals  bad dtype before null buffer before the mode's checks before the capacity
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "fake_device.h"
#include "wc_ctx.h"

using namespace wc;

static int g_checks = 0, g_fail = 0;
#define CHECK(c, ...)                                                             \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(c)) {                                                               \
            if (++g_fail <= 40) {                                                 \
                std::fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
                std::fprintf(stderr, __VA_ARGS__);                                \
                std::fprintf(stderr, "\n");                                       \
            }                                                                     \
        }                                                                         \
    } while (0)

// ---- the batch --------------------------------------------------------------------------------------------
// 8x8x8, 16x8x8, 8x8x16, a unit without cells, a unit 5 cells after its predecessor's end, and one
// back-to-back with it.  Runs at chunk 512: [0] [1] [2] [3 4] [5]; at 1500: [0 1] [2 3 4] [5].
constexpr int N = 6;
static const wc_unit g_units[N] = {{0, 8, 8, 8, 0},    {512, 16, 8, 8, 0}, {1536, 8, 8, 16, 0},
                                   {2560, 0, 8, 8, 0}, {2565, 8, 8, 8, 0}, {3077, 8, 8, 8, 0}};
constexpr uint64_t EXT = 3589;
static const int32_t g_levels[N] = {2, 1, 2, 1, 2, 1};
static const int32_t g_ones[N] = {1, 1, 1, 1, 1, 1};
static const double g_tol[N] = {0.5, 1.5, 2.5, 3.5, 4.5, 5.5};
static const uint32_t g_pairs[N] = {40, 41, 42, 43, 44, 45};
static const int32_t g_reduce[N] = {1, 0, 2, 0, 1, 1};   // <= g_levels
static const int32_t g_reduce1[N] = {1, 0, 1, 0, 0, 1};  // <= 1 (the packed units carry L = 1)
static float g_cells32[EXT];
static double g_cells64[EXT];
static const int64_t kChunks[3] = {0, 512, 1500};

static uint64_t ncells(const wc_unit& u) { return (uint64_t)u.nx * u.ny * u.nz; }

static int gidx(const wc_unit& u) {
    for (int i = 0; i < N; ++i)
        if (g_units[i].cell_offset == u.cell_offset && g_units[i].nx == u.nx && g_units[i].ny == u.ny &&
            g_units[i].nz == u.nz)
            return i;
    return -1;
}

// ---- the device entry points, restated --------------------------------------------------------------------
static int g_arg_bad = 0;     // a restated entry point saw an argument that is not the unit's
static long g_steps = 0;      // device steps so far
static long g_step_fail = 0;  // the k-th next device step fails
static int g_refuse = -1;     // the packed decoders raise the header bit for this unit

static bool step_fails(wc_ctx* c) {
    ++g_steps;
    if (g_step_fail > 0 && --g_step_fail == 0) {
        fail(c, WC_ERR_HIP, "injected device step");
        return true;
    }
    return false;
}

// units[i] is unit gidx of the batch: the per-unit inputs must be that unit's
template <class T>
static void expect_args(const wc_unit* units, int n, const T* got, const T* want) {
    for (int i = 0; i < n; ++i) {
        const int g = gidx(units[i]);
        if (g < 0 || !got || std::memcmp(&got[i], &want[g], sizeof(T)) != 0) ++g_arg_bad;
    }
}

static const int32_t* g_want_levels = g_levels;
static const int32_t* g_want_reduce = g_reduce;  // nullptr: the call passes none

extern "C" {

int wc_forward_tol(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const double* tol,
                   uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh,
                   double* d_bound) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, tol, g_tol);
    for (int i = 0; i < n; ++i) {
        d_thresh[i] = 100.0f + (float)gidx(units[i]);
        d_bound[i] = 200.0 + gidx(units[i]);
    }
    return wc_forward(c, d_cells, dtype, units, n, 0.0, d_payload, cap, d_offsets, d_kept);
}

int wc_forward_levels(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n, const int32_t* levels,
                      double keep, const float*, uint8_t* d_payload, uint64_t cap, uint64_t* d_offsets,
                      uint32_t* d_kept) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_want_levels);
    return wc_forward(c, d_cells, dtype, units, n, keep, d_payload, cap, d_offsets, d_kept);
}

int wc_forward_levels_tol(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n,
                          const int32_t* levels, const double* tol, uint8_t* d_payload, uint64_t cap,
                          uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_want_levels);
    expect_args(units, n, tol, g_tol);
    for (int i = 0; i < n; ++i) {
        for (int l = 0; l < WC_MAX_LEVELS; ++l) d_thresh[(size_t)WC_MAX_LEVELS * i + l] = 100.0f + 10.0f * l + (float)gidx(units[i]);
        d_bound[i] = 200.0 + gidx(units[i]);
    }
    return wc_forward(c, d_cells, dtype, units, n, 0.0, d_payload, cap, d_offsets, d_kept);
}

int wc_forward_levels_budget(wc_ctx* c, const void* d_cells, int dtype, const wc_unit* units, int n,
                             const int32_t* levels, const uint32_t* max_pairs, uint8_t* d_payload, uint64_t cap,
                             uint64_t* d_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_want_levels);
    expect_args(units, n, max_pairs, g_pairs);
    for (int i = 0; i < n; ++i) {
        for (int l = 0; l < WC_MAX_LEVELS; ++l) d_thresh[(size_t)WC_MAX_LEVELS * i + l] = 100.0f + 10.0f * l + (float)gidx(units[i]);
        d_key[i] = 300u + (uint32_t)gidx(units[i]);
    }
    return wc_forward(c, d_cells, dtype, units, n, 0.0, d_payload, cap, d_offsets, d_kept);
}

int wc_inverse_levels(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, float* d_out) {
    if (step_fails(c)) return WC_ERR_HIP;
    // (the coarse shortcut passes the derived units, which the batch does not know)
    for (int i = 0; i < n; ++i)
        if (gidx(units[i]) >= 0 && levels[i] != g_want_levels[gidx(units[i])]) ++g_arg_bad;
    return wc_inverse(c, d_payload, d_offsets, units, n, d_out);
}

int wc_inverse_rmse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const void* d_orig, int dtype, float* d_out, double* d_rmse) {
    const int rc = wc_inverse(c, d_payload, d_offsets, units, n, d_out);
    return rc ? rc : wc_rmse(c, d_orig, dtype, d_out, units, n, d_rmse);
}

// the stand-in decode into a smaller box is the decode cut off at the box's cells
int wc_inverse_coarse(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* d_out) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_want_levels);
    expect_args(units, n, reduce, g_want_reduce);
    return wc_inverse(c, d_payload, d_offsets, out_units, n, d_out);
}

int wc_inverse_region(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                      const int32_t* levels, const int32_t* reduce, const wc_region* regions, const wc_unit* out_units,
                      float* d_out) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_want_levels);
    if (g_want_reduce) expect_args(units, n, reduce, g_want_reduce);
    else if (reduce) ++g_arg_bad;
    for (int i = 0; i < n; ++i)
        if (regions[i].nx != (ncells(units[i]) ? units[i].nx : 0)) ++g_arg_bad;  // the whole box of its unit
    return wc_inverse(c, d_payload, d_offsets, out_units, n, d_out);
}

// The packed decoders read the uploaded bytes below cap: unit by unit through wc_unpack_unit, then the
// stand-in decode into the out unit.  The verdict on a unit is the error word's header bit.
static int packed_decode(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_off, uint64_t cap, const wc_unit* units,
                         int n, const int32_t* levels, const wc_unit* out_units, float* d_out) {
    if (step_fails(c)) return WC_ERR_HIP;
    expect_args(units, n, levels, g_ones);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, WC_ERR_HIP, "fake: packed decode");
    for (int i = 0; i < n; ++i) {
        uint64_t len = 0;
        if ((d_off[i] & 7) != 4 || d_off[i] + 20 > cap || wc_packed_size(d_packed + d_off[i], cap - d_off[i], &len) != WC_OK ||
            d_off[i] + len > cap) {
            ++g_arg_bad;
            continue;
        }
        if (gidx(units[i]) == g_refuse) {
            *(uint32_t*)c->errflag.p |= kErrHeader;
            continue;
        }
        std::vector<uint8_t> pay(20 + 8 * ncells(units[i]));
        size_t w = 0;
        if (wc_unpack_unit(d_packed + d_off[i], len, pay.data(), pay.size(), &w) != WC_OK) {
            ++g_arg_bad;
            continue;
        }
        const uint64_t nc = ncells(out_units[i]);
        float* o = d_out + out_units[i].cell_offset;
        std::fill(o, o + nc, 0.0f);
        for (uint64_t k = 0; 20 + 8 * k < w && k < nc; ++k) std::memcpy(&o[k], pay.data() + 24 + 8 * k, 4);
    }
    c->err_check_pending = true;
    return WC_OK;
}

int wc_inverse_packed(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_off, uint64_t cap, const wc_unit* units, int n,
                      const int32_t* levels, float* d_out) {
    return packed_decode(c, d_packed, d_off, cap, units, n, levels, units, d_out);
}

int wc_inverse_packed_coarse(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_off, uint64_t cap, const wc_unit* units,
                             int n, const int32_t* levels, const int32_t* reduce, const wc_unit* out_units, float* d_out) {
    expect_args(units, n, reduce, g_reduce1);
    return packed_decode(c, d_packed, d_off, cap, units, n, levels, out_units, d_out);
}

int wc_inverse_packed_region(wc_ctx* c, const uint8_t* d_packed, const uint64_t* d_off, uint64_t cap, const wc_unit* units,
                             int n, const int32_t* levels, const int32_t* reduce, const wc_region*, const wc_unit* out_units,
                             float* d_out) {
    if (reduce) ++g_arg_bad;  // the test passes none
    return packed_decode(c, d_packed, d_off, cap, units, n, levels, out_units, d_out);
}

uint64_t wc_thin_bound(const wc_unit* units, int n, const uint32_t* max_pairs) {  // wc_capi.cpp's
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) b += 24 + 8 * (max_pairs ? std::min<uint64_t>(max_pairs[i], ncells(units[i])) : ncells(units[i]));
    return b;
}

}  // extern "C"

namespace {
std::vector<std::unique_ptr<std::vector<UnitDev>>> g_tabs;  // launch_pack reads thin_device's slots from these
}

namespace wc {
// wc_packhost.cpp's kernels: nothing here calls wc_pack / wc_unpack or their _host forms
hipError_t launch_pack_units(hipStream_t, const PackDesc*, const FTile*, uint32_t, const uint8_t*, const uint64_t*, int, int,
                             uint8_t*, uint64_t*, uint64_t*, uint32_t*) {
    std::abort();
}
hipError_t launch_unpack_units(hipStream_t, const PackDesc*, const FTile*, uint32_t, const uint8_t*, const uint64_t*,
                               uint64_t, int, uint8_t*, uint64_t*, uint32_t*, uint32_t*) {
    std::abort();
}
hipError_t launch_dense(hipStream_t, bool, int, const uint64_t*, const uint32_t*, const uint64_t*, const uint8_t*, uint64_t*,
                        uint8_t*) {
    std::abort();
}

// the thinning's device call, after the uploads: unit u through wc_thin_unit into its slot of wc_forward's layout
int thin_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_out,
                uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    if (step_fails(c)) return WC_ERR_HIP;
    if (!full_slots || out_capacity < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "fake: thin_device");
    expect_args(units, n, levels, g_ones);
    if (max_pairs) expect_args(units, n, max_pairs, g_pairs);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, WC_ERR_HIP, "fake: thin_device");
    g_tabs.emplace_back(new std::vector<UnitDev>(n));
    std::vector<UnitDev>& tab = *g_tabs.back();
    c->plan.d_units.p = tab.data();
    uint64_t slot = 4;
    for (int u = 0; u < n; ++u) {
        tab[u].pay_off = slot;
        const uint8_t* p = d_payload + d_offsets[u];
        int32_t nrle;
        std::memcpy(&nrle, p + 16, 4);
        size_t written = 0;
        uint32_t key = 0;
        float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
        const int rc = wc_thin_unit(p, 20 + 8ull * (uint64_t)nrle, max_pairs ? max_pairs + u : nullptr,
                                    thresh ? thresh + (size_t)WC_MAX_LEVELS * u : nullptr, d_out + slot,
                                    20 + 8 * ncells(units[u]), &written, &key, th);
        if (rc != WC_OK) return fail(c, rc, "fake: wc_thin_unit refused unit " + std::to_string(u));
        d_out_offsets[u] = slot;
        d_kept[u] = (uint32_t)((written - 20) / 8);
        if (d_key) d_key[u] = key;
        if (d_thresh) std::memcpy(d_thresh + (size_t)WC_MAX_LEVELS * u, th, sizeof th);
        slot += 24 + 8 * ncells(units[u]);
    }
    c->err_check_pending = true;
    return WC_OK;
}
}  // namespace wc

// ---- contexts and caller buffers --------------------------------------------------------------------------
static wc_ctx* make_ctx(int64_t chunk) {
    wc_ctx* c = new wc_ctx();
    c->device = 0;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) std::abort();
    c->stream = c->own;
    if (wc::ensure(c, c->errflag, 16) != WC_OK || hipMemset(c->errflag.p, 0, 16) != hipSuccess) std::abort();
    c->opt_host_chunk = chunk;
    return c;
}

static void destroy_ctx(wc_ctx* c) {
    (void)hipStreamSynchronize(c->stream);
    c->plan.d_units.p = nullptr;  // the fake's and this file's own tables
    for (wc::DevBuf* b : {&c->errflag, &c->h_cells, &c->h_payload, &c->h_packed, &c->h_offsets, &c->h_poff, &c->h_kept,
                          &c->h_out, &c->h_rmse, &c->h_thresh, &c->h_bound, &c->pk_off})
        if (b->p) (void)hipFree(b->p);
    (void)hipStreamDestroy(c->own);
    fake::release_context_tables(c);
    delete c;
    g_tabs.clear();
}

// a heap block of exactly `bytes`, filled with the sentinel
struct Block {
    std::unique_ptr<uint8_t[]> p;
    size_t bytes = 0;
    void fresh(size_t b) {
        bytes = b;
        p.reset(new uint8_t[b ? b : 1]);
        std::memset(p.get(), 0x5a, b);
    }
    template <class T>
    T* as() const {
        return (T*)p.get();
    }
    bool untouched(size_t lo, size_t hi) const {
        return std::all_of(p.get() + lo, p.get() + hi, [](uint8_t b) { return b == 0x5a; });
    }
};

static void append(std::vector<uint8_t>& v, const void* p, size_t n) {
    v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n);
}

// One entry point under test.  call(c, short_by) runs it on fresh output blocks with its capacity short_by
// bytes below the bound; verify checks the outputs of a successful call and returns them, concatenated.
struct Case {
    std::string name;
    bool has_cap;
    bool packs;  // launch_pack is part of a run
    int steps_per_run = 1;
    std::function<int(wc_ctx*, uint64_t)> call;
    std::function<std::vector<uint8_t>(const char*)> verify;
};

// ---- the forward family -----------------------------------------------------------------------------------
struct FwdOut {
    Block pay, off, kept, thresh, bound, key, rmse;
};

// offsets, kept and the units' bytes of a packed output against the stand-in codec's
static std::vector<uint8_t> verify_packed(const char* what, const Block& pay, const Block& off, const Block& kept,
                                          const std::function<std::vector<uint8_t>(int)>& want) {
    std::vector<uint8_t> all;
    uint64_t o = 4;
    const uint64_t* offs = off.as<uint64_t>();
    CHECK(pay.untouched(0, 4), "%s: the 4 bytes before the first unit", what);
    for (int i = 0; i < N; ++i) {
        const std::vector<uint8_t> w = want(i);
        CHECK(offs[i] == o, "%s unit %d: offset %llu, want %llu", what, i, (unsigned long long)offs[i], (unsigned long long)o);
        CHECK(20 + 8ull * kept.as<uint32_t>()[i] == w.size(), "%s unit %d: kept %u", what, i, kept.as<uint32_t>()[i]);
        const bool fits = offs[i] == o && o + w.size() <= pay.bytes;
        CHECK(fits && std::memcmp(pay.p.get() + o, w.data(), w.size()) == 0, "%s unit %d: bytes", what, i);
        if (fits) append(all, pay.p.get() + o, w.size());
        o += (i + 1 < N ? 24 : 20) + w.size() - 20;
    }
    CHECK(offs[N] == o, "%s: offsets[n] %llu is not the packed end %llu", what, (unsigned long long)offs[N], (unsigned long long)o);
    CHECK(pay.untouched((size_t)std::min<uint64_t>(o, pay.bytes), pay.bytes), "%s: bytes past the packed end", what);
    append(all, offs, off.bytes);
    append(all, kept.p.get(), kept.bytes);
    return all;
}

static Case forward_case(int mode, int dtype, bool with_rmse) {
    auto out = std::make_shared<FwdOut>();
    const void* cells = dtype == WC_F64 ? (const void*)g_cells64 : (const void*)g_cells32;
    static const char* names[4] = {"forward_tol_host", "forward_levels_host", "forward_levels_tol_host",
                                   "forward_levels_budget_host"};
    Case k;
    k.name = std::string(names[mode]) + (dtype == WC_F64 ? " f64" : " f32") + (with_rmse ? " rmse" : "");
    k.has_cap = true;
    k.packs = true;
    k.steps_per_run = with_rmse && mode >= 2 ? 2 : 1;  // the round trip's wc_inverse_levels
    const size_t tstride = mode == 0 ? 1 : WC_MAX_LEVELS;
    k.call = [=](wc_ctx* c, uint64_t short_by) {
        g_want_levels = g_levels;
        const uint64_t cap = wc_payload_bound(g_units, N) - short_by;
        out->pay.fresh(cap);
        out->off.fresh(8 * (N + 1));
        out->kept.fresh(4 * N);
        out->thresh.fresh(4 * tstride * N);
        out->bound.fresh(8 * N);
        out->key.fresh(4 * N);
        out->rmse.fresh(8 * N);
        double* rm = with_rmse ? out->rmse.as<double>() : nullptr;
        uint8_t* pay = out->pay.as<uint8_t>();
        uint64_t* off = out->off.as<uint64_t>();
        uint32_t* kept = out->kept.as<uint32_t>();
        switch (mode) {
            case 0:
                return wc_forward_tol_host(c, cells, dtype, g_units, N, g_tol, pay, cap, off, kept, out->thresh.as<float>(),
                                           out->bound.as<double>(), rm);
            case 1:
                return wc_forward_levels_host(c, cells, dtype, g_units, N, g_levels, 0.5, nullptr, pay, cap, off, kept);
            case 2:
                return wc_forward_levels_tol_host(c, cells, dtype, g_units, N, g_levels, g_tol, pay, cap, off, kept,
                                                  out->thresh.as<float>(), out->bound.as<double>(), rm);
            default:
                return wc_forward_levels_budget_host(c, cells, dtype, g_units, N, g_levels, g_pairs, pay, cap, off, kept,
                                                     out->thresh.as<float>(), out->key.as<uint32_t>(), rm);
        }
    };
    k.verify = [=](const char* what) {
        std::vector<uint8_t> all = verify_packed(what, out->pay, out->off, out->kept,
                                                 [&](int i) { return fake::payload_of(g_units[i], cells, dtype); });
        for (int i = 0; i < N && mode != 1; ++i) {
            for (size_t l = 0; l < tstride; ++l)
                CHECK(out->thresh.as<float>()[tstride * i + l] == 100.0f + 10.0f * l + i, "%s unit %d: thresh[%zu]", what, i, l);
            if (mode == 3) CHECK(out->key.as<uint32_t>()[i] == 300u + i, "%s unit %d: key", what, i);
            else CHECK(out->bound.as<double>()[i] == 200.0 + i, "%s unit %d: bound", what, i);
            if (with_rmse) {  // the stand-in drops the cells past kept_of: their root mean square
                double s = 0.0;
                for (uint64_t j = fake::kept_of(g_units[i]); j < ncells(g_units[i]); ++j) {
                    const float v = dtype == WC_F64 ? (float)g_cells64[g_units[i].cell_offset + j] : g_cells32[g_units[i].cell_offset + j];
                    s += (double)v * v;
                }
                const double want = ncells(g_units[i]) ? std::sqrt(s / (double)ncells(g_units[i])) : 0.0;
                CHECK(out->rmse.as<double>()[i] == want, "%s unit %d: rmse %g, want %g", what, i, out->rmse.as<double>()[i], want);
            }
        }
        if (mode == 1) CHECK(out->thresh.untouched(0, out->thresh.bytes), "%s: no thresholds asked for", what);
        if (!with_rmse) CHECK(out->rmse.untouched(0, out->rmse.bytes), "%s: no rmse asked for", what);
        append(all, out->thresh.p.get(), out->thresh.bytes);
        append(all, out->bound.p.get(), out->bound.bytes);
        append(all, out->key.p.get(), out->key.bytes);
        append(all, out->rmse.p.get(), out->rmse.bytes);
        return all;
    };
    return k;
}

// ---- the decoders -----------------------------------------------------------------------------------------
// The source of every decoder: the stand-in codec's payloads of the batch, unit u at an offset == 4 (mod 8)
// with a gap before it, as standard payloads and as packed units (4 value bytes: nothing is lost).
struct Source {
    std::unique_ptr<uint8_t[]> pay, packed;  // exactly to the last unit's end
    uint64_t off[N], poff[N];
};
static Source g_src;

static void make_source() {
    std::vector<std::vector<uint8_t>> p(N), q(N);
    uint64_t a = 4, b = 12;
    for (int i = 0; i < N; ++i) {
        p[i] = fake::payload_of(g_units[i], g_cells32, WC_F32);
        q[i].resize(p[i].size() + 64 + p[i].size() / 8);
        size_t w = 0;
        if (wc_pack_unit(p[i].data(), p[i].size(), 4, q[i].data(), q[i].size(), &w) != WC_OK) std::abort();
        q[i].resize(w);
        g_src.off[i] = a + 8 * (uint64_t)(i % 3);
        a = (g_src.off[i] + p[i].size() + 7) / 8 * 8 + 4;
        g_src.poff[i] = b + 16 * (uint64_t)(i % 2);
        b = (g_src.poff[i] + q[i].size() + 7) / 8 * 8 + 4;
    }
    const uint64_t pe = g_src.off[N - 1] + p[N - 1].size(), qe = g_src.poff[N - 1] + q[N - 1].size();
    g_src.pay.reset(new uint8_t[pe]);
    g_src.packed.reset(new uint8_t[qe]);
    std::memset(g_src.pay.get(), 0xa5, pe);
    std::memset(g_src.packed.get(), 0xa5, qe);
    for (int i = 0; i < N; ++i) {
        std::memcpy(g_src.pay.get() + g_src.off[i], p[i].data(), p[i].size());
        std::memcpy(g_src.packed.get() + g_src.poff[i], q[i].data(), q[i].size());
    }
}

// every cell of a decoder's output: a unit's first min(kept, cells) cells are the source's, its others 0,
// and cells no unit owns keep the sentinel; *owned_from: the first cell of unit `from` (verdict test)
static void verify_cells(const char* what, const Block& out, const wc_unit* ou, int upto = N) {
    std::vector<int> owner(out.bytes / 4, -1);
    for (int i = 0; i < N; ++i)
        for (uint64_t j = 0; j < ncells(ou[i]); ++j) owner[ou[i].cell_offset + j] = i;
    int bad = 0;
    for (size_t q = 0; q < owner.size(); ++q) {
        const int i = owner[q];
        if (i < 0 || i >= upto) {
            bad += !out.untouched(4 * q, 4 * q + 4);
            continue;
        }
        const uint64_t j = q - ou[i].cell_offset;
        const float want = j < fake::kept_of(g_units[i]) ? g_cells32[g_units[i].cell_offset + j] : 0.0f;
        bad += std::memcmp(out.p.get() + 4 * q, &want, 4) != 0;
    }
    CHECK(bad == 0, "%s: %d cells are not what the decode gives (or lost their sentinel)", what, bad);
}

enum Dec { InvLevels, InvLevelsHdr, Coarse, CoarseZero, Region, RegionNoReduce, Packed, PackedCoarse, PackedRegion };

static Case decoder_case(Dec d) {
    static const char* names[] = {"inverse_levels_host", "inverse_levels_host (levels from the headers)",
                                  "inverse_coarse_host", "inverse_coarse_host (reduce all 0)",
                                  "inverse_region_host", "inverse_region_host (no reduce)",
                                  "inverse_packed_host", "inverse_packed_coarse_host", "inverse_packed_region_host"};
    auto out = std::make_shared<Block>();
    auto ou = std::make_shared<std::vector<wc_unit>>(g_units, g_units + N);
    auto rg = std::make_shared<std::vector<wc_region>>(N);
    for (int i = 0; i < N; ++i) (*rg)[i] = ncells(g_units[i]) ? wc_region{0, 0, 0, g_units[i].nx, g_units[i].ny, g_units[i].nz} : wc_region{0, 0, 0, 0, 0, 0};
    static const int32_t zeros[N] = {0, 0, 0, 0, 0, 0};
    uint64_t ext = EXT;
    const int32_t* red = d == Coarse ? g_reduce : d == CoarseZero ? zeros : d == Region ? g_reduce : d == PackedCoarse ? g_reduce1 : nullptr;
    if (d == Coarse || d == CoarseZero || d == PackedCoarse) {
        if (wc_coarse_units(g_units, red, N, ou->data(), &ext) != WC_OK) std::abort();
    } else if (d == Region || d == RegionNoReduce || d == PackedRegion) {
        if (wc_region_units(g_units, rg->data(), red, N, ou->data(), &ext) != WC_OK) std::abort();
    }
    if (d == Coarse || d == Region) (*ou)[4].cell_offset += 3, (*ou)[5].cell_offset += 3, ext += 3;  // a gap here too
    Case k;
    k.name = names[d];
    k.has_cap = false;
    k.packs = false;
    k.call = [=](wc_ctx* c, uint64_t) {
        out->fresh(4 * ext);
        float* o = out->as<float>();
        g_want_levels = d == InvLevelsHdr ? g_ones : g_levels;
        g_want_reduce = d == Region || d == Coarse ? g_reduce : nullptr;
        const uint8_t* pay = g_src.pay.get();
        const uint8_t* pk = g_src.packed.get();
        switch (d) {
            case InvLevels: return wc_inverse_levels_host(c, pay, g_src.off, g_units, N, g_levels, o);
            case InvLevelsHdr: return wc_inverse_levels_host(c, pay, g_src.off, g_units, N, nullptr, o);
            case Coarse:
            case CoarseZero: return wc_inverse_coarse_host(c, pay, g_src.off, g_units, N, g_levels, red, ou->data(), o);
            case Region:
            case RegionNoReduce:
                return wc_inverse_region_host(c, pay, g_src.off, g_units, N, g_levels, red, rg->data(), ou->data(), o);
            case Packed: return wc_inverse_packed_host(c, pk, g_src.poff, g_units, N, d % 2 ? g_ones : nullptr, o);
            case PackedCoarse:
                return wc_inverse_packed_coarse_host(c, pk, g_src.poff, g_units, N, g_ones, red, ou->data(), o);
            default:
                return wc_inverse_packed_region_host(c, pk, g_src.poff, g_units, N, nullptr, nullptr, rg->data(), ou->data(), o);
        }
    };
    k.verify = [=](const char* what) {
        verify_cells(what, *out, ou->data());
        return std::vector<uint8_t>(out->p.get(), out->p.get() + out->bytes);
    };
    return k;
}

// ---- thinning ---------------------------------------------------------------------------------------------
static Case thin_case(bool budget) {
    auto out = std::make_shared<FwdOut>();
    auto th = std::make_shared<std::vector<float>>((size_t)N * WC_MAX_LEVELS, 0.0f);
    for (int i = 0; i < N; ++i) (*th)[(size_t)i * WC_MAX_LEVELS] = 10.0f + 9.0f * i;  // L = 1: one threshold per unit
    Case k;
    k.name = budget ? "thin_budget_host" : "thin_thresh_host";
    k.has_cap = true;
    k.packs = true;
    k.call = [=](wc_ctx* c, uint64_t short_by) {
        const uint64_t cap = wc_thin_bound(g_units, N, budget ? g_pairs : nullptr) - short_by;
        out->pay.fresh(cap);
        out->off.fresh(8 * (N + 1));
        out->kept.fresh(4 * N);
        out->thresh.fresh(4 * WC_MAX_LEVELS * N);
        out->key.fresh(4 * N);
        return budget ? wc_thin_budget_host(c, g_src.pay.get(), g_src.off, g_units, N, nullptr, g_pairs, out->pay.as<uint8_t>(),
                                            cap, out->off.as<uint64_t>(), out->kept.as<uint32_t>(), out->thresh.as<float>(),
                                            out->key.as<uint32_t>())
                      : wc_thin_thresh_host(c, g_src.pay.get(), g_src.off, g_units, N, g_ones, th->data(),
                                            out->pay.as<uint8_t>(), cap, out->off.as<uint64_t>(), out->kept.as<uint32_t>());
    };
    k.verify = [=](const char* what) {
        std::vector<uint32_t> key(N);
        std::vector<float> tl((size_t)N * WC_MAX_LEVELS, 0.0f);
        std::vector<uint8_t> all = verify_packed(what, out->pay, out->off, out->kept, [&](int i) {  // the rule, unit by unit
            const std::vector<uint8_t> p = fake::payload_of(g_units[i], g_cells32, WC_F32);
            std::vector<uint8_t> w(p.size());
            size_t n = 0;
            if (wc_thin_unit(p.data(), p.size(), budget ? &g_pairs[i] : nullptr, budget ? nullptr : &(*th)[(size_t)i * WC_MAX_LEVELS],
                             w.data(), w.size(), &n, &key[i], &tl[(size_t)i * WC_MAX_LEVELS]) != WC_OK)
                std::abort();
            w.resize(n);
            return w;
        });
        for (int i = 0; i < N && budget; ++i) {
            CHECK(out->key.as<uint32_t>()[i] == key[i], "%s unit %d: key", what, i);
            CHECK(std::memcmp(out->thresh.as<float>() + (size_t)i * WC_MAX_LEVELS, &tl[(size_t)i * WC_MAX_LEVELS], 4 * WC_MAX_LEVELS) == 0,
                  "%s unit %d: thresholds", what, i);
        }
        if (!budget) CHECK(out->thresh.untouched(0, out->thresh.bytes) && out->key.untouched(0, out->key.bytes), "%s: no results", what);
        append(all, out->thresh.p.get(), out->thresh.bytes);
        append(all, out->key.p.get(), out->key.bytes);
        return all;
    };
    return k;
}

// ---- the tests --------------------------------------------------------------------------------------------
static void test_modes(const Case& k) {
    std::vector<uint8_t> first;
    for (int64_t chunk : kChunks) {
        const std::string what = k.name + " chunk " + std::to_string(chunk);
        wc_ctx* c = make_ctx(chunk);
        g_arg_bad = 0;
        const long steps0 = g_steps;
        const int rc = k.call(c, 0);
        CHECK(rc == WC_OK, "%s: rc %d %s", what.c_str(), rc, c->err.c_str());
        CHECK(fake::pending_copies() == 0, "%s: a copy outlives the call", what.c_str());
        CHECK(g_arg_bad == 0, "%s: %d per-unit arguments are not their unit's", what.c_str(), g_arg_bad);
        CHECK(g_steps - steps0 == k.steps_per_run * (chunk == 0 ? 1 : chunk == 512 ? 5 : 3), "%s: %ld device steps", what.c_str(),
              g_steps - steps0);
        if (rc == WC_OK) {
            const std::vector<uint8_t> got = k.verify(what.c_str());
            if (chunk == 0) first = got;
            CHECK(got == first, "%s: the outputs differ from one run's", what.c_str());
        }
        if (k.has_cap) {
            const int r2 = k.call(c, 1);
            CHECK(r2 == WC_ERR_INVALID, "%s: one byte short gives %d", what.c_str(), r2);
            CHECK(fake::pending_copies() == 0, "%s: a copy outlives the refused call", what.c_str());
        }
        destroy_ctx(c);
    }
}

// every call of `api` the entry point makes at chunk 512, failed in turn
static void test_failures(const Case& k, const char* api) {
    const bool step = std::strcmp(api, "step") == 0;
    auto count = [&] { return step ? g_steps : fake::count(api); };
    const size_t live0 = fake::live_allocations();
    wc_ctx* c = make_ctx(512);
    (void)k.call(c, 0);  // the staging is there from here on: the counts below are the call's own
    long a = count();
    const int rc0 = k.call(c, 0);
    const long calls = count() - a;
    CHECK(rc0 == WC_OK && calls >= (std::strcmp(api, "launch_pack") || k.packs ? 1 : 0), "%s: %ld calls of %s", k.name.c_str(), calls, api);
    for (long j = 1; j <= calls; ++j) {
        if (step) g_step_fail = j;
        else fake::fail_nth(api, (int)j);
        a = count();
        const int rc = k.call(c, 0);
        const long made = count() - a;
        fake::clear_failures();
        g_step_fail = 0;
        CHECK(rc == WC_ERR_HIP, "%s: %s call %ld of %ld failed, rc %d", k.name.c_str(), api, j, calls, rc);
        // the drain is a synchronize itself: where the failed one was the call's last, nothing more could be done
        if (std::strcmp(api, "hipStreamSynchronize") != 0 || made > j)
            CHECK(fake::pending_copies() == 0, "%s: %s call %ld of %ld failed and a copy outlives the call", k.name.c_str(), api, j, calls);
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemset(c->errflag.p, 0, 16);
        c->err_check_pending = false;
    }
    const int rc = k.call(c, 0);  // and the context still works
    CHECK(rc == WC_OK, "%s after the %s failures: rc %d", k.name.c_str(), api, rc);
    if (rc == WC_OK) (void)k.verify((k.name + " after failures").c_str());
    destroy_ctx(c);
    CHECK(fake::live_allocations() == live0, "%s: %zu allocations left", k.name.c_str(), fake::live_allocations() - live0);
}

// a unit the device refuses in run r: WC_ERR_FORMAT, the earlier runs' cells there, that run's and the later ones' untouched
static void test_verdict() {
    for (int refuse : {0, 4, 5}) {
        wc_ctx* c = make_ctx(512);
        Block out;
        out.fresh(4 * EXT);
        g_refuse = refuse;
        const int rc = wc_inverse_packed_host(c, g_src.packed.get(), g_src.poff, g_units, N, nullptr, out.as<float>());
        g_refuse = -1;
        CHECK(rc == WC_ERR_FORMAT, "refused unit %d: rc %d", refuse, rc);
        CHECK(fake::pending_copies() == 0, "refused unit %d: a copy outlives the call", refuse);
        verify_cells("refused unit", out, g_units, refuse == 4 ? 3 : refuse);  // unit 4's run begins with unit 3
        destroy_ctx(c);
    }
}

static void test_refusals() {
    wc_ctx* c = make_ctx(0);
    const uint64_t cap = wc_payload_bound(g_units, N);
    Block pay, off, kept, cells;
    pay.fresh(cap);
    off.fresh(8 * (N + 1));
    kept.fresh(4 * N);
    cells.fresh(4 * EXT);
    uint8_t* P = pay.as<uint8_t>();
    uint64_t* O = off.as<uint64_t>();
    uint32_t* K = kept.as<uint32_t>();
    float* C = cells.as<float>();
    const int32_t badlv[N] = {2, 1, 9, 1, 2, 1};
    const double badtol[N] = {0.5, -1.0, 2.5, 3.5, 4.5, 5.5};
    wc_unit odd[N];
    std::copy(g_units, g_units + N, odd);
    odd[5].nz = 7;
    auto is = [&](int rc, int code, const char* msg) { return rc == code && c->err.find(msg) != std::string::npos; };
    // the forward family: dtype, null buffer, the mode's checks, capacity
    for (int m = 0; m < 4; ++m) {
        auto call = [&](int dtype, const void* cl, const int32_t* lv, const double* tol, const wc_unit* us, uint64_t cp) {
            switch (m) {
                case 0: return wc_forward_tol_host(c, cl, dtype, us, N, tol, P, cp, O, K, nullptr, nullptr, nullptr);
                case 1: return wc_forward_levels_host(c, cl, dtype, us, N, lv, 0.5, nullptr, P, cp, O, K);
                case 2: return wc_forward_levels_tol_host(c, cl, dtype, us, N, lv, tol, P, cp, O, K, nullptr, nullptr, nullptr);
                default: return wc_forward_levels_budget_host(c, cl, dtype, us, N, lv, g_pairs, P, cp, O, K, nullptr, nullptr, nullptr);
            }
        };
        CHECK(is(call(99, nullptr, badlv, badtol, g_units, 0), WC_ERR_INVALID, "dtype"), "forward %d: dtype first (%s)", m, c->err.c_str());
        CHECK(is(call(WC_F32, nullptr, badlv, badtol, g_units, 0), WC_ERR_INVALID, "null buffer"), "forward %d: null buffer (%s)", m, c->err.c_str());
        const char* msg = m == 0 ? "tolerance is negative or NaN" : "levels 9 outside 1..";
        CHECK(is(call(WC_F32, g_cells32, badlv, badtol, g_units, 0), WC_ERR_INVALID, msg), "forward %d: the mode's checks (%s)", m, c->err.c_str());
        if (m == 2) CHECK(is(call(WC_F32, g_cells32, g_levels, badtol, g_units, 0), WC_ERR_INVALID, "tolerance is negative or NaN"), "levels before tolerances (%s)", c->err.c_str());
        if (m == 3) CHECK(is(call(WC_F32, g_cells32, g_ones, g_tol, odd, 0), WC_ERR_INVALID, "the size-budget mode needs even W, H and D"), "budget (%s)", c->err.c_str());
        if (m == 0) CHECK(is(call(WC_F32, g_cells32, g_ones, g_tol, odd, 0), WC_ERR_INVALID, "the RMSE-tolerance mode needs even W, H and D"), "tol (%s)", c->err.c_str());
        CHECK(is(call(WC_F32, g_cells32, g_levels, g_tol, g_units, cap - 1), WC_ERR_INVALID, "payload_capacity < wc_payload_bound"), "forward %d: capacity (%s)", m, c->err.c_str());
    }
    // the decoders: null buffer before the mode's checks
    const int32_t badred[N] = {0, 0, 3, 0, 0, 0};
    std::vector<wc_region> rg(N);
    for (int i = 0; i < N; ++i) rg[i] = ncells(g_units[i]) ? wc_region{0, 0, 0, g_units[i].nx, g_units[i].ny, g_units[i].nz} : wc_region{0, 0, 0, 0, 0, 0};
    const uint8_t* S = g_src.pay.get();
    const uint8_t* Q = g_src.packed.get();
    CHECK(is(wc_inverse_levels_host(c, S, g_src.off, g_units, N, badlv, nullptr), WC_ERR_INVALID, "null buffer"), "inverse_levels: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_levels_host(c, S, g_src.off, g_units, N, badlv, C), WC_ERR_INVALID, "levels 9 outside"), "inverse_levels: levels (%s)", c->err.c_str());
    CHECK(is(wc_inverse_coarse_host(c, S, g_src.off, g_units, N, badlv, badred, g_units, nullptr), WC_ERR_INVALID, "null buffer"), "coarse: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_coarse_host(c, S, g_src.off, g_units, N, badlv, badred, g_units, C), WC_ERR_INVALID, "levels 9 outside"), "coarse: levels first (%s)", c->err.c_str());
    CHECK(is(wc_inverse_coarse_host(c, S, g_src.off, g_units, N, g_levels, badred, g_units, C), WC_ERR_INVALID, "reduce 3 outside 0..2"), "coarse: reduce (%s)", c->err.c_str());
    CHECK(is(wc_inverse_region_host(c, S, g_src.off, g_units, N, g_levels, badred, nullptr, g_units, C), WC_ERR_INVALID, "null buffer"), "region: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_region_host(c, S, g_src.off, g_units, N, g_levels, badred, rg.data(), g_units, C), WC_ERR_INVALID, "reduce 3 outside 0..2"), "region: reduce (%s)", c->err.c_str());
    uint64_t misaligned[N];
    std::copy(g_src.off, g_src.off + N, misaligned);
    misaligned[1] += 2;
    CHECK(is(wc_inverse_levels_host(c, S, misaligned, g_units, N, badlv, C), WC_ERR_INVALID, "offsets must be multiples of 4"), "offsets before levels (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_host(c, Q, g_src.poff, g_units, N, badlv, nullptr), WC_ERR_INVALID, "null buffer"), "packed: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_host(c, Q, g_src.poff, g_units, N, badlv, C), WC_ERR_INVALID, "levels 9 outside"), "packed: levels (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_host(c, Q, g_src.poff, g_units, N, g_levels, C), WC_ERR_FORMAT, "unit 0: malformed packed unit"), "packed: the tag's level (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_coarse_host(c, Q, g_src.poff, g_units, N, g_ones, nullptr, g_units, C), WC_ERR_INVALID, "null buffer"), "packed coarse: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_coarse_host(c, Q, g_src.poff, g_units, N, g_ones, badred, g_units, C), WC_ERR_INVALID, "reduce 3 outside 0..1"), "packed coarse: reduce (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_region_host(c, Q, g_src.poff, g_units, N, g_ones, badred, rg.data(), nullptr, C), WC_ERR_INVALID, "null buffer"), "packed region: null (%s)", c->err.c_str());
    CHECK(is(wc_inverse_packed_region_host(c, Q, g_src.poff, g_units, N, g_ones, badred, rg.data(), g_units, C), WC_ERR_INVALID, "reduce 3 outside 0..1"), "packed region: reduce (%s)", c->err.c_str());
    CHECK(cells.untouched(0, cells.bytes), "a refused decode wrote cells");
    // thinning: null buffer, the headers, the thresholds, capacity
    float nanth[N * WC_MAX_LEVELS] = {};
    nanth[2 * WC_MAX_LEVELS] = NAN;
    CHECK(is(wc_thin_budget_host(c, S, g_src.off, g_units, N, g_levels, nullptr, P, 0, O, K, nullptr, nullptr), WC_ERR_INVALID, "null buffer"), "thin budget: null (%s)", c->err.c_str());
    CHECK(is(wc_thin_thresh_host(c, S, g_src.off, g_units, N, g_levels, nullptr, P, 0, O, K), WC_ERR_INVALID, "null buffer"), "thin thresh: null (%s)", c->err.c_str());
    CHECK(is(wc_thin_budget_host(c, S, g_src.off, g_units, N, g_levels, g_pairs, P, 0, O, K, nullptr, nullptr), WC_ERR_FORMAT, "the payload header disagrees with the unit"), "thin: header before capacity (%s)", c->err.c_str());
    CHECK(is(wc_thin_thresh_host(c, S, g_src.off, g_units, N, nullptr, nanth, P, 0, O, K), WC_ERR_INVALID, "a threshold is NaN or negative"), "thin: thresholds before capacity (%s)", c->err.c_str());
    CHECK(is(wc_thin_budget_host(c, S, g_src.off, g_units, N, nullptr, g_pairs, P, wc_thin_bound(g_units, N, g_pairs) - 1, O, K, nullptr, nullptr), WC_ERR_INVALID, "out_capacity < wc_thin_bound"), "thin: capacity (%s)", c->err.c_str());
    CHECK(pay.untouched(0, pay.bytes) && off.untouched(0, off.bytes) && kept.untouched(0, kept.bytes), "a refused call wrote outputs");
    CHECK(fake::pending_copies() == 0, "a refused call left a copy");
    destroy_ctx(c);
}

int main() {
    for (uint64_t j = 0; j < EXT; ++j) {
        g_cells32[j] = 1.0f + 0.25f * (float)(j % 251) - (j % 7 == 0 ? 40.0f : 0.0f);
        g_cells64[j] = g_cells32[j];
    }
    make_source();
    std::vector<Case> cases;
    for (int mode = 0; mode < 4; ++mode) {
        cases.push_back(forward_case(mode, WC_F32, mode != 1));
        cases.push_back(forward_case(mode, WC_F64, false));
    }
    for (Dec d : {InvLevels, InvLevelsHdr, Coarse, CoarseZero, Region, RegionNoReduce, Packed, PackedCoarse, PackedRegion})
        cases.push_back(decoder_case(d));
    cases.push_back(thin_case(true));
    cases.push_back(thin_case(false));
    for (const Case& k : cases) test_modes(k);
    for (const Case& k : cases) {
        if (k.name.find("f64") != std::string::npos) continue;
        for (const char* api : {"H2D", "D2H", "hipStreamSynchronize", "launch_pack", "step"})
            if (std::strcmp(api, "launch_pack") != 0 || k.packs) test_failures(k, api);
    }
    test_verdict();
    test_refusals();
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
