// test_plan.cpp — the plan builder of the C-ABI (wavelet-compression_amd/csrc/
// wc_plan.cpp get_plan / ensure_scratch) on the CPU, over the fake HIP runtime
// of tests/cpp/fake_device.cpp, for the ASan/UBSan and TSan builds (`make asan`
// / `make tsan`, run by tests/test_sanitizers.py).  No GPU and no kernel: what
// runs is the host code that decides how the row-indexed inverse (wc_inverse.hip
// k_rowindex + k_inverse_rows, "K6r") tiles a unit and which workgroup gets
// which tile, under every value of the options that change it:
//   WC_OPT_RIX_LDS {1024, 2048, 9216, 16384} x WC_OPT_RIX_TX 0..5 x
//   WC_OPT_RIX_XCD {0, 1} x WC_OPT_INV_GROUPS {1, 3} (groups only without XCD).
//
// The two batches are the ones tests/test_gpu_rix_options.py runs on the device
// (same units, same cell offsets): one with generic units mixed in, one of
// fast-shape units only.  After each get_plan + ensure_scratch:
//   partition  every unit is exactly one of row-indexed / dense / empty; a
//              row-indexed unit's K6r tiles cover every (bx, by) block once;
//              tyv, bx0, by0 and the unit fields of every tile;
//   budget     4 rix_wr floats <= the budget; lds_rows is their maximum, <= 64 KB;
//   fallback   a fast unit is row-indexed exactly when 4 D + 80 <= budget
//              (2 x 2 x 232 is, 2 x 2 x 240 is not, at 1024);
//   addresses  the kernel's index arithmetic, restated from wc_inverse.hip and
//              bounded from the plan alone: every LDS float the zeroing, the
//              scatter and the synthesis touch lies inside lds_rows and inside the
//              range that was scattered; every row-index entry rix_load_range reads
//              is at most the unit's closing entry; the synthesis' stores write
//              every cell of the unit exactly once and nothing else; the RMSE
//              pass reads every cell of the unit exactly once;
//   order      nat is the tile's position in the unit-major list, inside its
//              unit's [rt_begin, rt_begin + nrt); the XCD list is the documented
//              permutation of that list; the group boundaries are consistent with
//              the tile lists; a unit's row-index tile t comes after t - 1; the
//              scratch holds 4 doubles per K6r tile, the row index, the granules;
//   mirrors    the uploaded tables equal the host vectors;
//   cache      more than 16 distinct plans of the same units, then the first
//              option set again: the same tile list as the first time.
// Failure messages name the option set and the unit.
//
// A third batch: the units with one long axis of tests/long_axis_shapes.py (kLong
// below: same dims, same cell offsets, and the class table of that file).  Its
// fast-shape units of at most 300 000 cells go through the same checks at
// WC_OPT_RIX_LDS {9216, 16384} (and 9200, where 4 D + 80 equals the budget for D =
// 2280) x WC_OPT_RIX_TX {0, 4, 5}; the fallback boundaries 2280 / 2288 and 4072 /
// 4080 and every unit's K6r tile shape are compared with the table.  The whole
// list, the 2^21-cell units included, is planned once for the forward's fields:
//   forward    fast, sparse, lbx / lby / lbz, ntx, net, et_begin, the emit class
//              (which launch a unit's emit blocks are in, each tile once, in
//              order) and the emit descriptor's copies of the unit fields;
//   dmagic     div_rows (wc_device.h) restated: floor(p / D) at p = q D - 1, q D
//              and q D + 1 for every row q of the unit, and at 2^31 - 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fake_device.h"
#include "wc_ctx.h"

// The five symbols of the .hip files wc_plan.cpp links: the two LDS formulas
// restated (wc_transform.hip), the persistent-grid sizes any constant.
namespace wc {
size_t transform_lds_bytes(int lbx, int lby, int lbz) {
    return (size_t)4 * (1 << lbx) * (1 << lby) * (2 * (1 << lbz) + 1) * sizeof(float);
}
size_t transform_fast_lds_bytes(int lbx, int lby, int lbz) {
    return (size_t)4 * (1 << lbx) * (1 << lby) * (2 * (1 << lbz) + 4) * sizeof(float);
}
uint32_t transform_hist_grid(size_t) { return 8; }
uint32_t transform_pf_grid(size_t) { return 8; }
uint32_t inverse_rows_grid(size_t) { return 8; }
}  // namespace wc

using namespace wc;

static int g_checks = 0, g_fail = 0;
#define CHECK(c, ...)                                                             \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(c)) {                                                               \
            if (++g_fail <= 60) {                                                 \
                std::fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
                std::fprintf(stderr, __VA_ARGS__);                                \
                std::fprintf(stderr, "\n");                                       \
            }                                                                     \
        }                                                                         \
    } while (0)

static wc_ctx* make_ctx() {
    wc_ctx* c = new wc_ctx();
    c->device = 0;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) std::abort();
    c->stream = c->own;
    if (wc::ensure(c, c->errflag, 16) != WC_OK || hipMemset(c->errflag.p, 0, 16) != hipSuccess) std::abort();
    return c;
}

static void destroy_ctx(wc_ctx* c) {
    (void)hipStreamSynchronize(c->stream);
    free_plan(c->plan);
    for (Plan& p : c->plan_cache) free_plan(p);
    for (DevBuf* b : {&c->errflag, &c->coef, &c->part, &c->state, &c->flags, &c->rowinfo, &c->npairs, &c->istate})
        if (b->p) (void)hipFree(b->p);
    (void)hipStreamDestroy(c->own);
    delete c;
}

// The batch of tests/test_gpu_rix_options.py (W, H, D), in its order, with its
// cell offsets: gaps of whole x-quads, every third unit one element past a
// quad, unit 8 two past.
static const int kDims[][3] = {
    {5, 4, 8},      // generic (odd W)
    {64, 2, 8},     // TX reaches 32, a single y block
    {66, 6, 8},     // hx 33, hy 3: edge tiles in both axes; W % 4 == 2: x-pair stores
    {6, 6, 4},      // generic (D % 8 != 0)
    {72, 10, 16},   // hx 36, W % 4 == 0: x-quad stores with a 4-block edge tile; hy 5
    {64, 2, 120},   // 120 pairs per range; TX 32 at 16384: 63 744 B of LDS
    {32, 32, 32},   // a cube at an odd offset: scalar stores
    {64, 8, 24},    // TY 4 at 16384, 2 at 9216 (RIX_TX 5)
    {8, 64, 8},     // tall in y, TY up to 32; offset == 2 (mod 4): 8-B stores
    {0, 4, 8},      // empty
    {2, 2, 232},    // the fallback boundary at 1024: row-indexed
    {2, 2, 240},    // ... and dense
    {16, 16, 64},   // a cube
    {32, 4, 8},     // (the device test's all-zero unit)
    {64, 2, 16},    // (the device test's single pair at the last flat position)
};
static constexpr int kUnits = (int)(sizeof(kDims) / sizeof(kDims[0]));

// The device test's second batch: the two generic units replaced by fast-shape
// ones of about their size, so that every unit with cells is row-indexed and
// wc_inverse_rmse fuses the RMSE into K6r (one generic unit sends the whole
// batch through the two-call path).
static const int kFastDims[2][3] = {{4, 4, 8}, {6, 6, 8}};  // in place of units 0 and 3
static const char* g_batch = "mixed batch";

static std::vector<wc_unit> make_units(bool fast_only) {
    std::vector<wc_unit> us;
    uint64_t cur = 0;
    for (int i = 0; i < kUnits; ++i) {
        const int* d = fast_only && i == 0 ? kFastDims[0] : fast_only && i == 3 ? kFastDims[1] : kDims[i];
        cur += 4 * (uint64_t)((i * 3) % 5);
        cur = (cur + 3) & ~3ull;
        if (i % 3 == 0) cur += 1;
        else if (i == 8) cur += 2;
        us.push_back(wc_unit{cur, d[0], d[1], d[2], 0});
        cur += (uint64_t)d[0] * d[1] * d[2];
    }
    return us;
}

struct Opt {
    int lds, tx, xcd, groups;
    std::string str() const {
        return std::string(g_batch) + ", RIX_LDS " + std::to_string(lds) + " RIX_TX " + std::to_string(tx) + " RIX_XCD " + std::to_string(xcd) +
               " INV_GROUPS " + std::to_string(groups);
    }
};

static std::string uname(const Plan& P, uint32_t u) {
    if (u >= P.units.size()) return "unit " + std::to_string(u) + " (not in the batch)";
    const UnitDev& d = P.units[u];
    return "unit " + std::to_string(u) + " (" + std::to_string(d.nx) + " x " + std::to_string(d.ny) + " x " +
           std::to_string(d.nz) + ")";
}

struct TileKey {
    uint32_t unit;
    int32_t bx0, by0, lbx, lby, tyv;
    uint32_t nat;
    bool operator==(const TileKey& o) const {
        return unit == o.unit && bx0 == o.bx0 && by0 == o.by0 && lbx == o.lbx && lby == o.lby && tyv == o.tyv && nat == o.nat;
    }
};
static std::vector<TileKey> tile_list(const Plan& P) {
    std::vector<TileKey> v;
    for (const RTile& r : P.rtiles) v.push_back(TileKey{r.unit, r.bx0, r.by0, r.lbx, r.lby, r.tyv, r.nat});
    return v;
}

// What the sweep saw of the kernel's branches (each must occur somewhere).
struct Seen {
    bool tx32 = false, tx1_aligned = false, edge_x = false, edge_y = false, quad = false, quad_edge = false,
         pair8 = false, scalar = false, fallback = false, lds_63744 = false, ty32 = false;
};

// One K6r tile: the index arithmetic of k_inverse_rows (wc_inverse.hip),
// restated, against the plan's LDS size and the unit's extent.  `wrote` /
// `read` count the synthesis' stores and the RMSE pass' loads per unit cell.
static void check_tile_addresses(const Plan& P, const RTile& T, const std::string& tag, std::vector<uint8_t>& wrote,
                                 std::vector<uint8_t>& read, Seen& seen) {
    const std::string w = tag + ", " + uname(P, T.unit) + " tile (" + std::to_string(T.bx0) + ", " +
                          std::to_string(T.by0) + ")";
    const char* what = w.c_str();
    const int64_t ldsf = (int64_t)(P.lds_rows / 4);  // floats of the launch's dynamic LDS
    const int TX = 1 << T.lbx, RS = rix_rs(T.lby, T.D), WR = rix_wr(T.lbx, T.lby, T.D);
    const int64_t rlen = (int64_t)T.tyv * T.D;
    const int64_t ncells = (int64_t)T.W * T.H * T.D;
    const int hx = T.W >> 1, hy = T.H >> 1, hz = T.D >> 1;
    const int txv = std::min(TX, hx - T.bx0);
    seen.tx32 |= TX == 32;
    seen.ty32 |= (1 << T.lby) == 32;
    seen.edge_x |= txv < TX;
    seen.edge_y |= T.tyv < (1 << T.lby);
    seen.tx1_aligned |= TX == 1 && (T.cell_off & 3) == 0 && (T.W & 3) == 0 && hx > 1;
    CHECK(RS % 4 == 0 && WR % 4 == 0, "%s: RS %d WR %d not 16-B multiples", what, RS, WR);
    CHECK(rlen <= RS, "%s: a range of %lld floats in a slot of %d", what, (long long)rlen, RS);

    // 1. zeroing and scatter: wave w's region [w WR, w WR + TX RS), range j's pairs at w WR + j RS + pos, pos < rlen
    for (int wv = 0; wv < 4; ++wv) {
        CHECK((int64_t)wv * WR + (int64_t)TX * RS <= ldsf, "%s: wave %d zeroes floats up to %lld of %lld", what, wv,
              (long long)wv * WR + (long long)TX * RS, (long long)ldsf);
        CHECK(wv == 3 || (int64_t)TX * RS <= WR, "%s: wave regions overlap", what);
        for (int j = 0; j < TX; ++j)
            CHECK((int64_t)wv * WR + (int64_t)j * RS + rlen - 1 < ldsf, "%s: scatter wave %d range %d reaches float %lld of %lld",
                  what, wv, j, (long long)wv * WR + (long long)j * RS + rlen - 1, (long long)ldsf);
    }

    // 2. rix_load_range: lane l < TX of wave w reads rowinfo[row_off + r0] and [row_off + r0 + tyv]
    for (int wv = 0; wv < 4; ++wv)
        for (int l = 0; l < 64; ++l) {
            if (l >= TX) continue;
            const int g = wv + 4 * l, bxl = g & (TX - 1), ssy = (g >> T.lbx) & 1, ssx = g >> (T.lbx + 1);
            CHECK(ssx <= 1, "%s: range %d has no sub-band", what, g);
            const int bx = T.bx0 + bxl;
            if (bx >= hx) continue;
            const uint64_t r0 = (uint64_t)(bx + ssx * hx) * T.H + T.by0 + ssy * hy;
            CHECK(r0 + T.tyv <= (uint64_t)T.W * T.H, "%s: range %d reads row entry %llu past the closing entry %llu", what,
                  g, (unsigned long long)(r0 + T.tyv), (unsigned long long)T.W * T.H);
            CHECK(T.row_off + r0 + T.tyv < P.rowinfo_entries, "%s: range %d reads past the batch's row index", what, g);
        }

    // 3. synthesis: sub-band reads from LDS, stores to the unit's cells
    const int64_t sy = T.W, sz = (int64_t)T.W * T.H;
    const int64_t lo = (int64_t)T.bx0 * 2;
    auto lds_read = [&](int x, int t3, int s2, int bxl, int byl, int bzb, int width) {
        const int g = ((x * 2 + t3) << T.lbx) + bxl;
        // the range rix_load_range gave that index: the same block column and sub-bands
        CHECK((g & (TX - 1)) == bxl && ((g >> T.lbx) & 1) == t3 && (g >> (T.lbx + 1)) == x, "%s: range %d is not (%d, %d, %d)",
              what, g, bxl, t3, x);
        const int64_t in = (int64_t)byl * T.D + s2 * hz + bzb;  // within the range: flat row byl, K = s2 hz + bz
        const int64_t idx = (int64_t)(g & 3) * WR + (int64_t)(g >> 2) * RS + in;
        CHECK(idx % width == 0, "%s: LDS read of %d floats at float %lld", what, width, (long long)idx);
        CHECK(idx + width - 1 < ldsf, "%s: LDS read reaches float %lld of %lld", what, (long long)idx + width - 1,
              (long long)ldsf);
        CHECK(in + width - 1 < rlen, "%s: LDS read reaches float %lld of a %lld-float range", what, (long long)in + width - 1,
              (long long)rlen);
    };
    auto store = [&](int64_t p, int width) {
        CHECK(((int64_t)T.cell_off + p) % width == 0, "%s: %d-cell store at element %lld", what, width,
              (long long)T.cell_off + (long long)p);
        for (int k = 0; k < width; ++k) {
            CHECK(p + k >= 0 && p + k < ncells, "%s: store to cell %lld of %lld", what, (long long)p + k, (long long)ncells);
            if (p + k >= 0 && p + k < ncells) ++wrote[(size_t)(p + k)];
        }
    };
    const bool f4 = TX >= 2 && ((T.cell_off & 3) == 0) && ((T.W & 3) == 0);
    if (f4) {
        seen.quad = true;
        seen.quad_edge |= txv < TX;
        const int nq = (TX >> 1) * T.tyv * (hz >> 1);
        for (int ci = 0; ci < nq; ++ci) {
            const int bp = ci & ((TX >> 1) - 1), rest = ci >> (T.lbx - 1);
            const int byl = rest % T.tyv, bq = rest / T.tyv;
            const int bxl = 2 * bp, by = T.by0 + byl, bzb = 2 * bq;
            if (T.bx0 + bxl >= hx) continue;
            CHECK(T.bx0 + bxl + 1 < hx, "%s: the x-quad's second block %d is past hx %d", what, T.bx0 + bxl + 1, hx);
            for (int e = 0; e < 2; ++e)
                for (int s2 = 0; s2 < 2; ++s2)
                    for (int t3 = 0; t3 < 2; ++t3)
                        for (int x = 0; x < 2; ++x) lds_read(x, t3, s2, bxl + e, byl, bzb, 2);
            for (int qb = 0; qb < 2; ++qb)
                for (int dz = 0; dz < 2; ++dz)
                    for (int dy = 0; dy < 2; ++dy)
                        store(lo + 2 * bxl + sy * (2 * by + dy) + sz * (2 * (bzb + qb) + dz), 4);
        }
    } else {
        const bool vout = (T.cell_off & 1) == 0;
        (vout ? seen.pair8 : seen.scalar) = true;
        const int ncol = TX * T.tyv * (hz >> 2);
        for (int ci = 0; ci < ncol; ++ci) {
            const int bxl = ci & (TX - 1), rest = ci >> T.lbx;
            const int byl = rest % T.tyv, bq = rest / T.tyv;
            const int bx = T.bx0 + bxl, by = T.by0 + byl, bzb = 4 * bq;
            if (bx >= hx) continue;
            for (int s2 = 0; s2 < 2; ++s2)
                for (int t3 = 0; t3 < 2; ++t3)
                    for (int x = 0; x < 2; ++x) lds_read(x, t3, s2, bxl, byl, bzb, 4);
            for (int qb = 0; qb < 4; ++qb)
                for (int dz = 0; dz < 2; ++dz)
                    for (int dy = 0; dy < 2; ++dy) {
                        const int64_t p = 2 * (int64_t)bx + sy * (2 * by + dy) + sz * (2 * (bzb + qb) + dz);
                        if (vout) {
                            store(p, 2);
                        } else {
                            store(p, 1);
                            store(p + 1, 1);
                        }
                    }
        }
    }

    // 4. the separate RMSE pass (fp32 originals, fp64 at an unaligned base, or a tile without x-quads)
    {
        const int ny2 = 2 * T.tyv;
        const uint32_t nc = (uint32_t)(T.D * ny2) << T.lbx;
        const int64_t lo2 = 2 * (int64_t)T.bx0 + 2 * (int64_t)T.by0 * sy;  // relative to cell_off
        for (uint32_t ci = 0; ci < nc; ++ci) {
            const int x = (int)(ci & (uint32_t)(TX - 1));
            if (x >= txv) continue;
            const uint32_t row = ci >> T.lbx;
            const int64_t i = lo2 + 2 * x + sy * (int64_t)(row % (uint32_t)ny2) + sz * (int64_t)(row / (uint32_t)ny2);
            CHECK(i >= 0 && i + 1 < ncells, "%s: RMSE pass reads cell %lld of %lld", what, (long long)i + 1, (long long)ncells);
            if (i >= 0 && i + 1 < ncells) {
                ++read[(size_t)i];
                ++read[(size_t)i + 1];
            }
        }
    }
}

static void check_plan(wc_ctx* c, const std::vector<wc_unit>& units, const Opt& o, Seen& seen) {
    const Plan& P = c->plan;
    const std::string tag = o.str();
    const char* t = tag.c_str();
    const int n = (int)units.size();
    CHECK((int)P.units.size() == n, "%s: %zu unit descriptors", t, P.units.size());
    if ((int)P.units.size() != n) return;

    // the unit-major tile list, built here from the unit's tile shape alone
    std::vector<TileKey> natural;
    size_t max_floats = 0;
    for (int i = 0; i < n; ++i) {
        const UnitDev& d = P.units[i];
        const std::string un = uname(P, (uint32_t)i);
        const bool fast = d.ncells && d.nx % 2 == 0 && d.ny % 2 == 0 && d.nz % 8 == 0;
        CHECK((d.fast != 0) == fast, "%s, %s: fast %d", t, un.c_str(), d.fast);
        // fallback boundary: 4 rix_wr(0, 0, D) = 4 ((D + 4) + 16) floats is the one-block tile
        const bool want_rix = fast && 4 * d.nz + 80 <= o.lds;
        CHECK((d.rix != 0) == want_rix, "%s, %s: rix %d, 4 D + 80 = %d", t, un.c_str(), d.rix, 4 * d.nz + 80);
        seen.fallback |= fast && !d.rix;
        if (!d.rix) continue;
        const size_t floats = 4 * (size_t)rix_wr(d.ilbx, d.ilby, d.nz);
        CHECK(floats <= (size_t)o.lds, "%s, %s: tile 2^%d x 2^%d needs %zu floats", t, un.c_str(), d.ilbx, d.ilby, floats);
        CHECK(d.ilbx >= 0 && d.ilbx <= o.tx && d.ilby >= 0, "%s, %s: tile 2^%d x 2^%d", t, un.c_str(), d.ilbx, d.ilby);
        // no wider than the unit (a tile of only invalid ranges would still cost its LDS)
        CHECK((1 << d.ilbx) < 2 * d.hx && (1 << d.ilby) < 2 * d.hy, "%s, %s: tile 2^%d x 2^%d for %d x %d blocks", t,
              un.c_str(), d.ilbx, d.ilby, d.hx, d.hy);
        max_floats = std::max(max_floats, floats);
        CHECK(d.rt_begin == natural.size(), "%s, %s: rt_begin %u, %zu tiles before it", t, un.c_str(), d.rt_begin,
              natural.size());
        for (int by = 0; by < d.hy; by += 1 << d.ilby)
            for (int bx = 0; bx < d.hx; bx += 1 << d.ilbx)
                natural.push_back(TileKey{(uint32_t)i, bx, by, d.ilbx, d.ilby, std::min(1 << d.ilby, d.hy - by),
                                          (uint32_t)natural.size()});
        CHECK(d.rt_begin + d.nrt == natural.size(), "%s, %s: nrt %u", t, un.c_str(), d.nrt);
    }
    CHECK(P.lds_rows == 4 * max_floats, "%s: lds_rows %zu, the largest tile needs %zu bytes", t, P.lds_rows, 4 * max_floats);
    CHECK(P.lds_rows <= 65536, "%s: lds_rows %zu", t, P.lds_rows);
    seen.lds_63744 |= P.lds_rows == 63744;

    // the K6r list: the natural list, or with XCD the documented permutation of it
    const size_t T = P.rtiles.size();
    CHECK(T == natural.size(), "%s: %zu K6r tiles, %zu expected", t, T, natural.size());
    if (T != natural.size()) return;
    const std::vector<TileKey> got = tile_list(P);
    std::vector<int> hits(T, 0);
    for (size_t p = 0; p < T; ++p) {
        const RTile& r = P.rtiles[p];
        const std::string un = uname(P, r.unit);
        CHECK(r.nat < T, "%s, %s: nat %u of %zu", t, un.c_str(), r.nat, T);
        if (r.nat >= T) continue;
        ++hits[r.nat];
        CHECK(got[p] == natural[r.nat], "%s, %s: list position %zu (nat %u) is tile (%d, %d), the unit-major list has unit %u (%d, %d)",
              t, un.c_str(), p, r.nat, r.bx0, r.by0, natural[r.nat].unit, natural[r.nat].bx0, natural[r.nat].by0);
        if (!o.xcd || T <= 8) CHECK(r.nat == p, "%s, %s: nat %u at list position %zu", t, un.c_str(), r.nat, p);
        if (r.unit >= (uint32_t)n) continue;
        const UnitDev& d = P.units[r.unit];
        CHECK(d.rix, "%s, %s: a K6r tile of a unit that is not row-indexed", t, un.c_str());
        CHECK(r.nat >= d.rt_begin && r.nat < d.rt_begin + d.nrt, "%s, %s: nat %u outside the unit's partial sums [%u, %u)", t,
              un.c_str(), r.nat, d.rt_begin, d.rt_begin + d.nrt);
        CHECK(r.W == d.nx && r.H == d.ny && r.D == d.nz && r.row_off == d.row_off && r.cell_off == d.cell_off,
              "%s, %s: tile fields %d x %d x %d row_off %llu cell_off %llu", t, un.c_str(), r.W, r.H, r.D,
              (unsigned long long)r.row_off, (unsigned long long)r.cell_off);
        CHECK(r.cell_off == units[r.unit].cell_offset, "%s, %s: cell_off", t, un.c_str());
        CHECK(r.lbx == d.ilbx && r.lby == d.ilby, "%s, %s: tile shape 2^%d x 2^%d", t, un.c_str(), r.lbx, r.lby);
        CHECK(r.tyv == std::min(1 << r.lby, d.hy - r.by0) && r.tyv >= 1, "%s, %s: tyv %d at by0 %d of %d", t, un.c_str(), r.tyv,
              r.by0, d.hy);
        CHECK(r.bx0 >= 0 && r.bx0 < d.hx && r.bx0 % (1 << r.lbx) == 0, "%s, %s: bx0 %d", t, un.c_str(), r.bx0);
        CHECK(r.by0 >= 0 && r.by0 < d.hy && r.by0 % (1 << r.lby) == 0, "%s, %s: by0 %d", t, un.c_str(), r.by0);
    }
    for (size_t k = 0; k < T; ++k) CHECK(hits[k] == 1, "%s: unit-major tile %zu appears %d times", t, k, hits[k]);
    if (o.xcd && T > 8) {
        // positions x, x + 8, ... hold one contiguous unit-order run; the runs of x = 0..7 follow one another
        uint32_t next = 0;
        for (size_t x = 0; x < 8; ++x)
            for (size_t p = x; p < T; p += 8, ++next)
                CHECK(P.rtiles[p].nat == next, "%s: list position %zu holds unit-major tile %u, XCD %zu's run is at %u", t, p,
                      P.rtiles[p].nat, x, next);
    }

    // block coverage and addresses, per unit
    for (int i = 0; i < n; ++i) {
        const UnitDev& d = P.units[i];
        if (!d.rix) continue;
        const std::string un = uname(P, (uint32_t)i);
        std::vector<int> cover((size_t)d.hx * d.hy, 0);
        std::vector<uint8_t> wrote(d.ncells, 0), read(d.ncells, 0);
        for (const RTile& r : P.rtiles) {
            if (r.unit != (uint32_t)i) continue;
            const int TX = 1 << r.lbx;
            for (int by = r.by0; by < r.by0 + r.tyv; ++by)
                for (int bx = r.bx0; bx < std::min(r.bx0 + TX, d.hx); ++bx)
                    if (by >= 0 && by < d.hy && bx >= 0) ++cover[(size_t)by * d.hx + bx];
            check_tile_addresses(P, r, tag, wrote, read, seen);
        }
        size_t bad_blocks = 0, bad_w = 0, bad_r = 0;
        for (int v : cover) bad_blocks += v != 1;
        for (uint8_t v : wrote) bad_w += v != 1;
        for (uint8_t v : read) bad_r += v != 1;
        CHECK(bad_blocks == 0, "%s, %s: %zu of %d x %d blocks not covered exactly once", t, un.c_str(), bad_blocks, d.hx, d.hy);
        CHECK(bad_w == 0, "%s, %s: %zu cells not written exactly once", t, un.c_str(), bad_w);
        CHECK(bad_r == 0, "%s, %s: %zu cells not read exactly once by the RMSE pass", t, un.c_str(), bad_r);
    }

    // dense side: a unit is in ixtiles / dtiles exactly when it has cells and is not row-indexed
    {
        std::vector<int> in_ix(n, 0), in_d(n, 0), in_rd(n, 0);
        for (const XTile& x : P.ixtiles)
            if (x.unit < (uint32_t)n) ++in_ix[x.unit];
        std::vector<uint32_t> next_d(n, 0), next_rd(n, 0);
        for (const FTile& f : P.dtiles) {
            CHECK(f.unit < (uint32_t)n, "%s: dtile of unit %u", t, f.unit);
            if (f.unit >= (uint32_t)n) continue;
            CHECK(f.index == next_d[f.unit], "%s, %s: dense decode tile %u before tile %u", t, uname(P, f.unit).c_str(), f.index,
                  next_d[f.unit]);
            next_d[f.unit] = f.index + 1;
            ++in_d[f.unit];
        }
        for (const FTile& f : P.rdtiles) {
            CHECK(f.unit < (uint32_t)n, "%s: rdtile of unit %u", t, f.unit);
            if (f.unit >= (uint32_t)n) continue;
            // the look-back's premise: a unit's tile t is launched after its tile t - 1
            CHECK(f.index == next_rd[f.unit], "%s, %s: row-index tile %u before tile %u", t, uname(P, f.unit).c_str(), f.index,
                  next_rd[f.unit]);
            next_rd[f.unit] = f.index + 1;
            ++in_rd[f.unit];
        }
        CHECK(P.ign + P.ifast == P.ixtiles.size(), "%s: ixtiles split %u + %u of %zu", t, P.ign, P.ifast, P.ixtiles.size());
        uint64_t granules = 0;
        for (int i = 0; i < n; ++i) {
            const UnitDev& d = P.units[i];
            const std::string un = uname(P, (uint32_t)i);
            const int kinds = (d.rix ? 1 : 0) + ((!d.rix && d.ncells) ? 1 : 0) + (d.ncells == 0 ? 1 : 0);
            CHECK(kinds == 1, "%s, %s: row-indexed %d cells %llu", t, un.c_str(), d.rix, (unsigned long long)d.ncells);
            if (d.rix) {
                CHECK(in_ix[i] == 0 && in_d[i] == 0, "%s, %s: row-indexed, yet %d dense inverse and %d dense decode tiles", t,
                      un.c_str(), in_ix[i], in_d[i]);
                CHECK(d.ndt == d.ncells / kRixTile + 1 && (uint32_t)in_rd[i] == d.ndt, "%s, %s: %d row-index tiles, ndt %u", t,
                      un.c_str(), in_rd[i], d.ndt);
                CHECK(d.nrt > 0, "%s, %s: no K6r tile", t, un.c_str());
            } else if (d.ncells) {
                CHECK(in_rd[i] == 0 && d.nrt == 0, "%s, %s: dense, yet %d row-index and %u K6r tiles", t, un.c_str(), in_rd[i],
                      d.nrt);
                CHECK((uint32_t)in_ix[i] == d.ntx && d.ntx > 0, "%s, %s: %d dense inverse tiles of %u", t, un.c_str(), in_ix[i],
                      d.ntx);
                CHECK(d.ndt == (d.ncells + kFlatTile - 1) / kFlatTile && (uint32_t)in_d[i] == d.ndt,
                      "%s, %s: %d dense decode tiles, ndt %u", t, un.c_str(), in_d[i], d.ndt);
            } else {
                CHECK(in_ix[i] == 0 && in_d[i] == 0 && in_rd[i] == 0 && d.nrt == 0, "%s, %s: an empty unit with tiles", t,
                      un.c_str());
            }
            CHECK(d.dt_begin == granules, "%s, %s: dt_begin %u after %llu granules", t, un.c_str(), d.dt_begin,
                  (unsigned long long)granules);
            granules += d.ndt;
        }
        CHECK(c->istate.bytes >= 8 * granules, "%s: %zu bytes of look-back granules for %llu tiles", t, c->istate.bytes,
              (unsigned long long)granules);
        CHECK(c->state.bytes >= decode_state_bytes(P), "%s: decode state %zu < %zu", t, c->state.bytes, decode_state_bytes(P));
    }

    // groups
    {
        const size_t ng = P.ig_rd.size();
        CHECK(ng >= 1 && P.ig_rt.size() == ng, "%s: %zu / %zu group boundaries", t, P.ig_rd.size(), P.ig_rt.size());
        if (ng < 1 || P.ig_rt.size() != ng) return;
        CHECK(P.ig_rd[0] == 0 && P.ig_rt[0] == 0, "%s: groups start at %u / %u", t, P.ig_rd[0], P.ig_rt[0]);
        CHECK(P.ig_rd.back() == P.rdtiles.size(), "%s: ig_rd ends at %u of %zu", t, P.ig_rd.back(), P.rdtiles.size());
        CHECK(P.ig_rt.back() == T, "%s: ig_rt ends at %u of %zu", t, P.ig_rt.back(), T);
        CHECK((int)ng - 1 <= (o.xcd ? 1 : o.groups), "%s: %zu groups", t, ng - 1);
        CHECK((T > 0) == (ng > 1), "%s: %zu K6r tiles in %zu groups", t, T, ng - 1);
        if (!o.xcd && o.groups == 3) CHECK(ng - 1 > 1, "%s: one group only", t);
        std::vector<int> group_of(n, -1);
        for (size_t g = 0; g + 1 < ng; ++g) {
            CHECK(P.ig_rd[g] <= P.ig_rd[g + 1] && P.ig_rt[g] <= P.ig_rt[g + 1], "%s: group %zu boundaries decrease", t, g);
            for (uint32_t k = P.ig_rd[g]; k < P.ig_rd[g + 1] && k < P.rdtiles.size(); ++k) {
                const uint32_t u = P.rdtiles[k].unit;
                if (u >= (uint32_t)n) continue;
                const UnitDev& d = P.units[u];
                CHECK(group_of[u] < 0 || group_of[u] == (int)g, "%s, %s: row-index tiles in groups %d and %zu", t,
                      uname(P, u).c_str(), group_of[u], g);
                group_of[u] = (int)g;
                // the group's K6r launch covers the unit's tiles (it waits for this group's row index only)
                if (!o.xcd)
                    CHECK(d.rt_begin >= P.ig_rt[g] && d.rt_begin + d.nrt <= P.ig_rt[g + 1],
                          "%s, %s: row index in group %zu, K6r tiles [%u, %u) outside the group's [%u, %u)", t, uname(P, u).c_str(),
                          g, d.rt_begin, d.rt_begin + d.nrt, P.ig_rt[g], P.ig_rt[g + 1]);
            }
            for (uint32_t p = P.ig_rt[g]; p < P.ig_rt[g + 1] && p < T; ++p) {
                const uint32_t u = P.rtiles[p].unit;
                if (u < (uint32_t)n)
                    CHECK(group_of[u] == (int)g, "%s, %s: K6r tile at %u in group %zu, the unit's row index in group %d", t,
                          uname(P, u).c_str(), p, g, group_of[u]);
            }
        }
    }

    // scratch
    CHECK(c->part.bytes >= sizeof(double) * 4 * T, "%s: %zu bytes of partial sums for %zu K6r tiles", t, c->part.bytes, T);
    CHECK(c->part.bytes >= sizeof(double) * P.ftiles.size(), "%s: partial sums of the flat tiles", t);
    CHECK(c->rowinfo.bytes >= 8 * P.rowinfo_entries, "%s: %zu bytes of row index for %llu entries", t, c->rowinfo.bytes,
          (unsigned long long)P.rowinfo_entries);
    CHECK(8 * P.rowinfo_entries == wc_rowindex_bytes(units.data(), n), "%s: %llu row entries, wc_rowindex_bytes %llu", t,
          (unsigned long long)P.rowinfo_entries, (unsigned long long)wc_rowindex_bytes(units.data(), n));
    CHECK(c->npairs.bytes >= 4 * (size_t)n, "%s: npairs", t);

    // the mirrors the kernels read
    auto same = [&](const DevBuf& d, const void* h, size_t bytes) {
        return bytes == 0 || (d.p && d.bytes >= bytes && std::memcmp(d.p, h, bytes) == 0);
    };
    CHECK(same(P.d_units, P.units.data(), sizeof(UnitDev) * P.units.size()), "%s: d_units differs from the plan", t);
    CHECK(same(P.d_rtiles, P.rtiles.data(), sizeof(RTile) * P.rtiles.size()), "%s: d_rtiles differs from the plan", t);
    CHECK(same(P.d_rdtiles, P.rdtiles.data(), sizeof(FTile) * P.rdtiles.size()), "%s: d_rdtiles differs from the plan", t);
    CHECK(same(P.d_ixtiles, P.ixtiles.data(), sizeof(XTile) * P.ixtiles.size()), "%s: d_ixtiles differs from the plan", t);
    CHECK(same(P.d_dtiles, P.dtiles.data(), sizeof(FTile) * P.dtiles.size()), "%s: d_dtiles differs from the plan", t);
}

static int build(wc_ctx* c, const std::vector<wc_unit>& units, const Opt& o) {
    c->opt_rix_lds = o.lds;
    c->opt_rix_lx = o.tx;
    c->opt_rix_xcd = o.xcd != 0;
    c->opt_inv_groups = o.groups;
    int rc = get_plan(c, units.data(), (int)units.size());
    if (rc == WC_OK) rc = ensure_scratch(c);
    CHECK(rc == WC_OK, "%s: get_plan / ensure_scratch rc %d (%s)", o.str().c_str(), rc, c->err.c_str());
    return rc;
}

// tile shape of unit u in the current plan
static bool shape_is(const Plan& P, int u, int tx, int ty) {
    return P.units[u].rix && (1 << P.units[u].ilbx) == tx && (1 << P.units[u].ilby) == ty;
}

// The whole sweep over one batch, on a context of its own.
static size_t sweep_batch(bool fast_only, Seen& seen) {
    g_batch = fast_only ? "fast-only batch" : "mixed batch";
    const std::vector<wc_unit> units = make_units(fast_only);
    wc_ctx* c = make_ctx();
    std::vector<Opt> sweep;
    for (int lds : {1024, 2048, 9216, 16384})
        for (int tx = 0; tx <= 5; ++tx) {
            sweep.push_back(Opt{lds, tx, 0, 1});
            sweep.push_back(Opt{lds, tx, 0, 3});
            sweep.push_back(Opt{lds, tx, 1, 1});
        }
    std::vector<TileKey> first;
    size_t plans = 0;
    for (const Opt& o : sweep) {
        const uint64_t gen = c->plan_gen;
        if (build(c, units, o) != WC_OK) continue;
        CHECK(c->plan_gen != gen, "%s: the previous option set's plan was reused", o.str().c_str());
        ++plans;
        check_plan(c, units, o, seen);
        if (first.empty()) first = tile_list(c->plan);
        const Plan& P = c->plan;
        // tile shapes worked out by hand from rix_wr (4 ((TY D + 4) TX + 16) floats <= budget)
        if (o.lds == 9216 && o.tx == 4) CHECK(shape_is(P, 6, 16, 4), "%s: 32^3 is not 16 x 4", o.str().c_str());
        if (o.lds == 9216 && o.tx == 5) CHECK(shape_is(P, 7, 32, 2), "%s: 64 x 8 x 24 is not 32 x 2", o.str().c_str());
        if (o.lds == 16384 && o.tx == 5) {
            CHECK(shape_is(P, 7, 32, 4), "%s: 64 x 8 x 24 is not 32 x 4", o.str().c_str());
            CHECK(shape_is(P, 5, 32, 1) && P.lds_rows == 63744, "%s: 64 x 2 x 120 is not 32 x 1 in 63744 B (lds_rows %zu)",
                  o.str().c_str(), P.lds_rows);
        }
        if (o.lds == 1024) {
            CHECK(P.units[10].rix && !P.units[11].rix, "%s: 2 x 2 x 232 rix %d, 2 x 2 x 240 rix %d", o.str().c_str(),
                  P.units[10].rix, P.units[11].rix);
            int rt[2] = {0, 0}, rd[2] = {0, 0}, ix[2] = {0, 0}, dt[2] = {0, 0};  // tiles of units 10 and 11 per list
            for (const RTile& r : P.rtiles)
                if (r.unit == 10 || r.unit == 11) ++rt[r.unit - 10];
            for (const FTile& f : P.rdtiles)
                if (f.unit == 10 || f.unit == 11) ++rd[f.unit - 10];
            for (const XTile& x : P.ixtiles)
                if (x.unit == 10 || x.unit == 11) ++ix[x.unit - 10];
            for (const FTile& f : P.dtiles)
                if (f.unit == 10 || f.unit == 11) ++dt[f.unit - 10];
            CHECK(rt[0] == 1 && rd[0] == 1 && ix[0] == 0 && dt[0] == 0, "%s: 2 x 2 x 232 has %d K6r, %d row-index, %d dense inverse, %d dense decode tiles",
                  o.str().c_str(), rt[0], rd[0], ix[0], dt[0]);
            CHECK(rt[1] == 0 && rd[1] == 0 && ix[1] == (int)P.units[11].ntx && ix[1] > 0 && dt[1] == 1, "%s: 2 x 2 x 240 has %d K6r, %d row-index, %d dense inverse, %d dense decode tiles",
                  o.str().c_str(), rt[1], rd[1], ix[1], dt[1]);
        }
    }
    CHECK(plans > 16 && c->plan_cache.size() == 16, "%zu plans built, %zu cached", plans, c->plan_cache.size());
    // the first option set again, long evicted from the cache, then once more from the cache
    for (int again = 0; again < 2 && !sweep.empty(); ++again) {
        const long calls = fake::calls();
        if (build(c, units, sweep[0]) != WC_OK) break;
        // a rebuild uploads its tables; a cached plan comes back without a runtime call
        CHECK((fake::calls() != calls) == (again == 0), "%s again (%d): %ld runtime calls", sweep[0].str().c_str(), again,
              fake::calls() - calls);
        CHECK(tile_list(c->plan) == first, "%s again (%d): another tile list than the first time", sweep[0].str().c_str(), again);
        check_plan(c, units, sweep[0], seen);
        if (again == 0) build(c, units, sweep[1]);  // push it into the cache
    }
    // what makes wc_inverse_rmse fuse the RMSE (wc_capi.cpp wc_inverse_rows): every unit with cells row-indexed;
    // from budget 2048 on that is the fast-only batch, never the mixed one
    if (build(c, units, Opt{2048, 5, 1, 1}) == WC_OK) {
        bool all_rix = true;
        for (const UnitDev& d : c->plan.units) all_rix &= d.rix || d.ncells == 0;
        CHECK(all_rix == fast_only, "%s: every unit row-indexed %d at budget 2048", g_batch, all_rix);
    }
    destroy_ctx(c);
    return plans;
}

// The units of tests/long_axis_shapes.py (UNITS + RIX16K, in that order, at layout()'s cell
// offsets) with its class table CLASSES; tests/test_long_axis_cpu.py compares these rows with
// that file.  rix: {ilbx, ilby} at that WC_OPT_RIX_LDS and WC_OPT_RIX_TX 4, {-1, -1}: dense decode.
struct LongUnit {
    const char* tag;
    int w, h, d;
    uint64_t off;
    int fast, sparse, lbx, lby, lbz, big;
    uint32_t net, ntx;
    int rix9216[2], rix16384[2];
};
static const LongUnit kLong[] = {
    {"big_x", 2048, 32, 32, 3, 1, 1, 5, 1, 4, 1, 128, 256, {4, 2}, {4, 2}},
    {"big_y", 32, 2048, 32, 2097157, 1, 1, 4, 2, 4, 1, 128, 256, {4, 2}, {4, 2}},
    {"big_z", 32, 32, 2048, 4194316, 1, 1, 4, 1, 5, 1, 128, 256, {0, 0}, {0, 0}},
    {"below_big", 2046, 32, 32, 6291471, 1, 1, 5, 1, 4, 0, 256, 256, {4, 2}, {4, 2}},
    {"s32_x", 2048, 2, 64, 8386584, 1, 1, 5, 0, 5, 0, 32, 32, {4, 0}, {4, 0}},
    {"s32_z", 64, 2, 2048, 8648736, 1, 1, 5, 0, 5, 0, 32, 32, {0, 0}, {0, 0}},
    {"pencil_x", 4096, 2, 8, 8910887, 1, 0, 5, 0, 2, 0, 8, 64, {4, 0}, {4, 0}},
    {"s32_y", 64, 34, 64, 8976428, 1, 1, 5, 0, 5, 0, 17, 17, {4, 1}, {4, 1}},
    {"pencil_y", 2, 4096, 8, 9115692, 1, 0, 0, 8, 2, 0, 8, 8, {0, 8}, {0, 8}},
    {"pencil_z", 2, 2, 4096, 9181235, 1, 1, 0, 0, 5, 0, 2, 64, {-1, -1}, {-1, -1}},
    {"rix_edge_in", 2, 2, 2280, 9197626, 1, 0, 0, 0, 5, 0, 2, 36, {0, 0}, {0, 0}},
    {"rix_edge_out", 2, 2, 2288, 9206751, 1, 0, 0, 0, 5, 0, 2, 36, {-1, -1}, {0, 0}},
    {"rix_edge_wide", 4, 6, 2280, 9215905, 1, 0, 1, 2, 5, 0, 7, 36, {0, 0}, {0, 0}},
    {"magic_d_x", 130, 2, 1000, 9270625, 1, 0, 5, 0, 5, 0, 32, 48, {1, 0}, {2, 0}},
    {"magic_d_y", 2, 130, 1000, 9530633, 1, 0, 0, 5, 5, 0, 32, 48, {0, 1}, {0, 2}},
    {"magic_d_3000", 8, 8, 3000, 9790635, 1, 0, 2, 2, 5, 0, 24, 47, {-1, -1}, {0, 0}},
    {"magic_d_200", 66, 2, 200, 9982641, 1, 0, 5, 0, 5, 0, 4, 8, {3, 0}, {4, 0}},
    {"lx_shrink_264", 256, 2, 264, 10009045, 1, 0, 5, 0, 5, 0, 17, 20, {3, 0}, {3, 0}},
    {"lx_shrink_hx513", 1026, 4, 40, 10144217, 1, 0, 5, 0, 5, 0, 21, 34, {4, 1}, {4, 1}},
    {"lx_shrink_hy513", 4, 1026, 24, 10308381, 1, 0, 1, 5, 4, 0, 13, 17, {1, 5}, {1, 6}},
    {"lx_shrink_160", 192, 6, 160, 10406877, 1, 0, 5, 0, 5, 0, 23, 27, {3, 0}, {4, 0}},
    {"slab_x", 320, 64, 8, 10591199, 1, 0, 5, 3, 2, 0, 20, 20, {4, 4}, {4, 4}},
    {"slab_y", 64, 320, 8, 10755040, 1, 0, 5, 3, 2, 0, 20, 20, {4, 4}, {4, 4}},
    {"odd_x", 2049, 3, 5, 10918881, 0, 0, 5, 1, 2, 0, 4, 33, {-1, -1}, {-1, -1}},
    {"odd_y", 3, 2049, 5, 10949619, 0, 0, 1, 7, 2, 0, 4, 9, {-1, -1}, {-1, -1}},
    {"odd_z", 3, 5, 2049, 10980358, 0, 0, 1, 2, 5, 0, 4, 33, {-1, -1}, {-1, -1}},
    {"line_x", 4097, 1, 1, 11011097, 0, 0, 5, 0, 0, 0, 1, 65, {-1, -1}, {-1, -1}},
    {"line_y", 1, 4097, 1, 11015195, 0, 0, 0, 10, 0, 0, 1, 3, {-1, -1}, {-1, -1}},
    {"line_z", 1, 1, 4097, 11019299, 0, 0, 0, 0, 5, 0, 1, 65, {-1, -1}, {-1, -1}},
    {"empty", 0, 2048, 8, 11023399, 0, 0, 0, 8, 2, 0, 1, 0, {-1, -1}, {-1, -1}},
    {"s32_x_odd", 2048, 2, 64, 11023407, 1, 1, 5, 0, 5, 0, 32, 32, {4, 0}, {4, 0}},
    {"s32_z_odd", 64, 2, 2048, 11285559, 1, 1, 5, 0, 5, 0, 32, 32, {0, 0}, {0, 0}},
    {"s32_y_odd", 64, 34, 64, 11547705, 1, 1, 5, 0, 5, 0, 17, 17, {4, 1}, {4, 1}},
    {"rix16k_in", 2, 2, 4072, 11686977, 1, 0, 0, 0, 5, 0, 2, 64, {-1, -1}, {0, 0}},
    {"rix16k_out", 2, 2, 4080, 11703269, 1, 0, 0, 0, 5, 0, 2, 64, {-1, -1}, {-1, -1}},
};
static constexpr int kLongUnits = (int)(sizeof(kLong) / sizeof(kLong[0]));
static constexpr uint64_t kLongPlanCells = 300000;  // long_axis_shapes.PLAN_CELLS

// div_rows of wc_device.h, restated
static uint32_t div_rows_host(uint32_t p, uint64_t dmagic) {
    if ((uint32_t)dmagic == 0u) return p >> (uint32_t)(dmagic >> 32);
    return (uint32_t)(((uint64_t)p * (uint32_t)dmagic) >> (uint32_t)(dmagic >> 32));
}

// The forward's fields of a plan of `rows` (a subset of kLong, in its order) against the table.
static void check_forward_fields(const Plan& P, const std::vector<const LongUnit*>& rows, const char* t) {
    const int n = (int)rows.size();
    CHECK((int)P.units.size() == n, "%s: %zu unit descriptors", t, P.units.size());
    if ((int)P.units.size() != n) return;
    uint32_t et = 0, small_blocks = 0;
    uint64_t row_entries = 0;
    for (int i = 0; i < n; ++i) {
        const UnitDev& d = P.units[i];
        const LongUnit& L = *rows[i];
        const char* g = L.tag;
        CHECK(d.nx == L.w && d.ny == L.h && d.nz == L.d && d.cell_off == L.off, "%s, %s: dims %d x %d x %d at %llu", t, g, d.nx,
              d.ny, d.nz, (unsigned long long)d.cell_off);
        CHECK(d.fast == L.fast, "%s, %s: fast %d", t, g, d.fast);
        CHECK((int)d.sparse == L.sparse, "%s, %s: sparse %u", t, g, d.sparse);
        CHECK(d.lbx == L.lbx && d.lby == L.lby && d.lbz == L.lbz, "%s, %s: transform tile 2^(%d, %d, %d)", t, g, d.lbx, d.lby,
              d.lbz);
        CHECK(d.lbx + d.lby + d.lbz <= 10, "%s, %s: more than kMaxTileBlocks blocks per tile", t, g);
        CHECK(d.ntx == L.ntx, "%s, %s: ntx %u", t, g, d.ntx);
        CHECK(d.net == L.net, "%s, %s: net %u", t, g, d.net);
        CHECK(d.et_begin == et, "%s, %s: et_begin %u after %u emit tiles", t, g, d.et_begin, et);
        et += d.net;
        CHECK((d.ncells >= kEmitBigCells) == (L.big != 0), "%s, %s: %llu cells, big %d", t, g, (unsigned long long)d.ncells, L.big);
        if (!L.big) small_blocks += d.net;
        CHECK(d.row_off == row_entries, "%s, %s: row_off %llu", t, g, (unsigned long long)d.row_off);
        if (d.ncells) row_entries += (uint64_t)L.w * L.h + 1;
        // the transform tiles of the unit: a grid of ntx tiles over its blocks, inside the unit
        uint32_t tiles = 0;
        for (const XTile& x : P.xtiles)
            if (x.unit == (uint32_t)i) {
                ++tiles;
                CHECK((int)x.bx0 < d.nbx && (int)x.by0 < d.nby && (int)x.bz0 < d.nbz && x.bx0 % (1u << d.lbx) == 0 &&
                          x.by0 % (1u << d.lby) == 0 && x.bz0 % (1u << d.lbz) == 0,
                      "%s, %s: transform tile at block (%u, %u, %u)", t, g, x.bx0, x.by0, x.bz0);
            }
        CHECK(tiles == d.ntx, "%s, %s: %u transform tiles listed, ntx %u", t, g, tiles, d.ntx);
        // dmagic: the shift form for D = 2^l, else m = floor(2^(31 + l) / D) + 1 with the shift 31 + l
        if (!L.fast) {
            CHECK(d.dmagic == 0, "%s, %s: dmagic %llx of a unit without a row index", t, g, (unsigned long long)d.dmagic);
            continue;
        }
        const uint32_t D = (uint32_t)L.d;
        const bool pow2 = (D & (D - 1)) == 0;
        CHECK(((uint32_t)d.dmagic == 0u) == pow2, "%s, %s: dmagic %llx for D %u", t, g, (unsigned long long)d.dmagic, D);
        CHECK((d.dmagic >> 32) == (uint64_t)ceil_log2(D) + (pow2 ? 0 : 31), "%s, %s: dmagic shift %llu", t, g,
              (unsigned long long)(d.dmagic >> 32));
        uint64_t bad = 0, first_bad = 0;
        auto probe = [&](uint64_t p) {
            if (p >= (uint64_t(1) << 31)) return;
            ++g_checks;
            if (div_rows_host((uint32_t)p, d.dmagic) != (uint32_t)(p / D) && !bad++) first_bad = p;
        };
        for (uint64_t q = 0; q <= (uint64_t)L.w * L.h; ++q) {
            if (q) probe(q * D - 1);
            probe(q * D);
            probe(q * D + 1);
        }
        probe((uint64_t(1) << 31) - 1);
        CHECK(bad == 0, "%s, %s: div_rows wrong at %llu positions, first p = %llu: %u, floor(p / %u) = %llu", t, g,
              (unsigned long long)bad, (unsigned long long)first_bad, div_rows_host((uint32_t)first_bad, d.dmagic), D,
              (unsigned long long)(first_bad / D));
    }
    CHECK(P.netiles == et, "%s: netiles %u of %u", t, P.netiles, et);
    CHECK(P.rowinfo_entries == row_entries, "%s: %llu row entries", t, (unsigned long long)P.rowinfo_entries);
    // emit blocks: [small-unit launch | big-unit launch], each tile of each unit once, a unit's tiles in order
    CHECK(P.nedesc_small == small_blocks && P.edesc.size() == et, "%s: %u small emit blocks of %zu, expected %u of %u", t,
          P.nedesc_small, P.edesc.size(), small_blocks, et);
    std::vector<uint32_t> next(n, 0);
    for (size_t k = 0; k < P.edesc.size(); ++k) {
        const EmitDesc& e = P.edesc[k];
        CHECK(e.unit < (uint32_t)n, "%s: emit block %zu of unit %u", t, k, e.unit);
        if (e.unit >= (uint32_t)n) continue;
        const UnitDev& d = P.units[e.unit];
        const LongUnit& L = *rows[e.unit];
        CHECK((k >= P.nedesc_small) == (L.big != 0), "%s, %s: emit block %zu in the %s launch", t, L.tag, k,
              k >= P.nedesc_small ? "big" : "small");
        CHECK(e.index == next[e.unit], "%s, %s: emit tile %u before tile %u", t, L.tag, e.index, next[e.unit]);
        next[e.unit] = e.index + 1;
        CHECK(e.coef_off == d.coef_off && e.pay_off == d.pay_off && e.ncells == d.ncells && e.et_begin == d.et_begin &&
                  e.net == d.net && e.nx == d.nx && e.ny == d.ny && e.nz == d.nz,
              "%s, %s: emit block %zu does not carry its unit's fields", t, L.tag, k);
        CHECK((e.mode & 1u) == d.sparse && ((e.mode >> 1) & 7u) == (uint32_t)d.lbz && (e.mode >> 8) == (uint32_t)(d.dmagic >> 32) &&
                  e.dmul == (uint32_t)d.dmagic,
              "%s, %s: emit block %zu mode %x dmul %x", t, L.tag, k, e.mode, e.dmul);
        CHECK(e.row_off == d.row_off && e.flag_off == (uint32_t)d.flag_off, "%s, %s: emit block %zu row_off %u flag_off %u", t, L.tag,
              k, e.row_off, e.flag_off);
    }
    for (int i = 0; i < n; ++i) CHECK(next[i] == P.units[i].net, "%s, %s: %u of %u emit tiles listed", t, rows[i]->tag, next[i], P.units[i].net);
}

static int long_index(const std::vector<const LongUnit*>& rows, const char* tag) {
    for (size_t i = 0; i < rows.size(); ++i)
        if (std::strcmp(rows[i]->tag, tag) == 0) return (int)i;
    CHECK(false, "long-axis batch: no unit %s", tag);
    return 0;
}

// The third batch.
static size_t sweep_long_axis(Seen& seen) {
    g_batch = "long-axis batch";
    size_t plans = 0;
    // the fast-shape units of at most kLongPlanCells cells: every check of the other batches
    std::vector<const LongUnit*> rows;
    std::vector<wc_unit> units;
    for (const LongUnit& L : kLong)
        if (L.fast && (uint64_t)L.w * L.h * L.d <= kLongPlanCells) {
            rows.push_back(&L);
            units.push_back(wc_unit{L.off, L.w, L.h, L.d, 0});
        }
    CHECK(rows.size() == 24, "long-axis batch: %zu fast units of at most %llu cells", rows.size(), (unsigned long long)kLongPlanCells);
    const int in9216 = long_index(rows, "rix_edge_in"), out9216 = long_index(rows, "rix_edge_out");
    const int in16k = long_index(rows, "rix16k_in"), out16k = long_index(rows, "rix16k_out");
    CHECK(rows[in9216]->d == 2280 && rows[out9216]->d == 2288 && rows[in16k]->d == 4072 && rows[out16k]->d == 4080,
          "long-axis batch: the boundary units are not D = 2280 / 2288 / 4072 / 4080");
    wc_ctx* c = make_ctx();
    std::vector<Opt> sweep;
    for (int lds : {9216, 16384})
        for (int tx : {0, 4, 5}) {
            sweep.push_back(Opt{lds, tx, 0, 1});
            if (tx == 4) {
                sweep.push_back(Opt{lds, tx, 0, 3});
                sweep.push_back(Opt{lds, tx, 1, 1});
            }
        }
    sweep.push_back(Opt{9200, 4, 0, 1});  // 4 D + 80 == the budget for D = 2280: still row-indexed
    for (const Opt& o : sweep) {
        if (build(c, units, o) != WC_OK) continue;
        ++plans;
        check_plan(c, units, o, seen);
        const Plan& P = c->plan;
        const std::string tag = o.str();
        const char* t = tag.c_str();
        check_forward_fields(P, rows, t);
        // the fallback boundary of each budget, by name
        const bool r2280 = P.units[in9216].rix, r2288 = P.units[out9216].rix, r4072 = P.units[in16k].rix, r4080 = P.units[out16k].rix;
        if (o.lds == 9216 || o.lds == 9200)
            CHECK(r2280 && !r2288 && !r4072 && !r4080, "%s: rix of 2 x 2 x 2280 / 2288 / 4072 / 4080 = %d / %d / %d / %d", t, r2280,
                  r2288, r4072, r4080);
        else
            CHECK(r2280 && r2288 && r4072 && !r4080, "%s: rix of 2 x 2 x 2280 / 2288 / 4072 / 4080 = %d / %d / %d / %d", t, r2280, r2288,
                  r4072, r4080);
        for (size_t i = 0; i < rows.size(); ++i) {
            const UnitDev& d = P.units[i];
            const int* want = o.lds == 16384 ? rows[i]->rix16384 : rows[i]->rix9216;
            if (want[0] < 0) {
                CHECK(!d.rix, "%s, %s: row-indexed, the table says dense", t, rows[i]->tag);
                // a dense fast unit: every transform tile once in the dense inverse list, one decode tile per 4096 cells
                uint32_t ix = 0;
                for (const XTile& x : P.ixtiles) ix += x.unit == (uint32_t)i;
                CHECK(ix == d.ntx && d.nrt == 0, "%s, %s: %u dense inverse tiles of %u, %u K6r tiles", t, rows[i]->tag, ix, d.ntx, d.nrt);
            } else if (o.tx == 4 && o.lds != 9200) {
                CHECK(shape_is(P, (int)i, 1 << want[0], 1 << want[1]), "%s, %s: K6r tile 2^%d x 2^%d, the table says 2^%d x 2^%d", t,
                      rows[i]->tag, d.ilbx, d.ilby, want[0], want[1]);
            } else {
                CHECK(d.rix && d.ilbx <= o.tx, "%s, %s: rix %d, K6r tile 2^%d x 2^%d", t, rows[i]->tag, d.rix, d.ilbx, d.ilby);
            }
        }
    }
    destroy_ctx(c);
    // the whole list once, at the defaults: the forward's fields, the 2^21-cell units and the generic ones included
    {
        std::vector<const LongUnit*> all;
        std::vector<wc_unit> all_units;
        uint64_t end = 0;
        for (const LongUnit& L : kLong) {
            CHECK(L.off >= end && L.off <= end + 10, "long-axis batch, %s: offset %llu after %llu", L.tag, (unsigned long long)L.off,
                  (unsigned long long)end);
            end = L.off + (uint64_t)L.w * L.h * L.d;
            all.push_back(&L);
            all_units.push_back(wc_unit{L.off, L.w, L.h, L.d, 0});
        }
        wc_ctx* c2 = make_ctx();
        const Opt o{9216, 4, 0, 1};
        if (build(c2, all_units, o) == WC_OK) {
            ++plans;
            const std::string tag = o.str() + " (whole list)";
            check_forward_fields(c2->plan, all, tag.c_str());
            for (int i = 0; i < kLongUnits; ++i) {
                const UnitDev& d = c2->plan.units[i];
                const int* want = kLong[i].rix9216;
                CHECK(want[0] < 0 ? !d.rix : shape_is(c2->plan, i, 1 << want[0], 1 << want[1]), "%s, %s: rix %d, K6r tile 2^%d x 2^%d",
                      tag.c_str(), kLong[i].tag, d.rix, d.ilbx, d.ilby);
            }
        }
        destroy_ctx(c2);
    }
    return plans;
}

int main() {
    Seen seen;
    size_t plans = sweep_batch(false, seen);
    plans += sweep_batch(true, seen);
    plans += sweep_long_axis(seen);
    // every branch the device test is after was in the sweep
    CHECK(seen.tx32 && seen.ty32 && seen.tx1_aligned && seen.edge_x && seen.edge_y && seen.quad && seen.quad_edge &&
              seen.pair8 && seen.scalar && seen.fallback && seen.lds_63744,
          "branches seen: tx32 %d ty32 %d tx1 %d edge_x %d edge_y %d quad %d quad_edge %d pair8 %d scalar %d fallback %d 63744 %d",
          seen.tx32, seen.ty32, seen.tx1_aligned, seen.edge_x, seen.edge_y, seen.quad, seen.quad_edge, seen.pair8, seen.scalar,
          seen.fallback, seen.lds_63744);
    std::printf("test_plan: %d checks, %d failed, %zu plans, %zu allocations left\n", g_checks, g_fail, plans,
                fake::live_allocations());
    return g_fail ? 1 : 0;
}
