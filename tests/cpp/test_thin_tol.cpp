// test_thin_tol.cpp — the host side of the tolerance forms of the compressed-domain thinning and
// split on the CPU, for the ASan + UBSan build (`make thintolsan`, run by tests/test_thin_tol_san.py):
// wc_thin_tol_unit / wc_split_tol_unit (wc_thintolrule.cpp) and the host drivers wc_thin_tol_host /
// wc_split_tol_host (wc_thintolhost.cpp, on wc_hostserial.cpp's driver) over the fake HIP runtime of
// tests/cpp/fake_device.cpp.  No GPU and no kernel: the device entry points the drivers call
// (wc::thin_tol_device, wc::split_tol_device) are restated here on the unit rule, into wc_forward's
// slot layout, as the real ones write it.  Every buffer the rule or a driver reads or writes is a heap
// block of exactly the documented size, so a read or write past one is reported.
//
//   rule     on seeded payloads (runs that overshoot, surplus pairs, values +-0, NaN, +-inf,
//            subnormals) at tolerances 0, fractions of the payload's weighted RMS and +inf: output
//            capacity exactly 20 + 8 kept (one byte less: WC_ERR_INVALID, nothing written); a
//            brute-force restatement on the dense array (per-level counts of every entry, zeros
//            included, wc_tol_levels_threshold, the threshold test) gives the same thresholds, bound
//            and kept set; bound <= tol; tol = 0 keeps every candidate; the split's base is the
//            thinning, its rest the other candidates, and wc_merge_unit gives canon(P) back; the
//            refusals.
//   drivers  the same payloads as one batch with gaps between them, levels from the headers and
//            given, WC_OPT_HOST_CHUNK 0 / small (several runs): packed offsets, counts and bytes
//            equal to the unit rule's, thresholds and bounds; null thresh / bound; a capacity one
//            byte short; a NaN tolerance; a header that disagrees (WC_ERR_FORMAT before anything
//            runs, outputs untouched).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

extern "C" uint64_t wc_thin_bound(const wc_unit* units, int n, const uint32_t* max_pairs) {  // wc_capi.cpp's
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) {
        const uint64_t N = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        b += 24 + 8 * (max_pairs ? std::min<uint64_t>(max_pairs[i], N) : N);
    }
    return b;
}

// wc_tolhost.cpp is linked for validate_tol; the device entry points of its own host form never run here
extern "C" int wc_forward_tol(wc_ctx*, const void*, int, const wc_unit*, int, const double*, uint8_t*, uint64_t, uint64_t*,
                              uint32_t*, float*, double*) {
    std::abort();
}
extern "C" int wc_inverse_rmse(wc_ctx*, const uint8_t*, const uint64_t*, const wc_unit*, int, const void*, int, float*,
                               double*) {
    std::abort();
}

namespace {
std::vector<std::unique_ptr<std::vector<UnitDev>>> g_tabs;  // launch_pack reads the slots from these

uint64_t unit_len(const uint8_t* p) {
    int32_t nrle;
    std::memcpy(&nrle, p + 16, 4);
    return 20 + 8ull * (uint64_t)nrle;
}

std::vector<UnitDev>& slot_table(wc_ctx* c, const wc_unit* units, int n) {
    g_tabs.emplace_back(new std::vector<UnitDev>(n));
    std::vector<UnitDev>& tab = *g_tabs.back();
    c->plan.d_units.p = tab.data();
    uint64_t slot = 4;
    for (int u = 0; u < n; ++u) {
        tab[u].pay_off = slot;
        slot += 24 + 8 * (uint64_t)units[u].nx * units[u].ny * units[u].nz;
    }
    return tab;
}
}  // namespace

// The device calls, restated: after the uploads, unit u through the unit rule into its slots.
namespace wc {
int split_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                     const int32_t* levels, const double* tol, uint8_t* d_base, uint64_t base_capacity,
                     uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest, float* d_thresh,
                     double* d_bound) {
    (void)levels;
    if (base_capacity < wc_payload_bound(units, n) || rest.capacity < wc_payload_bound(units, n))
        return fail(c, WC_ERR_INVALID, "capacity");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return WC_ERR_HIP;
    const std::vector<UnitDev>& tab = slot_table(c, units, n);
    for (int u = 0; u < n; ++u) {
        const uint64_t N = (uint64_t)units[u].nx * units[u].ny * units[u].nz, slot = tab[u].pay_off;
        const uint8_t* p = d_payload + d_offsets[u];
        size_t bl = 0, rl = 0;
        float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
        double bound = 0.0;
        const int rc = rest.d_rest ? wc_split_tol_unit(p, unit_len(p), tol[u], d_base + slot, 20 + 8 * N, &bl,
                                                       rest.d_rest + slot, 20 + 8 * N, &rl, th, &bound)
                                   : wc_thin_tol_unit(p, unit_len(p), tol[u], d_base + slot, 20 + 8 * N, &bl, th, &bound);
        if (rc != WC_OK) return fail(c, rc, "fake: the unit rule refused unit " + std::to_string(u));
        d_base_offsets[u] = slot;
        d_kept[u] = (uint32_t)((bl - 20) / 8);
        if (rest.d_rest) {
            rest.d_offsets[u] = slot;
            rest.d_pairs[u] = (uint32_t)((rl - 20) / 8);
        }
        if (d_thresh) std::memcpy(d_thresh + (size_t)WC_MAX_LEVELS * u, th, sizeof th);
        if (d_bound) d_bound[u] = bound;
        if (u == n - 1) {
            d_base_offsets[n] = slot + bl;
            if (rest.d_rest) rest.d_offsets[n] = slot + rl;
        }
    }
    c->err_check_pending = true;
    return WC_OK;
}

int thin_tol_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                    const int32_t* levels, const double* tol, uint8_t* d_out, uint64_t out_capacity,
                    uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, double* d_bound) {
    return split_tol_device(c, d_payload, d_offsets, units, n, levels, tol, d_out, out_capacity, d_out_offsets, d_kept,
                            SplitOut{nullptr, ~0ull, nullptr, nullptr}, d_thresh, d_bound);
}
}  // namespace wc

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
    c->plan.d_units.p = nullptr;  // this file's own tables
    for (wc::DevBuf* b : {&c->errflag, &c->h_payload, &c->h_packed, &c->h_offsets, &c->h_poff, &c->h_kept, &c->h_out,
                          &c->h_thresh, &c->h_bound, &c->pk_off, &c->h_second, &c->h_second_off, &c->h_second_cnt})
        if (b->p) (void)hipFree(b->p);
    (void)hipStreamDestroy(c->own);
    fake::release_context_tables(c);
    delete c;
}

// ---- seeded payloads ------------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

using Bytes = std::vector<uint8_t>;
struct Pay {
    int32_t W, H, D, L;
    Bytes bytes;  // exactly 20 + 8 nrle
};

static Pay make_payload(Rng& r, int32_t W, int32_t H, int32_t D, int L, uint32_t n, uint32_t max_run) {
    Pay p{W, H, D, L, Bytes(20 + 8ull * n)};
    const int64_t N = (int64_t)W * H * D;
    const int32_t h[5] = {W, H, D, L >= 2 ? -L : (int32_t)N, (int32_t)n};
    std::memcpy(p.bytes.data(), h, 20);
    static const uint32_t special[] = {0u, 0x80000000u, 0x7FC00000u, 0xFF800001u, 0x7F800000u, 0xFF800000u, 1u, 0x80000003u};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t c = r.next() % 100;
        int32_t run = (int32_t)(r.next() % (max_run + 1));
        if (c == 0) run = 0x7fffffff;  // overshoots
        uint32_t bits;
        if (c < 6) {
            bits = special[r.next() % 8];
        } else {  // magnitudes over six decades, either sign
            const float v = std::ldexp((float)(1 + r.next() % 1000) * 1e-3f, (int)(r.next() % 20) - 10) * (r.next() % 2 ? -1.f : 1.f);
            std::memcpy(&bits, &v, 4);
        }
        std::memcpy(p.bytes.data() + 20 + 8ull * k, &run, 4);
        std::memcpy(p.bytes.data() + 24 + 8ull * k, &bits, 4);
    }
    return p;
}

// the dense array of a payload and the level index of every entry, by the definitions
static void dense_of(const Pay& p, std::vector<uint32_t>& A, std::vector<int>& lv) {
    const uint64_t N = (uint64_t)p.W * p.H * p.D;
    A.assign(N, 0u);
    lv.assign(N, 0);
    for (uint64_t q = 0; q < N; ++q) {
        const uint64_t K = q % p.D, J = (q / p.D) % p.H, I = q / ((uint64_t)p.D * p.H);
        for (int s = 1; s < p.L; ++s) lv[q] += (I < (uint64_t)(p.W >> s) && J < (uint64_t)(p.H >> s) && K < (uint64_t)(p.D >> s));
    }
    int32_t n;
    std::memcpy(&n, p.bytes.data() + 16, 4);
    uint64_t pos = 0;
    for (int32_t k = 0; k < n; ++k) {
        int32_t run;
        uint32_t b;
        std::memcpy(&run, p.bytes.data() + 20 + 8ull * k, 4);
        std::memcpy(&b, p.bytes.data() + 24 + 8ull * k, 4);
        pos += (uint64_t)run;
        if (pos >= N) break;
        A[pos++] = b;
    }
}

static bool candidate(uint32_t bits) {
    const uint32_t m = bits & 0x7fffffffu;
    return m >= 1u && m <= 0x7f800000u;
}

// the payload of the entries of A that `keep` selects
template <class Keep>
static Bytes emit(const Pay& p, const std::vector<uint32_t>& A, Keep keep) {
    Bytes out(20);
    std::memcpy(out.data(), p.bytes.data(), 16);
    int64_t last = -1;
    int32_t n = 0;
    for (size_t q = 0; q < A.size(); ++q) {
        if (!keep(q)) continue;
        const int32_t run = (int32_t)((int64_t)q - last - 1);
        out.resize(out.size() + 8);
        std::memcpy(out.data() + out.size() - 8, &run, 4);
        std::memcpy(out.data() + out.size() - 4, &A[q], 4);
        last = (int64_t)q;
        ++n;
    }
    std::memcpy(out.data() + 16, &n, 4);
    return out;
}

struct Thinned {
    Bytes bytes, rest;
    float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
    double bound = 0.0;
    bool ok = false;
};

// wc_thin_tol_unit and wc_split_tol_unit with exact-size heap buffers
static Thinned thin_exact(const Pay& p, double tol, const char* what) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[p.bytes.size()]);
    std::memcpy(in.get(), p.bytes.data(), p.bytes.size());
    std::unique_ptr<uint8_t[]> big(new uint8_t[p.bytes.size()]), big2(new uint8_t[p.bytes.size()]);
    size_t w = 0, rl = 0;
    Thinned t;
    std::unique_ptr<float[]> tl(new float[p.L]);
    int rc = wc_thin_tol_unit(in.get(), p.bytes.size(), tol, big.get(), p.bytes.size(), &w, tl.get(), &t.bound);
    CHECK(rc == WC_OK && w >= 20 && w <= p.bytes.size() && (w - 20) % 8 == 0, "%s rc %d", what, rc);
    if (rc != WC_OK) return t;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[w]);
    size_t w2 = 0;
    rc = wc_thin_tol_unit(in.get(), p.bytes.size(), tol, exact.get(), w, &w2, nullptr, nullptr);
    CHECK(rc == WC_OK && w2 == w && std::memcmp(exact.get(), big.get(), w) == 0, "%s exact capacity", what);
    size_t w3 = 77;
    std::unique_ptr<uint8_t[]> small(new uint8_t[w - 1]);
    std::memset(small.get(), 0x5a, w - 1);
    rc = wc_thin_tol_unit(in.get(), p.bytes.size(), tol, small.get(), w - 1, &w3, nullptr, nullptr);
    CHECK(rc == WC_ERR_INVALID && w3 == 77 && std::all_of(small.get(), small.get() + w - 1, [](uint8_t b) { return b == 0x5a; }),
          "%s short capacity", what);
    t.bytes.assign(exact.get(), exact.get() + w);
    std::memcpy(t.th, tl.get(), sizeof(float) * p.L);
    // the split: first into ample blocks for the lengths, then into exact ones
    size_t bl = 0;
    std::unique_ptr<float[]> tl2(new float[p.L]);
    double bound2 = -1.0;
    rc = wc_split_tol_unit(in.get(), p.bytes.size(), tol, big.get(), p.bytes.size(), &bl, big2.get(), p.bytes.size(), &rl,
                           tl2.get(), &bound2);
    CHECK(rc == WC_OK && bl == w && std::memcmp(big.get(), exact.get(), w) == 0, "%s: the base is the thinning", what);
    CHECK(rc == WC_OK && std::memcmp(tl2.get(), tl.get(), sizeof(float) * p.L) == 0 && std::memcmp(&bound2, &t.bound, 8) == 0,
          "%s: the split's thresholds and bound", what);
    if (rc != WC_OK) return t;
    std::unique_ptr<uint8_t[]> eb(new uint8_t[bl]), er(new uint8_t[rl]);
    size_t bl2 = 0, rl2 = 0;
    rc = wc_split_tol_unit(in.get(), p.bytes.size(), tol, eb.get(), bl, &bl2, er.get(), rl, &rl2, nullptr, nullptr);
    CHECK(rc == WC_OK && bl2 == bl && rl2 == rl && std::memcmp(er.get(), big2.get(), rl) == 0, "%s: exact split", what);
    if (rl > 20) {
        std::unique_ptr<uint8_t[]> sr(new uint8_t[rl - 1]);
        rc = wc_split_tol_unit(in.get(), p.bytes.size(), tol, eb.get(), bl, &bl2, sr.get(), rl - 1, &rl2, nullptr, nullptr);
        CHECK(rc == WC_ERR_INVALID, "%s: short rest", what);
    }
    t.rest.assign(big2.get(), big2.get() + rl);
    t.ok = true;
    return t;
}

static double weighted_rms(const std::vector<uint32_t>& A, const std::vector<int>& lv) {
    double s = 0.0;
    for (size_t q = 0; q < A.size(); ++q) {
        float v;
        std::memcpy(&v, &A[q], 4);
        if (std::isfinite(v)) s += std::pow(8.0, lv[q] + 1) * (double)v * (double)v;
    }
    return A.empty() ? 0.0 : std::sqrt(s / (double)A.size());
}

static void test_rule(const std::vector<Pay>& pays) {
    const double inf = std::numeric_limits<double>::infinity();
    for (size_t i = 0; i < pays.size(); ++i) {
        const Pay& p = pays[i];
        std::vector<uint32_t> A;
        std::vector<int> lv;
        dense_of(p, A, lv);
        const double rms = weighted_rms(A, lv);
        // the counts of the forward's rule on A: every entry, zeros included; NaN nowhere
        std::vector<uint64_t> cnt((size_t)p.L * WC_HIST_BINS, 0);
        for (size_t q = 0; q < A.size(); ++q) {
            const uint32_t m = A[q] & 0x7fffffffu;
            if (m <= 0x7f800000u) ++cnt[(size_t)lv[q] * WC_HIST_BINS + (m >> WC_HIST_SHIFT)];
        }
        const Bytes canon = emit(p, A, [&](size_t q) { return candidate(A[q]); });
        for (double tol : {0.0, 1e-6 * rms, 0.01 * rms, 0.2 * rms, 0.7 * rms, 1.5 * rms, inf}) {
            char what[96];
            std::snprintf(what, sizeof what, "payload %zu tol %g", i, tol);
            const Thinned t = thin_exact(p, tol, what);
            if (!t.ok) continue;
            float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
            double bound = -1.0;
            CHECK(wc_tol_levels_threshold(cnt.data(), p.L, A.size(), tol, th, &bound) == WC_OK, "%s: the rule", what);
            CHECK(std::memcmp(th, t.th, sizeof(float) * p.L) == 0 && std::memcmp(&bound, &t.bound, 8) == 0,
                  "%s: thresholds / bound %g / %g", what, t.bound, bound);
            CHECK(t.bound <= tol, "%s: bound %g", what, t.bound);
            auto kept = [&](size_t q) {
                float v;
                const uint32_t m = A[q] & 0x7fffffffu;
                std::memcpy(&v, &m, 4);
                return v > th[lv[q]];  // strict: false for NaN
            };
            CHECK(t.bytes == emit(p, A, kept), "%s: the kept set", what);
            CHECK(t.rest == emit(p, A, [&](size_t q) { return candidate(A[q]) && !kept(q); }), "%s: the rest", what);
            if (tol == 0.0) CHECK(t.bytes == canon, "%s: tol = 0 is the canonical form", what);
            Bytes merged(canon.size());
            size_t ml = 0;
            const int rc = wc_merge_unit(t.bytes.data(), t.bytes.size(), t.rest.data(), t.rest.size(), merged.data(),
                                         merged.size(), &ml);
            CHECK(rc == WC_OK && ml == canon.size() && merged == canon, "%s: merge(split) == canon", what);
        }
    }
    // refusals
    const Pay& p = pays[1];
    Bytes out(p.bytes.size()), out2(p.bytes.size());
    size_t w = 0, w2 = 0;
    CHECK(wc_thin_tol_unit(p.bytes.data(), p.bytes.size(), NAN, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "NaN");
    CHECK(wc_thin_tol_unit(p.bytes.data(), p.bytes.size(), -1.0, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "negative");
    CHECK(wc_split_tol_unit(p.bytes.data(), p.bytes.size(), NAN, out.data(), out.size(), &w, out2.data(), out2.size(), &w2, nullptr,
                            nullptr) == WC_ERR_INVALID, "split NaN");
    CHECK(wc_thin_tol_unit(p.bytes.data(), p.bytes.size() - 8, 0.5, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "short");
    CHECK(wc_thin_tol_unit(p.bytes.data(), p.bytes.size(), 0.5, nullptr, out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "null out");
    Bytes bad = p.bytes;
    const int32_t m1 = -1;
    std::memcpy(bad.data() + 28, &m1, 4);
    CHECK(wc_thin_tol_unit(bad.data(), bad.size(), 0.5, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_FORMAT, "negative run");
    bad = p.bytes;
    const int32_t tag = -9;
    std::memcpy(bad.data() + 12, &tag, 4);
    CHECK(wc_thin_tol_unit(bad.data(), bad.size(), 0.5, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_FORMAT, "ncoeff field");
    Rng r{0x0dd};
    const Pay odd = make_payload(r, 3, 5, 7, 1, 60, 4);  // an odd L = 1 box with cells
    CHECK(wc_thin_tol_unit(odd.bytes.data(), odd.bytes.size(), 0.5, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "odd box");
}

static void test_drivers(const std::vector<Pay>& pays) {
    const int n = (int)pays.size();
    std::vector<wc_unit> units(n);
    std::vector<int32_t> levels(n);
    std::vector<uint64_t> offsets(n);
    std::vector<double> tol(n);
    uint64_t cur = 8;
    for (int i = 0; i < n; ++i) {
        units[i] = wc_unit{0, pays[i].W, pays[i].H, pays[i].D, 0};
        levels[i] = pays[i].L;
        cur = (cur + 7) / 8 * 8 + (i % 2 ? 4 : 0) + 8 * (uint64_t)(i % 3);
        offsets[i] = cur;
        cur += pays[i].bytes.size();
    }
    std::unique_ptr<uint8_t[]> buf(new uint8_t[cur]);  // exactly to the last payload's end
    std::memset(buf.get(), 0xa5, cur);
    for (int i = 0; i < n; ++i) std::memcpy(buf.get() + offsets[i], pays[i].bytes.data(), pays[i].bytes.size());
    std::vector<Thinned> want(n);
    for (int i = 0; i < n; ++i) {
        std::vector<uint32_t> A;
        std::vector<int> lv;
        dense_of(pays[i], A, lv);
        const double fr[] = {0.3, 0.0, 0.05, std::numeric_limits<double>::infinity(), 0.9};
        tol[i] = fr[i % 5] == 0.0 || std::isinf(fr[i % 5]) ? fr[i % 5] : fr[i % 5] * weighted_rms(A, lv);
        want[i] = thin_exact(pays[i], tol[i], "driver reference");
    }
    uint64_t bcap = 0, rcap = 0;
    CHECK(wc_split_bound(units.data(), n, nullptr, &bcap, &rcap) == WC_OK && bcap == wc_thin_bound(units.data(), n, nullptr),
          "the bounds");
    for (int64_t chunk : {int64_t(0), int64_t(700), int64_t(1) << 25}) {
        for (int form = 0; form < 8; ++form) {  // thin / split x levels given / from the headers x thresh and bound asked for / null
            const bool split = form & 1, nulls = form & 4;
            const int32_t* lv = form & 2 ? levels.data() : nullptr;
            wc_ctx* c = make_ctx();
            c->opt_host_chunk = chunk;
            std::unique_ptr<uint8_t[]> out(new uint8_t[bcap]), rest(new uint8_t[rcap]);
            std::memset(out.get(), 0x5a, bcap);
            std::memset(rest.get(), 0x5a, rcap);
            std::unique_ptr<uint64_t[]> ooff(new uint64_t[n + 1]), roff(new uint64_t[n + 1]);
            std::unique_ptr<uint32_t[]> kept(new uint32_t[n]), rp(new uint32_t[n]);
            std::unique_ptr<float[]> tout(new float[(size_t)n * WC_MAX_LEVELS]);
            std::unique_ptr<double[]> bout(new double[n]);
            auto call = [&](const wc_unit* us, const double* tl, uint64_t cap, uint64_t cap2) {
                float* th = nulls ? nullptr : tout.get();
                double* bd = nulls ? nullptr : bout.get();
                return split ? wc_split_tol_host(c, buf.get(), offsets.data(), us, n, lv, tl, out.get(), cap, ooff.get(),
                                                 kept.get(), rest.get(), cap2, roff.get(), rp.get(), th, bd)
                             : wc_thin_tol_host(c, buf.get(), offsets.data(), us, n, lv, tl, out.get(), cap, ooff.get(),
                                                kept.get(), th, bd);
            };
            const int rc = call(units.data(), tol.data(), bcap, rcap);
            CHECK(rc == WC_OK, "driver form %d chunk %lld: rc %d %s", form, (long long)chunk, rc, c->err.c_str());
            uint64_t o = 4, ro = 4;
            for (int i = 0; i < n && rc == WC_OK; ++i) {
                const Thinned& w = want[i];
                CHECK(ooff[i] == o && 20 + 8ull * kept[i] == w.bytes.size(), "form %d unit %d: offset, kept", form, i);
                CHECK(o + w.bytes.size() <= bcap && std::memcmp(out.get() + o, w.bytes.data(), w.bytes.size()) == 0,
                      "form %d unit %d: bytes", form, i);
                o += (i + 1 < n ? 24 : 20) + 8ull * kept[i];
                if (split) {
                    CHECK(roff[i] == ro && 20 + 8ull * rp[i] == w.rest.size(), "form %d unit %d: rest offset, pairs", form, i);
                    CHECK(ro + w.rest.size() <= rcap && std::memcmp(rest.get() + ro, w.rest.data(), w.rest.size()) == 0,
                          "form %d unit %d: rest bytes", form, i);
                    ro += (i + 1 < n ? 24 : 20) + 8ull * rp[i];
                }
                if (!nulls) {
                    CHECK(std::memcmp(&bout[i], &w.bound, 8) == 0, "unit %d bound", i);
                    for (int l = 0; l < WC_MAX_LEVELS; ++l) {
                        const float t = l < pays[i].L ? w.th[l] : 0.0f;
                        CHECK(std::memcmp(&tout[(size_t)i * WC_MAX_LEVELS + l], &t, 4) == 0, "unit %d thresh %d", i, l);
                    }
                }
            }
            if (rc == WC_OK) CHECK(ooff[n] == o && (!split || roff[n] == ro), "form %d: the end", form);
            // before anything runs, outputs untouched: a capacity one byte short, a NaN tolerance, a header that disagrees
            std::memset(out.get(), 0x5a, bcap);
            std::memset(rest.get(), 0x5a, rcap);
            auto clean = [&] {
                return std::all_of(out.get(), out.get() + bcap, [](uint8_t b) { return b == 0x5a; }) &&
                       std::all_of(rest.get(), rest.get() + rcap, [](uint8_t b) { return b == 0x5a; });
            };
            int r2 = call(units.data(), tol.data(), bcap - 1, rcap);
            CHECK(r2 == WC_ERR_INVALID && clean(), "short capacity: %d", r2);
            if (split) {
                r2 = call(units.data(), tol.data(), bcap, rcap - 1);
                CHECK(r2 == WC_ERR_INVALID && clean(), "short rest capacity: %d", r2);
            }
            std::vector<double> badtol = tol;
            badtol[n / 2] = NAN;
            r2 = call(units.data(), badtol.data(), bcap, rcap);
            CHECK(r2 == WC_ERR_INVALID && clean() && c->err.find("unit " + std::to_string(n / 2)) != std::string::npos,
                  "NaN tolerance: %d %s", r2, c->err.c_str());
            std::vector<wc_unit> other = units;
            std::swap(other[2].ny, other[2].nz);
            r2 = call(other.data(), tol.data(), bcap, rcap);
            CHECK(r2 == WC_ERR_FORMAT && clean(), "mismatched header: %d", r2);
            destroy_ctx(c);
        }
    }
    g_tabs.clear();
}

int main() {
    Rng r{0x7018};
    std::vector<Pay> pays;
    pays.push_back(make_payload(r, 8, 8, 8, 3, 300, 3));
    pays.push_back(make_payload(r, 16, 8, 4, 2, 200, 6));
    pays.push_back(make_payload(r, 6, 10, 14, 1, 260, 4));
    pays.push_back(make_payload(r, 16, 16, 16, 4, 4200, 1));  // surplus pairs
    pays.push_back(make_payload(r, 0, 4, 4, 1, 0, 0));
    pays.push_back(make_payload(r, 4, 4, 4, 2, 0, 0));
    pays.push_back(make_payload(r, 12, 20, 8, 1, 1900, 0));
    pays.push_back(make_payload(r, 48, 16, 80, 4, 9000, 9));
    test_rule(pays);
    test_drivers(pays);
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
