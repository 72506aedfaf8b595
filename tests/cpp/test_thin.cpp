// test_thin.cpp — the host side of the compressed-domain thinning on the CPU, for the
// ASan + UBSan build (`make thinsan`, run by tests/test_thin_san.py): wc_thin_unit
// (wc_thinrule.cpp) and the host drivers wc_thin_budget_host / wc_thin_thresh_host
// (wc_thinhost.cpp, on wc_hostserial.cpp's driver) over the fake HIP runtime of tests/cpp/fake_device.cpp.  No GPU
// and no kernel: the device entry point the drivers call (wc::thin_device) is
// restated here on wc_thin_unit, into wc_forward's slot layout, as the real one
// writes it.  Every buffer the rule or a driver reads or writes is a heap block of
// exactly the documented size, so a read or write past one is reported.
//
//   rule     wc_thin_unit on seeded payloads (runs that overshoot, surplus pairs,
//            values +-0, NaN, +-inf, subnormals) at budgets 0, 1, c - 1, c, c + 1
//            and the thresholds of each T: output capacity exactly 20 + 8 kept
//            (one byte less: WC_ERR_INVALID, nothing written); kept <= K; the
//            thresholds of T keep the same bytes; idempotence; a brute-force
//            restatement of the budget rule on the dense array gives the same T
//            and kept count; the refusals.
//   drivers  the same payloads as one batch with gaps between them, levels from
//            the headers and given, WC_OPT_HOST_CHUNK 0 / small (several runs):
//            packed offsets, kept, bytes equal to wc_thin_unit's, thresholds and
//            keys; out_capacity one byte short; a header that disagrees
//            (WC_ERR_FORMAT before anything runs, outputs untouched).
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

extern "C" uint64_t wc_thin_bound(const wc_unit* units, int n, const uint32_t* max_pairs) {  // wc_capi.cpp's
    uint64_t b = 4;
    for (int i = 0; i < n; ++i) {
        const uint64_t N = (uint64_t)units[i].nx * units[i].ny * units[i].nz;
        b += 24 + 8 * (max_pairs ? std::min<uint64_t>(max_pairs[i], N) : N);
    }
    return b;
}

namespace {
std::vector<std::unique_ptr<std::vector<UnitDev>>> g_tabs;  // launch_pack reads the slots from these
}

// The device call, restated: after the uploads, unit u through wc_thin_unit into its slot.
namespace wc {
int thin_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_out,
                uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_kept, float* d_thresh, uint32_t* d_key) {
    if (!full_slots) return fail(c, WC_ERR_INVALID, "fake: the drivers ask for wc_forward's slots");
    if (out_capacity < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "out_capacity");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return WC_ERR_HIP;
    g_tabs.emplace_back(new std::vector<UnitDev>(n));
    std::vector<UnitDev>& tab = *g_tabs.back();
    c->plan.d_units.p = tab.data();
    uint64_t slot = 4;
    for (int u = 0; u < n; ++u) {
        const uint64_t N = (uint64_t)units[u].nx * units[u].ny * units[u].nz;
        tab[u].pay_off = slot;
        const uint8_t* p = d_payload + d_offsets[u];
        int32_t nrle;
        std::memcpy(&nrle, p + 16, 4);
        size_t written = 0;
        uint32_t key = 0;
        float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
        const int rc = wc_thin_unit(p, 20 + 8ull * (uint64_t)nrle, max_pairs ? max_pairs + u : nullptr,
                                    thresh ? thresh + (size_t)WC_MAX_LEVELS * u : nullptr, d_out + slot, 20 + 8 * N,
                                    &written, &key, th);
        if (rc != WC_OK) return fail(c, rc, "fake: wc_thin_unit refused unit " + std::to_string(u));
        (void)levels;
        d_out_offsets[u] = slot;
        d_kept[u] = (uint32_t)((written - 20) / 8);
        if (d_key) d_key[u] = key;
        if (d_thresh) std::memcpy(d_thresh + (size_t)WC_MAX_LEVELS * u, th, sizeof th);
        if (u == n - 1) d_out_offsets[n] = slot + written;
        slot += 24 + 8 * N;
    }
    c->err_check_pending = true;
    return WC_OK;
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
                          &c->h_thresh, &c->h_bound, &c->pk_off})
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

struct Pay {
    int32_t W, H, D, L;
    std::vector<uint8_t> bytes;  // exactly 20 + 8 nrle
};

static Pay make_payload(Rng& r, int32_t W, int32_t H, int32_t D, int L, uint32_t n, uint32_t max_run) {
    Pay p{W, H, D, L, std::vector<uint8_t>(20 + 8ull * n)};
    const int64_t N = (int64_t)W * H * D;
    const int32_t h[5] = {W, H, D, L >= 2 ? -L : (int32_t)N, (int32_t)n};
    std::memcpy(p.bytes.data(), h, 20);
    static const uint32_t special[] = {0u, 0x80000000u, 0x7FC00000u, 0xFF800001u, 0x7F800000u, 0xFF800000u, 1u, 0x80000003u};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t c = r.next() % 100;
        int32_t run = (int32_t)(r.next() % (max_run + 1));
        if (c == 0) run = 0x7fffffff;  // overshoots
        uint32_t bits;
        if (c < 8) {
            bits = special[r.next() % 8];
        } else {
            const float v = (float)((int)(r.next() % 2001) - 1000) * 0.03125f + 0.5f;
            std::memcpy(&bits, &v, 4);
            if (c < 30) bits = (bits & 0x80000000u) | 0x40500000u;  // ties
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

struct Thinned {
    std::vector<uint8_t> bytes;
    uint32_t key = 0;
    float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
};

// wc_thin_unit with exact-size heap buffers
static Thinned thin_exact(const Pay& p, const uint32_t* K, const float* th, const char* what) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[p.bytes.size()]);
    std::memcpy(in.get(), p.bytes.data(), p.bytes.size());
    std::unique_ptr<uint8_t[]> big(new uint8_t[p.bytes.size()]);
    size_t w = 0;
    Thinned t;
    std::unique_ptr<float[]> tl(new float[p.L]);
    int rc = wc_thin_unit(in.get(), p.bytes.size(), K, th, big.get(), p.bytes.size(), &w, &t.key, tl.get());
    CHECK(rc == WC_OK && w >= 20 && w <= p.bytes.size() && (w - 20) % 8 == 0, "%s rc %d", what, rc);
    if (rc != WC_OK) return t;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[w]);
    size_t w2 = 0;
    rc = wc_thin_unit(in.get(), p.bytes.size(), K, th, exact.get(), w, &w2, nullptr, nullptr);
    CHECK(rc == WC_OK && w2 == w && std::memcmp(exact.get(), big.get(), w) == 0, "%s exact capacity", what);
    size_t w3 = 77;
    std::unique_ptr<uint8_t[]> small(new uint8_t[w - 1]);
    std::memset(small.get(), 0x5a, w - 1);
    rc = wc_thin_unit(in.get(), p.bytes.size(), K, th, small.get(), w - 1, &w3, nullptr, nullptr);
    CHECK(rc == WC_ERR_INVALID && w3 == 77 && std::all_of(small.get(), small.get() + w - 1, [](uint8_t b) { return b == 0x5a; }),
          "%s short capacity", what);
    t.bytes.assign(exact.get(), exact.get() + w);
    std::memcpy(t.th, tl.get(), sizeof(float) * p.L);
    return t;
}

static void test_rule(const std::vector<Pay>& pays) {
    for (size_t i = 0; i < pays.size(); ++i) {
        const Pay& p = pays[i];
        std::vector<uint32_t> A;
        std::vector<int> lv;
        dense_of(p, A, lv);
        std::vector<uint32_t> keys;
        for (size_t q = 0; q < A.size(); ++q) {
            const uint32_t m = A[q] & 0x7fffffffu;
            if (m >= 1u && m <= 0x7f800000u) keys.push_back(m + ((uint32_t)(WC_LTOL_SHIFT * lv[q]) << WC_HIST_SHIFT));
        }
        std::sort(keys.begin(), keys.end(), std::greater<uint32_t>());
        const uint32_t c = (uint32_t)keys.size();
        for (uint32_t K : {0u, 1u, c ? c - 1 : 0u, c, c + 1, c / 2, c / 3, 0xffffffffu}) {
            char what[96];
            std::snprintf(what, sizeof what, "payload %zu K %u", i, K);
            const Thinned t = thin_exact(p, &K, nullptr, what);
            if (t.bytes.empty()) continue;
            const uint32_t T = c > K ? keys[K] : 0u;
            const uint32_t kept = (uint32_t)std::count_if(keys.begin(), keys.end(), [T](uint32_t k) { return k > T; });
            int32_t nk;
            std::memcpy(&nk, t.bytes.data() + 16, 4);
            CHECK(t.key == T && (uint32_t)nk == kept && kept <= K, "%s: T %x / %x kept %d / %u", what, t.key, T, nk, kept);
            CHECK(t.bytes.size() == 20 + 8ull * kept && std::memcmp(t.bytes.data(), p.bytes.data(), 16) == 0, "%s header", what);
            // the kept pairs are exactly the entries of A with key > T, in order
            uint64_t pos = 0, q = 0;
            bool same = true;
            for (uint32_t k = 0; k < kept && same; ++k) {
                int32_t run;
                uint32_t b;
                std::memcpy(&run, t.bytes.data() + 20 + 8ull * k, 4);
                std::memcpy(&b, t.bytes.data() + 24 + 8ull * k, 4);
                pos += (uint64_t)run;
                for (;; ++q) {
                    const uint32_t m = q < A.size() ? A[q] & 0x7fffffffu : 1u;
                    if (q >= A.size() || (m >= 1u && m <= 0x7f800000u &&
                                          m + ((uint32_t)(WC_LTOL_SHIFT * lv[q]) << WC_HIST_SHIFT) > T))
                        break;
                }
                same = run >= 0 && q < A.size() && pos == q && A[q] == b;
                ++pos;
                ++q;
            }
            CHECK(same, "%s: the kept set", what);
            // the thresholds of T keep the same bytes; both forms are idempotent
            const Thinned u = thin_exact(p, nullptr, t.th, what);
            CHECK(u.bytes == t.bytes, "%s: thresholds of T", what);
            Pay again{p.W, p.H, p.D, p.L, t.bytes};
            CHECK(thin_exact(again, &K, nullptr, what).bytes == t.bytes, "%s: idempotent (budget)", what);
            CHECK(thin_exact(again, nullptr, t.th, what).bytes == t.bytes, "%s: idempotent (thresholds)", what);
        }
    }
    // refusals
    const Pay& p = pays[1];
    std::vector<uint8_t> out(p.bytes.size());
    size_t w = 0;
    const uint32_t K = 3;
    const float th[4] = {0.f, 0.f, 0.f, 0.f}, nan[4] = {NAN, 0.f, 0.f, 0.f}, neg[4] = {-1.f, 0.f, 0.f, 0.f};
    CHECK(wc_thin_unit(p.bytes.data(), p.bytes.size(), nullptr, nullptr, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "neither");
    CHECK(wc_thin_unit(p.bytes.data(), p.bytes.size(), &K, th, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "both");
    CHECK(wc_thin_unit(p.bytes.data(), p.bytes.size(), nullptr, nan, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "NaN");
    CHECK(wc_thin_unit(p.bytes.data(), p.bytes.size(), nullptr, neg, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "negative");
    CHECK(wc_thin_unit(p.bytes.data(), p.bytes.size() - 8, &K, nullptr, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_INVALID, "short");
    std::vector<uint8_t> bad = p.bytes;
    const int32_t m1 = -1;
    std::memcpy(bad.data() + 28, &m1, 4);
    CHECK(wc_thin_unit(bad.data(), bad.size(), &K, nullptr, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_FORMAT, "negative run");
    bad = p.bytes;
    const int32_t tag = -9;
    std::memcpy(bad.data() + 12, &tag, 4);
    CHECK(wc_thin_unit(bad.data(), bad.size(), &K, nullptr, out.data(), out.size(), &w, nullptr, nullptr) == WC_ERR_FORMAT, "ncoeff field");
}

static void test_drivers(const std::vector<Pay>& pays) {
    const int n = (int)pays.size();
    std::vector<wc_unit> units(n);
    std::vector<int32_t> levels(n);
    std::vector<uint64_t> offsets(n);
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
    std::vector<uint32_t> K(n);
    std::vector<float> th((size_t)n * WC_MAX_LEVELS, 0.f);
    std::vector<Thinned> wb(n), wt(n);
    for (int i = 0; i < n; ++i) {
        int32_t nr;
        std::memcpy(&nr, pays[i].bytes.data() + 16, 4);
        K[i] = (uint32_t)nr / 3 + (uint32_t)i;
        wb[i] = thin_exact(pays[i], &K[i], nullptr, "driver reference");
        std::memcpy(&th[(size_t)i * WC_MAX_LEVELS], wb[i].th, sizeof(float) * pays[i].L);
        wt[i] = thin_exact(pays[i], nullptr, &th[(size_t)i * WC_MAX_LEVELS], "driver reference");
    }
    for (int64_t chunk : {int64_t(0), int64_t(700), int64_t(1) << 25}) {
        for (int form = 0; form < 4; ++form) {  // budget / thresholds x levels given / from the headers
            const bool budget = form < 2;
            const int32_t* lv = form % 2 ? levels.data() : nullptr;
            wc_ctx* c = make_ctx();
            c->opt_host_chunk = chunk;
            const uint64_t cap = wc_thin_bound(units.data(), n, budget ? K.data() : nullptr);
            std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
            std::memset(out.get(), 0x5a, cap);
            std::unique_ptr<uint64_t[]> ooff(new uint64_t[n + 1]);
            std::unique_ptr<uint32_t[]> kept(new uint32_t[n]), key(new uint32_t[n]);
            std::unique_ptr<float[]> tout(new float[(size_t)n * WC_MAX_LEVELS]);
            const int rc = budget ? wc_thin_budget_host(c, buf.get(), offsets.data(), units.data(), n, lv, K.data(), out.get(),
                                                        cap, ooff.get(), kept.get(), tout.get(), key.get())
                                  : wc_thin_thresh_host(c, buf.get(), offsets.data(), units.data(), n, lv, th.data(),
                                                        out.get(), cap, ooff.get(), kept.get());
            CHECK(rc == WC_OK, "driver form %d chunk %lld: rc %d %s", form, (long long)chunk, rc, c->err.c_str());
            uint64_t o = 4;
            for (int i = 0; i < n && rc == WC_OK; ++i) {
                const Thinned& w = budget ? wb[i] : wt[i];
                CHECK(ooff[i] == o && 20 + 8ull * kept[i] == w.bytes.size(), "form %d unit %d: offset, kept", form, i);
                CHECK(o + w.bytes.size() <= cap && std::memcmp(out.get() + o, w.bytes.data(), w.bytes.size()) == 0,
                      "form %d unit %d: bytes", form, i);
                if (budget) {
                    CHECK(key[i] == w.key, "unit %d key", i);
                    for (int l = 0; l < WC_MAX_LEVELS; ++l) {
                        const float want = l < pays[i].L ? w.th[l] : 0.0f;
                        CHECK(std::memcmp(&tout[(size_t)i * WC_MAX_LEVELS + l], &want, 4) == 0, "unit %d thresh %d", i, l);
                    }
                }
                o += (i + 1 < n ? 24 : 20) + 8ull * kept[i];
            }
            if (rc == WC_OK) CHECK(ooff[n] == o, "form %d: the end", form);
            // one byte short of the bound; a header that disagrees: before anything runs, outputs untouched
            std::memset(out.get(), 0x5a, cap);
            int r2 = budget ? wc_thin_budget_host(c, buf.get(), offsets.data(), units.data(), n, lv, K.data(), out.get(),
                                                  cap - 1, ooff.get(), kept.get(), nullptr, nullptr)
                            : wc_thin_thresh_host(c, buf.get(), offsets.data(), units.data(), n, lv, th.data(), out.get(),
                                                  cap - 1, ooff.get(), kept.get());
            CHECK(r2 == WC_ERR_INVALID, "short capacity: %d", r2);
            std::vector<wc_unit> other = units;
            std::swap(other[2].ny, other[2].nz);
            r2 = budget ? wc_thin_budget_host(c, buf.get(), offsets.data(), other.data(), n, lv, K.data(), out.get(), cap,
                                              ooff.get(), kept.get(), nullptr, nullptr)
                        : wc_thin_thresh_host(c, buf.get(), offsets.data(), other.data(), n, lv, th.data(), out.get(), cap,
                                              ooff.get(), kept.get());
            CHECK(r2 == WC_ERR_FORMAT && std::all_of(out.get(), out.get() + cap, [](uint8_t b) { return b == 0x5a; }),
                  "mismatched header: %d", r2);
            destroy_ctx(c);
        }
    }
    g_tabs.clear();
}

int main() {
    Rng r{0x7417};
    std::vector<Pay> pays;
    pays.push_back(make_payload(r, 8, 8, 8, 3, 300, 3));
    pays.push_back(make_payload(r, 16, 8, 4, 2, 200, 6));
    pays.push_back(make_payload(r, 3, 5, 7, 1, 60, 4));
    pays.push_back(make_payload(r, 16, 16, 16, 4, 4200, 1));  // surplus pairs
    pays.push_back(make_payload(r, 0, 4, 4, 1, 0, 0));
    pays.push_back(make_payload(r, 4, 4, 4, 2, 0, 0));
    pays.push_back(make_payload(r, 12, 20, 8, 1, 1900, 0));
    test_rule(pays);
    test_drivers(pays);
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
