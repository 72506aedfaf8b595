// test_layers.cpp — the host side of the progressive layers on the CPU, for the
// ASan + UBSan build (`make layersan`, run by tests/test_layers_san.py): wc_split_unit
// and wc_merge_unit (wc_layersrule.cpp) and the host drivers wc_split_budget_host /
// wc_split_thresh_host / wc_merge_host (wc_layershost.cpp, on wc_hostserial.cpp's
// driver with its second stream) over the fake HIP runtime of tests/cpp/fake_device.cpp.
// No GPU and no kernel: the device entry points the drivers call (wc::split_device,
// wc::merge_device) are restated here on the rule, into wc_forward's slot layout, as
// the real ones write it.  Every buffer the rule or a driver reads or writes is a heap
// block of exactly the documented size, so a read or write past one is reported.
//
//   rule     wc_split_unit on seeded payloads (runs that overshoot, surplus pairs,
//            values +-0, NaN, +-inf, subnormals, ties) at budgets 0, 1, c - 1, c, c + 1,
//            c / 2 and the thresholds of each T: capacities exactly 20 + 8 pairs (one
//            byte less on either side: WC_ERR_INVALID, nothing written); base ==
//            wc_thin_unit's bytes, T and thresholds; base and rest disjoint, together
//            the pairs of canon(P); wc_merge_unit(base, rest) == canon(P) in both
//            orders at the exact capacity; three layers in both groupings; the refusals
//            (overlap at the first, a middle and the last pair, headers that differ,
//            a negative run, a short input).
//   drivers  the same payloads as one batch with gaps between them, levels from the
//            headers and given, WC_OPT_HOST_CHUNK 0 / small (several runs): both packed
//            outputs equal to the rule's; wc_merge_host of the two layers == canon(P);
//            a capacity one byte short; a header that disagrees (WC_ERR_FORMAT before
//            anything runs, outputs untouched).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// The device calls, restated: after the uploads, unit u through the rule into its slots.
namespace wc {
int split_device(wc_ctx* c, const uint8_t* d_payload, const uint64_t* d_offsets, const wc_unit* units, int n,
                 const int32_t* levels, const uint32_t* max_pairs, const float* thresh, bool full_slots, uint8_t* d_base,
                 uint64_t base_capacity, uint64_t* d_base_offsets, uint32_t* d_kept, const SplitOut& rest,
                 float* d_thresh, uint32_t* d_key) {
    (void)levels;
    if (!full_slots) return fail(c, WC_ERR_INVALID, "fake: the drivers ask for wc_forward's slots");
    if (base_capacity < wc_payload_bound(units, n) || rest.capacity < wc_payload_bound(units, n))
        return fail(c, WC_ERR_INVALID, "capacity");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return WC_ERR_HIP;
    const std::vector<UnitDev>& tab = slot_table(c, units, n);
    for (int u = 0; u < n; ++u) {
        const uint64_t N = (uint64_t)units[u].nx * units[u].ny * units[u].nz, slot = tab[u].pay_off;
        const uint8_t* p = d_payload + d_offsets[u];
        size_t bl = 0, rl = 0;
        uint32_t key = 0;
        float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
        const int rc = wc_split_unit(p, unit_len(p), max_pairs ? max_pairs + u : nullptr,
                                     thresh ? thresh + (size_t)WC_MAX_LEVELS * u : nullptr, d_base + slot, 20 + 8 * N, &bl,
                                     rest.d_rest + slot, 20 + 8 * N, &rl, &key, th);
        if (rc != WC_OK) return fail(c, rc, "fake: wc_split_unit refused unit " + std::to_string(u));
        d_base_offsets[u] = rest.d_offsets[u] = slot;
        d_kept[u] = (uint32_t)((bl - 20) / 8);
        rest.d_pairs[u] = (uint32_t)((rl - 20) / 8);
        if (d_key) d_key[u] = key;
        if (d_thresh) std::memcpy(d_thresh + (size_t)WC_MAX_LEVELS * u, th, sizeof th);
        if (u == n - 1) {
            d_base_offsets[n] = slot + bl;
            rest.d_offsets[n] = slot + rl;
        }
    }
    c->err_check_pending = true;
    return WC_OK;
}

int merge_device(wc_ctx* c, const uint8_t* d_a, const uint64_t* d_a_offsets, const uint8_t* d_b,
                 const uint64_t* d_b_offsets, const wc_unit* units, int n, const int32_t* levels, uint8_t* d_out,
                 uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_pairs) {
    (void)levels;
    if (out_capacity < wc_payload_bound(units, n)) return fail(c, WC_ERR_INVALID, "out_capacity");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return WC_ERR_HIP;
    const std::vector<UnitDev>& tab = slot_table(c, units, n);
    for (int u = 0; u < n; ++u) {
        const uint64_t N = (uint64_t)units[u].nx * units[u].ny * units[u].nz, slot = tab[u].pay_off;
        const uint8_t *pa = d_a + d_a_offsets[u], *pb = d_b + d_b_offsets[u];
        size_t w = 0;
        const int rc = wc_merge_unit(pa, unit_len(pa), pb, unit_len(pb), d_out + slot, 20 + 8 * N, &w);
        if (rc != WC_OK) return fail(c, rc, "fake: wc_merge_unit refused unit " + std::to_string(u));
        d_out_offsets[u] = slot;
        d_pairs[u] = (uint32_t)((w - 20) / 8);
        if (u == n - 1) d_out_offsets[n] = slot + w;
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

// a copy in a heap block of exactly its size
static std::unique_ptr<uint8_t[]> exact_copy(const Bytes& b) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[b.size()]);
    std::memcpy(p.get(), b.data(), b.size());
    return p;
}

// (position, bits) of the pairs below N, by the definition
static std::vector<std::pair<uint64_t, uint32_t>> pairs_of(const Bytes& b) {
    int32_t h[5];
    std::memcpy(h, b.data(), 20);
    const uint64_t N = (uint64_t)h[0] * h[1] * h[2];
    std::vector<std::pair<uint64_t, uint32_t>> out;
    uint64_t pos = 0;
    for (int32_t k = 0; k < h[4]; ++k) {
        int32_t run;
        uint32_t v;
        std::memcpy(&run, b.data() + 20 + 8ull * k, 4);
        std::memcpy(&v, b.data() + 24 + 8ull * k, 4);
        pos += (uint64_t)run;
        if (pos >= N) break;
        out.emplace_back(pos++, v);
    }
    return out;
}

static Bytes thin_of(const Bytes& p, const uint32_t* K, const float* th, uint32_t* key, float* tout) {
    Bytes out(p.size());
    size_t w = 0;
    const int rc = wc_thin_unit(p.data(), p.size(), K, th, out.data(), out.size(), &w, key, tout);
    CHECK(rc == WC_OK, "wc_thin_unit rc %d", rc);
    out.resize(rc == WC_OK ? w : 0);
    return out;
}

struct Split {
    Bytes base, rest;
    uint32_t key = 0;
    float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
};

// wc_split_unit with exact-size heap buffers
static Split split_exact(const Pay& p, const uint32_t* K, const float* th, const char* what) {
    const std::unique_ptr<uint8_t[]> in = exact_copy(p.bytes);
    const size_t len = p.bytes.size();
    std::unique_ptr<uint8_t[]> b0(new uint8_t[len]), r0(new uint8_t[len]);
    size_t bl = 0, rl = 0;
    Split s;
    std::unique_ptr<float[]> tl(new float[p.L]);
    int rc = wc_split_unit(in.get(), len, K, th, b0.get(), len, &bl, r0.get(), len, &rl, &s.key, tl.get());
    CHECK(rc == WC_OK && bl >= 20 && rl >= 20 && bl + rl - 20 <= len, "%s rc %d", what, rc);
    if (rc != WC_OK) return s;
    std::unique_ptr<uint8_t[]> b1(new uint8_t[bl]), r1(new uint8_t[rl]);
    size_t bl1 = 0, rl1 = 0;
    rc = wc_split_unit(in.get(), len, K, th, b1.get(), bl, &bl1, r1.get(), rl, &rl1, nullptr, nullptr);
    CHECK(rc == WC_OK && bl1 == bl && rl1 == rl && !std::memcmp(b1.get(), b0.get(), bl) && !std::memcmp(r1.get(), r0.get(), rl),
          "%s exact capacities", what);
    for (int side = 0; side < 2; ++side) {  // one byte short on either side: nothing written
        const size_t bc = bl - (side == 0), rc2 = rl - (side == 1);
        std::unique_ptr<uint8_t[]> b2(new uint8_t[bc]), r2(new uint8_t[rc2]);
        std::memset(b2.get(), 0x5a, bc);
        std::memset(r2.get(), 0x5a, rc2);
        size_t x = 77, y = 78;
        rc = wc_split_unit(in.get(), len, K, th, b2.get(), bc, &x, r2.get(), rc2, &y, nullptr, nullptr);
        CHECK(rc == WC_ERR_INVALID && x == 77 && y == 78 &&
                  std::all_of(b2.get(), b2.get() + bc, [](uint8_t v) { return v == 0x5a; }) &&
                  std::all_of(r2.get(), r2.get() + rc2, [](uint8_t v) { return v == 0x5a; }),
              "%s short capacity (side %d): %d", what, side, rc);
    }
    s.base.assign(b0.get(), b0.get() + bl);
    s.rest.assign(r0.get(), r0.get() + rl);
    std::memcpy(s.th, tl.get(), sizeof(float) * p.L);
    return s;
}

// wc_merge_unit with exact-size heap buffers; rc_want != WC_OK: the refusal, nothing written
static Bytes merge_exact(const Bytes& a, const Bytes& b, size_t want_len, int rc_want, const char* what) {
    const std::unique_ptr<uint8_t[]> pa = exact_copy(a), pb = exact_copy(b);
    std::unique_ptr<uint8_t[]> out(new uint8_t[want_len]);
    std::memset(out.get(), 0x5a, want_len);
    size_t w = 77;
    const int rc = wc_merge_unit(pa.get(), a.size(), pb.get(), b.size(), out.get(), want_len, &w);
    CHECK(rc == rc_want, "%s: rc %d, want %d", what, rc, rc_want);
    if (rc != WC_OK) {
        CHECK(w == 77 && std::all_of(out.get(), out.get() + want_len, [](uint8_t v) { return v == 0x5a; }),
              "%s: written on a refusal", what);
        return {};
    }
    CHECK(w == want_len, "%s: %zu bytes, want %zu", what, w, want_len);
    if (want_len) {
        std::unique_ptr<uint8_t[]> small(new uint8_t[want_len - 1]);
        size_t w2 = 77;
        CHECK(wc_merge_unit(pa.get(), a.size(), pb.get(), b.size(), small.get(), want_len - 1, &w2) == WC_ERR_INVALID && w2 == 77,
              "%s: short capacity", what);
    }
    return Bytes(out.get(), out.get() + w);
}

static void test_rule(const std::vector<Pay>& pays) {
    const float zero[WC_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = 0; i < pays.size(); ++i) {
        const Pay& p = pays[i];
        const Bytes canon = thin_of(p.bytes, nullptr, zero, nullptr, nullptr);
        const auto cp = pairs_of(canon);
        const uint32_t c = (uint32_t)cp.size();
        for (uint32_t K : {0u, 1u, c ? c - 1 : 0u, c, c + 1, c / 2, c / 3, 0xffffffffu}) {
            char what[96];
            std::snprintf(what, sizeof what, "payload %zu K %u", i, K);
            const Split s = split_exact(p, &K, nullptr, what);
            if (s.base.empty()) continue;
            uint32_t T = 0;
            float th[WC_MAX_LEVELS] = {0, 0, 0, 0};
            CHECK(s.base == thin_of(p.bytes, &K, nullptr, &T, th), "%s: base != wc_thin_unit", what);
            CHECK(s.key == T && !std::memcmp(s.th, th, sizeof(float) * p.L), "%s: T or thresholds", what);
            CHECK(!std::memcmp(s.rest.data(), p.bytes.data(), 16), "%s: rest header", what);
            // disjoint, and together the pairs of canon(P) in order
            const auto bp = pairs_of(s.base), rp = pairs_of(s.rest);
            std::vector<std::pair<uint64_t, uint32_t>> all(bp);
            all.insert(all.end(), rp.begin(), rp.end());
            std::sort(all.begin(), all.end());
            CHECK(all == cp && bp.size() + rp.size() == cp.size(), "%s: base + rest != canon", what);
            CHECK(merge_exact(s.base, s.rest, canon.size(), WC_OK, what) == canon, "%s: merge(base, rest)", what);
            CHECK(merge_exact(s.rest, s.base, canon.size(), WC_OK, what) == canon, "%s: merge(rest, base)", what);
            // the threshold form at the thresholds of T: the same layers
            const Split t = split_exact(p, nullptr, s.th, what);
            CHECK(t.base == s.base && t.rest == s.rest, "%s: thresholds of T", what);
            // three layers in both groupings
            const uint32_t K2 = (uint32_t)rp.size() / 2;
            Pay rest{p.W, p.H, p.D, p.L, s.rest};
            const Split s2 = split_exact(rest, &K2, nullptr, what);
            if (s2.base.empty()) continue;
            const Bytes ab = merge_exact(s.base, s2.base, s.base.size() + s2.base.size() - 20, WC_OK, what);
            const Bytes bc = merge_exact(s2.base, s2.rest, s.rest.size(), WC_OK, what);
            CHECK(bc == s.rest, "%s: the second split's layers != rest", what);
            CHECK(merge_exact(ab, s2.rest, canon.size(), WC_OK, what) == canon &&
                      merge_exact(s.base, bc, canon.size(), WC_OK, what) == canon,
                  "%s: three layers", what);
            // an overlap at the first, a middle and the last pair of the base
            for (size_t at : {size_t(0), bp.size() / 2, bp.size() ? bp.size() - 1 : 0}) {
                if (bp.empty()) break;
                Bytes one(28);
                std::memcpy(one.data(), p.bytes.data(), 16);
                const int32_t n1 = 1, run = (int32_t)bp[at].first;
                std::memcpy(one.data() + 16, &n1, 4);
                std::memcpy(one.data() + 20, &run, 4);
                std::memcpy(one.data() + 24, &bp[at].second, 4);
                (void)merge_exact(s.base, one, s.base.size() + 8, WC_ERR_FORMAT, "overlap");
                (void)merge_exact(one, s.base, s.base.size() + 8, WC_ERR_FORMAT, "overlap");
            }
        }
        // merge with an empty payload: canon without the value filter (the pairs below N, verbatim)
        Bytes empty(p.bytes.begin(), p.bytes.begin() + 20);
        std::memset(empty.data() + 16, 0, 4);
        const auto pp = pairs_of(p.bytes);
        const Bytes m = merge_exact(p.bytes, empty, 20 + 8 * pp.size(), WC_OK, "merge with empty");
        CHECK(!m.empty() && pairs_of(m) == pp, "payload %zu: merge(a, empty)", i);
        CHECK(merge_exact(empty, p.bytes, 20 + 8 * pp.size(), WC_OK, "merge with empty") == m, "payload %zu: merge(empty, a)", i);
    }
    // refusals
    const Pay& p = pays[1];
    Bytes out(p.bytes.size()), out2(p.bytes.size());
    size_t w = 0, w2 = 0;
    const uint32_t K = 3;
    const float nan[4] = {NAN, 0.f, 0.f, 0.f};
    const uint8_t* in = p.bytes.data();
    const size_t len = p.bytes.size();
    CHECK(wc_split_unit(in, len, nullptr, nullptr, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_INVALID, "neither");
    CHECK(wc_split_unit(in, len, &K, zero, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_INVALID, "both");
    CHECK(wc_split_unit(in, len, nullptr, nan, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_INVALID, "NaN");
    CHECK(wc_split_unit(in, len - 8, &K, nullptr, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_INVALID, "short");
    Bytes bad = p.bytes;
    const int32_t m1 = -1;
    std::memcpy(bad.data() + 28, &m1, 4);
    CHECK(wc_split_unit(bad.data(), len, &K, nullptr, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_FORMAT, "negative run");
    (void)merge_exact(bad, p.bytes, 2 * len, WC_ERR_FORMAT, "negative run in a");
    (void)merge_exact(p.bytes, bad, 2 * len, WC_ERR_FORMAT, "negative run in b");
    bad = p.bytes;
    const int32_t tag = -9;
    std::memcpy(bad.data() + 12, &tag, 4);
    CHECK(wc_split_unit(bad.data(), len, &K, nullptr, out.data(), len, &w, out2.data(), len, &w2, nullptr, nullptr) == WC_ERR_FORMAT, "ncoeff field");
    (void)merge_exact(bad, p.bytes, 2 * len, WC_ERR_FORMAT, "ncoeff field");
    bad = p.bytes;
    const int32_t l3 = -3;  // another level count (pays[1] has L = 2)
    std::memcpy(bad.data() + 12, &l3, 4);
    (void)merge_exact(bad, p.bytes, 2 * len, WC_ERR_FORMAT, "levels differ");
    (void)merge_exact(pays[0].bytes, p.bytes, 2 * len + pays[0].bytes.size(), WC_ERR_FORMAT, "boxes differ");
    Bytes shortb(p.bytes.begin(), p.bytes.end() - 8);
    CHECK(wc_merge_unit(shortb.data(), shortb.size(), in, len, out.data(), out.size(), &w) == WC_ERR_INVALID, "short a");
}

// the payloads laid out with gaps, in a block that ends with the last payload
struct Batch {
    std::unique_ptr<uint8_t[]> buf;
    std::vector<uint64_t> offsets;
};
static Batch lay_out(const std::vector<Bytes>& pays, int skew) {
    Batch b;
    b.offsets.resize(pays.size());
    uint64_t cur = 8;
    for (size_t i = 0; i < pays.size(); ++i) {
        cur = (cur + 7) / 8 * 8 + ((i + skew) % 2 ? 4 : 0) + 8 * (uint64_t)((i + skew) % 3);
        b.offsets[i] = cur;
        cur += pays[i].size();
    }
    b.buf.reset(new uint8_t[cur]);
    std::memset(b.buf.get(), 0xa5, cur);
    for (size_t i = 0; i < pays.size(); ++i) std::memcpy(b.buf.get() + b.offsets[i], pays[i].data(), pays[i].size());
    return b;
}

static void check_packed(const uint8_t* out, uint64_t cap, const uint64_t* off, const uint32_t* cnt, const std::vector<Bytes>& want,
                         const char* what) {
    const int n = (int)want.size();
    uint64_t o = 4;
    for (int i = 0; i < n; ++i) {
        CHECK(off[i] == o && 20 + 8ull * cnt[i] == want[i].size(), "%s unit %d: offset, count", what, i);
        CHECK(o + want[i].size() <= cap && std::memcmp(out + o, want[i].data(), want[i].size()) == 0, "%s unit %d: bytes", what, i);
        o += (i + 1 < n ? 24 : 20) + 8ull * cnt[i];
    }
    CHECK(off[n] == o, "%s: the end", what);
}

static void test_drivers(const std::vector<Pay>& pays) {
    const int n = (int)pays.size();
    std::vector<wc_unit> units(n);
    std::vector<int32_t> levels(n);
    std::vector<Bytes> in(n);
    for (int i = 0; i < n; ++i) {
        units[i] = wc_unit{0, pays[i].W, pays[i].H, pays[i].D, 0};
        levels[i] = pays[i].L;
        in[i] = pays[i].bytes;
    }
    const Batch B = lay_out(in, 0);
    const float zero[WC_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    std::vector<uint32_t> K(n);
    std::vector<float> th((size_t)n * WC_MAX_LEVELS, 0.f);
    std::vector<Split> wb(n), wt(n);
    std::vector<Bytes> canon(n);
    for (int i = 0; i < n; ++i) {
        int32_t nr;
        std::memcpy(&nr, pays[i].bytes.data() + 16, 4);
        K[i] = (uint32_t)nr / 3 + (uint32_t)i;
        wb[i] = split_exact(pays[i], &K[i], nullptr, "driver reference");
        std::memcpy(&th[(size_t)i * WC_MAX_LEVELS], wb[i].th, sizeof(float) * pays[i].L);
        wt[i] = split_exact(pays[i], nullptr, &th[(size_t)i * WC_MAX_LEVELS], "driver reference");
        canon[i] = thin_of(pays[i].bytes, nullptr, zero, nullptr, nullptr);
    }
    for (int64_t chunk : {int64_t(0), int64_t(700), int64_t(1) << 25}) {
        for (int form = 0; form < 4; ++form) {  // budget / thresholds x levels given / from the headers
            const bool budget = form < 2;
            const int32_t* lv = form % 2 ? levels.data() : nullptr;
            wc_ctx* c = make_ctx();
            c->opt_host_chunk = chunk;
            uint64_t bcap = 0, rcap = 0;
            CHECK(wc_split_bound(units.data(), n, budget ? K.data() : nullptr, &bcap, &rcap) == WC_OK &&
                      rcap == wc_payload_bound(units.data(), n) && bcap <= rcap,
                  "wc_split_bound");
            std::unique_ptr<uint8_t[]> base(new uint8_t[bcap]), rest(new uint8_t[rcap]);
            std::memset(base.get(), 0x5a, bcap);
            std::memset(rest.get(), 0x5a, rcap);
            std::unique_ptr<uint64_t[]> boff(new uint64_t[n + 1]), roff(new uint64_t[n + 1]);
            std::unique_ptr<uint32_t[]> kept(new uint32_t[n]), rpairs(new uint32_t[n]), key(new uint32_t[n]);
            std::unique_ptr<float[]> tout(new float[(size_t)n * WC_MAX_LEVELS]);
            auto call = [&](const wc_unit* un, uint64_t bc, uint64_t rc_) {
                return budget ? wc_split_budget_host(c, B.buf.get(), B.offsets.data(), un, n, lv, K.data(), base.get(), bc,
                                                     boff.get(), kept.get(), rest.get(), rc_, roff.get(), rpairs.get(),
                                                     tout.get(), key.get())
                              : wc_split_thresh_host(c, B.buf.get(), B.offsets.data(), un, n, lv, th.data(), base.get(), bc,
                                                     boff.get(), kept.get(), rest.get(), rc_, roff.get(), rpairs.get());
            };
            const int rc = call(units.data(), bcap, rcap);
            CHECK(rc == WC_OK, "split driver form %d chunk %lld: rc %d %s", form, (long long)chunk, rc, c->err.c_str());
            std::vector<Bytes> wbase(n), wrest(n);
            for (int i = 0; i < n; ++i) {
                wbase[i] = (budget ? wb[i] : wt[i]).base;
                wrest[i] = (budget ? wb[i] : wt[i]).rest;
            }
            if (rc == WC_OK) {
                check_packed(base.get(), bcap, boff.get(), kept.get(), wbase, "base");
                check_packed(rest.get(), rcap, roff.get(), rpairs.get(), wrest, "rest");
                for (int i = 0; i < n && budget; ++i) {
                    CHECK(key[i] == wb[i].key, "unit %d key", i);
                    for (int l = 0; l < WC_MAX_LEVELS; ++l) {
                        const float want = l < pays[i].L ? wb[i].th[l] : 0.0f;
                        CHECK(std::memcmp(&tout[(size_t)i * WC_MAX_LEVELS + l], &want, 4) == 0, "unit %d thresh %d", i, l);
                    }
                }
            }
            // a capacity one byte short; a header that disagrees: before anything runs, outputs untouched
            std::memset(base.get(), 0x5a, bcap);
            std::memset(rest.get(), 0x5a, rcap);
            CHECK(call(units.data(), bcap - 1, rcap) == WC_ERR_INVALID && call(units.data(), bcap, rcap - 1) == WC_ERR_INVALID,
                  "short capacity");
            std::vector<wc_unit> other = units;
            std::swap(other[2].ny, other[2].nz);
            const int r2 = call(other.data(), bcap, rcap);
            CHECK(r2 == WC_ERR_FORMAT && std::all_of(base.get(), base.get() + bcap, [](uint8_t b) { return b == 0x5a; }) &&
                      std::all_of(rest.get(), rest.get() + rcap, [](uint8_t b) { return b == 0x5a; }),
                  "mismatched header: %d", r2);

            // the merge of the two layers, b's bytes laid out at other distances than a's
            const Batch A = lay_out(wrest, 1), Bb = lay_out(wbase, 2);
            const uint64_t mcap = wc_merge_bound(units.data(), n);
            std::unique_ptr<uint8_t[]> out(new uint8_t[mcap]);
            std::memset(out.get(), 0x5a, mcap);
            std::unique_ptr<uint64_t[]> moff(new uint64_t[n + 1]);
            std::unique_ptr<uint32_t[]> mp(new uint32_t[n]);
            const int r3 = wc_merge_host(c, A.buf.get(), A.offsets.data(), Bb.buf.get(), Bb.offsets.data(), units.data(), n, lv,
                                         out.get(), mcap, moff.get(), mp.get());
            CHECK(r3 == WC_OK, "merge driver form %d chunk %lld: rc %d %s", form, (long long)chunk, r3, c->err.c_str());
            if (r3 == WC_OK) check_packed(out.get(), mcap, moff.get(), mp.get(), canon, "merged");
            std::memset(out.get(), 0x5a, mcap);
            CHECK(wc_merge_host(c, A.buf.get(), A.offsets.data(), Bb.buf.get(), Bb.offsets.data(), units.data(), n, lv, out.get(),
                                mcap - 1, moff.get(), mp.get()) == WC_ERR_INVALID,
                  "merge: short capacity");
            // b's header of unit 1 names another level count than a's
            std::vector<Bytes> wrong = wbase;
            const int32_t l4 = pays[1].L == 4 ? -3 : -4;
            std::memcpy(wrong[1].data() + 12, &l4, 4);
            const Batch Bw = lay_out(wrong, 2);
            const int r4 = wc_merge_host(c, A.buf.get(), A.offsets.data(), Bw.buf.get(), Bw.offsets.data(), units.data(), n,
                                         nullptr, out.get(), mcap, moff.get(), mp.get());
            CHECK(r4 == WC_ERR_FORMAT && std::all_of(out.get(), out.get() + mcap, [](uint8_t b) { return b == 0x5a; }),
                  "merge: header pair that disagrees: %d", r4);
            destroy_ctx(c);
        }
    }
    g_tabs.clear();
}

int main() {
    Rng r{0x1a7e45};
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
