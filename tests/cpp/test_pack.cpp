// test_pack.cpp — the packed payload format's host rule (csrc/wc_packrule.cpp with
// wc_packfmt.h, linked alone: plain C++ without the HIP runtime), built with
// ASan + UBSan by `make packsan`.
//
//   test_pack TABLE
// TABLE (text, written by tests/test_pack_cpu.py from the numpy restatement), one
// case per line:
//   V len payload(hex) packed(hex) quantised(hex)
// Every buffer is a heap allocation of exactly the size the call may touch.
// After the table: units from a seeded generator of the classes tests/pack_rule.py
// draws (odd dimensions, pair counts at the chunk and tile edges, every width,
// slots filled to S(N)), held against a bit-by-bit restatement in this file; and
// corrupted copies of their packed forms (a header field, a table byte, the
// length): wc_packed_size, wc_unpack_unit and wc_pack_unit either refuse and
// write nothing, or give what the restatement gives.
// Prints "<cases> cases, <checks> checks, <failed> failed" (cases: the table's);
// exit status 0 only if none failed.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "wavelet_amd.h"

static int failed = 0, checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        ++checks;                         \
        if (!(cond)) {                    \
            ++failed;                     \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");   \
        }                                 \
    } while (0)

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)(nib(s[2 * i]) << 4 | nib(s[2 * i + 1]));
    return out;
}

// ---- generated units, and corrupted copies of their packed forms --------------
// The format restated bit by bit, apart from wc_packrule.cpp (only the value rule
// wc_pack_value is taken from it: the table's cases hold it against numpy).

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 32);
    }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

static const int kDims[][3] = {{1, 1, 1}, {2, 2, 2}, {3, 5, 7},  {5, 1, 9},    {6, 10, 14},
                               {33, 17, 9}, {0, 4, 4}, {8, 8, 8}, {16, 16, 16}, {24, 8, 40}};
static const int kFullDims[][3] = {{2, 2, 2}, {3, 5, 7}, {8, 8, 8}, {6, 10, 14}};
static const uint32_t kSpecials[] = {0x3F808000u, 0x3F818000u, 0x3F800080u, 0x3F800180u, 0x3FFFFFFFu, 0x407FFFFFu,
                                     0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u, 0x7F800001u, 0xFFC00000u,
                                     0x7FBFFFFFu, 0x7F80FFFFu, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x00008000u,
                                     0x00018000u, 0x807F8000u, 0x00000000u, 0x80000000u, 0x00800000u, 0x3F800000u};

static void put32(std::vector<uint8_t>& v, size_t at, uint32_t x) { std::memcpy(v.data() + at, &x, 4); }
static int32_t get32(const uint8_t* p, size_t at) {
    int32_t x;
    std::memcpy(&x, p + at, 4);
    return x;
}

// A standard payload of the class the numpy generator draws (tests/pack_rule.py fuzz_batch): dimensions, L, a pair
// count at the edges of a chunk and of a 2048-pair tile, per chunk a width 0..31 met exactly; full: n = cells, w = 31.
static std::vector<uint8_t> gen_unit(Rng& r, const int* d, int cls, bool full) {
    const int W = d[0], H = d[1], D = d[2];
    const uint32_t cells = (uint32_t)(W * H * D);
    int L = 1;
    if (!full)
        for (int l = 2; l <= 4; ++l)
            if (((W | H | D) & ((1 << l) - 1)) == 0 && r.below(2)) L = l;
    const uint32_t k64 = 1 + r.below(cells / 64 ? cells / 64 : 1), k2048 = 1 + r.below(cells / 2048 ? cells / 2048 : 1);
    const int64_t pick[] = {0, 1, cells, (int64_t)cells - 1, 64 * k64 - 1, 64 * k64, 64 * k64 + 1,
                            2048 * k2048 - 1, 2048 * k2048, 2048 * k2048 + 1, r.below(cells + 1)};
    int64_t want = full ? cells : pick[cls < 10 ? cls : 10];
    const uint32_t n = (uint32_t)(want < 0 ? 0 : want > (int64_t)cells ? cells : want);
    std::vector<uint8_t> pay(20 + 8 * (size_t)n);
    put32(pay, 0, W), put32(pay, 4, H), put32(pay, 8, D), put32(pay, 12, L == 1 ? cells : (uint32_t)-L), put32(pay, 16, n);
    for (uint32_t c = 0; 64 * c < n; ++c) {
        const uint32_t m = n - 64 * c < 64 ? n - 64 * c : 64;
        const uint32_t w = full ? 31 : r.below(8) ? r.below(32) : 0;
        const uint32_t top = r.below(m);
        for (uint32_t j = 0; j < m; ++j) {
            uint32_t run = w ? r.next() & ((1u << w) - 1u) : 0u;
            if (w && j == top) run |= 1u << (w - 1);
            put32(pay, 20 + 8 * (64 * c + j), run);
            put32(pay, 24 + 8 * (64 * c + j), r.below(4) ? r.next() : kSpecials[r.below(sizeof kSpecials / 4)]);
        }
    }
    return pay;
}

// The fourth header field against the box.  packed: a tag -(16 V + L); else W*H*D (L = 1) or -L (L = 2..4).
static bool ref_header(const uint8_t* u, bool packed, int& L, int& V, uint64_t& n) {
    const int64_t W = get32(u, 0), H = get32(u, 4), D = get32(u, 8), t = get32(u, 12), nr = get32(u, 16);
    if (W < 0 || H < 0 || D < 0) return false;
    const unsigned __int128 cells = (unsigned __int128)(uint64_t)W * (uint64_t)H * (uint64_t)D;
    if (cells > 0x7FFFFFFFu) return false;
    V = 0, L = 1;
    if (packed) {
        if (t >= 0 || (-t) / 16 < 2 || (-t) / 16 > 4) return false;
        V = (int)((-t) / 16), L = (int)((-t) % 16);
    } else if (t < 0) {
        L = (int)-t;
        if (L < 2) return false;
    } else if ((unsigned __int128)t != cells) {
        return false;
    }
    if (L < 1 || L > 4) return false;
    if (L >= 2 && cells != 0 && ((W | H | D) & ((1 << L) - 1))) return false;
    if (nr < 0 || (unsigned __int128)nr > cells) return false;
    n = (uint64_t)nr;
    return true;
}

enum { kGood = 0, kMalformed = 1, kShort = 2 };

// A packed unit in u[0..len): its length from header and table.  kShort: the table or the body passes len.
static int ref_packed(const uint8_t* u, size_t len, int& L, int& V, uint64_t& n, uint64_t& size, bool& table_ok) {
    table_ok = false;
    if (len < 20) return kShort;
    if (!ref_header(u, true, L, V, n)) return kMalformed;
    const uint64_t nch = (n + 63) / 64, npad = (nch + 7) / 8 * 8;
    if (len < 20 + npad) return kShort;
    size = 20 + npad;
    for (uint64_t c = 0; c < nch; ++c) {
        if (u[20 + c] > 31) return kMalformed;
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * c;
        size += u[20 + c] * ((m + 7) / 8) + (uint64_t)V * m;
    }
    table_ok = true;
    return len < size ? kShort : kGood;
}

static std::vector<uint8_t> ref_unpack(const uint8_t* u, int L, int V, uint64_t n) {
    std::vector<uint8_t> pay(20 + 8 * n, 0);
    std::memcpy(pay.data(), u, 20);
    put32(pay, 12, L >= 2 ? (uint32_t)-L : (uint32_t)((uint64_t)get32(u, 0) * (uint64_t)get32(u, 4) * (uint64_t)get32(u, 8)));
    const uint64_t nch = (n + 63) / 64;
    size_t base = 20 + (nch + 7) / 8 * 8;
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * c, pl = (m + 7) / 8, w = u[20 + c];
        for (uint64_t j = 0; j < m; ++j) {
            uint32_t run = 0, val = 0;
            for (uint64_t b = 0; b < w; ++b) run |= (uint32_t)((u[base + b * pl + j / 8] >> (j % 8)) & 1) << b;
            for (int p = 0; p < V; ++p) val |= (uint32_t)u[base + w * pl + p * m + j] << (8 * (3 - p));
            put32(pay, 20 + 8 * (64 * c + j), run);
            put32(pay, 24 + 8 * (64 * c + j), val);
        }
        base += w * pl + V * m;
    }
    return pay;
}

// A standard payload in p[0..len): kGood if wc_pack_unit must take it.
static int ref_standard(const uint8_t* p, size_t len, int& L, uint64_t& n) {
    int V;
    if (len < 20) return kShort;
    if (!ref_header(p, false, L, V, n)) return kMalformed;
    if (len < 20 + 8 * n) return kShort;
    for (uint64_t k = 0; k < n; ++k)
        if (get32(p, 20 + 8 * k) < 0) return kMalformed;
    return kGood;
}

static std::vector<uint8_t> ref_pack(const uint8_t* p, int L, int V, uint64_t n) {
    const uint64_t nch = (n + 63) / 64, npad = (nch + 7) / 8 * 8;
    std::vector<uint8_t> out(20 + npad, 0);
    std::memcpy(out.data(), p, 20);
    put32(out, 12, (uint32_t)-(16 * V + L));
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t m = c + 1 < nch ? 64 : n - 64 * c, pl = (m + 7) / 8;
        uint32_t acc = 0;
        for (uint64_t j = 0; j < m; ++j) acc |= (uint32_t)get32(p, 20 + 8 * (64 * c + j));
        int w = 0;
        while (w < 32 && (acc >> w)) ++w;
        out[20 + c] = (uint8_t)w;
        const size_t base = out.size();
        out.resize(base + w * pl + V * m, 0);
        for (uint64_t j = 0; j < m; ++j) {
            const uint32_t run = (uint32_t)get32(p, 20 + 8 * (64 * c + j));
            const uint32_t val = wc_pack_value((uint32_t)get32(p, 24 + 8 * (64 * c + j)), V);
            for (int b = 0; b < w; ++b) out[base + b * pl + j / 8] |= (uint8_t)(((run >> b) & 1u) << (j % 8));
            for (int q = 0; q < V; ++q) out[base + w * pl + q * m + j] = (uint8_t)(val >> (8 * (3 - q)));
        }
    }
    return out;
}

static bool untouched(const std::vector<uint8_t>& v) {
    for (uint8_t x : v)
        if (x != 0xA5) return false;
    return true;
}

static int accepted = 0, refused = 0;

// u[0..len) stands where a packed unit should: every call either refuses and writes nothing, or gives what the
// restatement gives.  The inputs and outputs are heap blocks of exactly the bytes a call may touch.
static void check_claimed_packed(const std::vector<uint8_t>& u, const char* what, int id) {
    int L = 0, V = 0;
    uint64_t n = 0, size = 0;
    bool table_ok = false;
    const int ref = ref_packed(u.data(), u.size(), L, V, n, size, table_ok);
    uint64_t s = 77;
    int rc = wc_packed_size(u.data(), u.size(), &s);
    if (table_ok)
        CHECK(rc == WC_OK && s == size, "%s %d: packed_size rc %d, %" PRIu64 " (want %" PRIu64 ")", what, id, rc, s, size);
    else
        CHECK(rc != WC_OK && s == 77, "%s %d: packed_size took a bad unit (rc %d)", what, id, rc);
    size_t w = 77;
    if (ref == kGood) {
        const std::vector<uint8_t> want = ref_unpack(u.data(), L, V, n);
        std::vector<uint8_t> out(want.size(), 0xA5);
        rc = wc_unpack_unit(u.data(), u.size(), out.data(), out.size(), &w);
        CHECK(rc == WC_OK && w == want.size() && out == want, "%s %d: unpack rc %d", what, id, rc);
        // what it gave packs to the restatement's bytes
        int L2 = 0;
        uint64_t n2 = 0;
        CHECK(ref_standard(want.data(), want.size(), L2, n2) == kGood, "%s %d: the unpacked payload", what, id);
        const std::vector<uint8_t> again = ref_pack(want.data(), L2, V, n2);
        std::vector<uint8_t> pk(again.size(), 0xA5);
        rc = wc_pack_unit(want.data(), want.size(), V, pk.data(), pk.size(), &w);
        CHECK(rc == WC_OK && w == again.size() && pk == again, "%s %d: pack of the unpacked payload rc %d", what, id, rc);
        ++accepted;
    } else {
        const int64_t claimed = u.size() >= 20 ? get32(u.data(), 16) : 0;
        std::vector<uint8_t> out(20 + 8 * (size_t)(claimed < 0 ? 0 : claimed > 4096 ? 4096 : claimed), 0xA5);
        rc = wc_unpack_unit(u.data(), u.size(), out.data(), out.size(), &w);
        CHECK(rc != WC_OK && w == 77 && untouched(out), "%s %d: unpack took a bad unit (rc %d)", what, id, rc);
        ++refused;
    }
    // the same bytes offered to wc_pack_unit as a payload: a packed tag is no standard header
    int Ls = 0;
    uint64_t ns = 0;
    const int std_ref = ref_standard(u.data(), u.size(), Ls, ns);
    w = 77;
    if (std_ref == kGood) {
        const std::vector<uint8_t> want = ref_pack(u.data(), Ls, 3, ns);
        std::vector<uint8_t> pk(want.size(), 0xA5);
        rc = wc_pack_unit(u.data(), u.size(), 3, pk.data(), pk.size(), &w);
        CHECK(rc == WC_OK && w == want.size() && pk == want, "%s %d: pack of a standard header rc %d", what, id, rc);
    } else {
        std::vector<uint8_t> pk(64, 0xA5);
        rc = wc_pack_unit(u.data(), u.size(), 3, pk.data(), pk.size(), &w);
        CHECK(rc != WC_OK && w == 77 && untouched(pk), "%s %d: pack took a bad payload (rc %d)", what, id, rc);
    }
}

static const int32_t kFieldValues[] = {0, 1, -1, 2, 7, 64, 65, 512, -2, -4, -5, -33, -36, -37, -52, -68, -69, -80,
                                       1 << 16, 1 << 30, INT32_MAX, INT32_MIN};

static void fuzz(uint64_t seed, int& units, int& corruptions) {
    Rng r{seed};
    const int ndims = (int)(sizeof kDims / sizeof kDims[0]), nfull = (int)(sizeof kFullDims / sizeof kFullDims[0]);
    for (int i = 0; i < ndims * 4 + nfull; ++i, ++units) {
        const bool full = i >= ndims * 4;
        const std::vector<uint8_t> pay = gen_unit(r, full ? kFullDims[i - ndims * 4] : kDims[i % ndims], (i * 7 + (int)seed) % 16, full);
        int L = 0;
        uint64_t n = 0;
        CHECK(ref_standard(pay.data(), pay.size(), L, n) == kGood, "unit %d: the generator", i);
        const uint64_t cells = (uint64_t)get32(pay.data(), 0) * get32(pay.data(), 4) * get32(pay.data(), 8);
        for (int V = 2; V <= 4; ++V) {
            const std::vector<uint8_t> want = ref_pack(pay.data(), L, V, n);
            const uint64_t worst = 20 + ((cells + 63) / 64 + 7) / 8 * 8 + 31 * ((cells + 7) / 8) + V * cells;
            CHECK(full ? want.size() == worst : want.size() <= worst, "unit %d: %zu bytes against S(N) %" PRIu64, i,
                  want.size(), worst);
            std::vector<uint8_t> out(want.size(), 0xA5);
            size_t w = 77;
            const int rc = wc_pack_unit(pay.data(), pay.size(), V, out.data(), out.size(), &w);
            CHECK(rc == WC_OK && w == want.size() && out == want, "unit %d V %d: pack rc %d", i, V, rc);
            check_claimed_packed(want, "unit", i);
            // corrupted copies: a header field, a table byte, the length
            const uint64_t nch = (n + 63) / 64;
            for (int k = 0; k < 24; ++k, ++corruptions) {
                std::vector<uint8_t> bad = want;
                const uint32_t kind = r.below(8);
                if (kind < 3) {
                    const size_t at = 4 * r.below(5);
                    const uint32_t how = r.below(4);
                    const int32_t old = get32(bad.data(), at);
                    put32(bad, at, how == 0   ? (uint32_t)old ^ (1u << r.below(32))
                                   : how == 1 ? (uint32_t)old + 1u
                                   : how == 2 ? (uint32_t)old - 1u
                                              : (uint32_t)kFieldValues[r.below(sizeof kFieldValues / 4)]);
                } else if (kind < 5 && nch) {
                    const size_t at = 20 + r.below((uint32_t)nch);
                    const uint32_t how = r.below(4);
                    bad[at] = how == 0 ? (uint8_t)r.next() : how == 1 ? (uint8_t)(bad[at] + 1) : how == 2 ? (uint8_t)(bad[at] - 1) : 32;
                } else if (kind == 5) {
                    bad.resize(r.below((uint32_t)bad.size()));
                } else if (kind == 6) {
                    bad.resize(bad.size() - 1 - (bad.size() > 20 ? r.below(8) % (bad.size() - 20) : 0));
                } else {  // two fields at once: dimensions whose product passes 2^31, or 2^64
                    put32(bad, 4 * r.below(3), kFieldValues[r.below(sizeof kFieldValues / 4)]);
                    put32(bad, 4 * r.below(3), kFieldValues[r.below(sizeof kFieldValues / 4)]);
                    if (r.below(2)) put32(bad, 16, 0);
                }
                check_claimed_packed(std::vector<uint8_t>(bad.begin(), bad.end()), "corruption", corruptions);
            }
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_pack TABLE\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int cases = 0;
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int V;
        size_t len;
        std::string a, b, c;
        if (!(in >> V >> len >> a >> b >> c) || a.size() != 2 * len) {
            std::fprintf(stderr, "table: bad case %d\n", cases);
            return 2;
        }
        const std::vector<uint8_t> pay = unhex(a), want = unhex(b), quant = unhex(c);
        // pack into exactly the expected length, and into one byte less
        std::vector<uint8_t> out(want.size(), 0xA5);
        size_t w = 77;
        int rc = wc_pack_unit(pay.data(), pay.size(), V, out.data(), out.size(), &w);
        CHECK(rc == WC_OK && w == want.size() && out == want, "case %d: pack rc %d, %zu bytes (want %zu)", cases, rc, w,
              want.size());
        if (want.size() > 20) {
            std::vector<uint8_t> tight(want.size() - 1, 0xA5);
            w = 77;
            rc = wc_pack_unit(pay.data(), pay.size(), V, tight.data(), tight.size(), &w);
            bool clean = true;
            for (uint8_t x : tight) clean = clean && x == 0xA5;
            CHECK(rc == WC_ERR_INVALID && w == 77 && clean, "case %d: pack into a short buffer: rc %d", cases, rc);
        }
        uint64_t size = 0;
        int nrle;
        std::memcpy(&nrle, want.data() + 16, 4);
        const size_t table_end = 20 + (((size_t)nrle + 63) / 64 + 7) / 8 * 8;
        CHECK(wc_packed_size(want.data(), table_end, &size) == WC_OK && size == want.size(), "case %d: size %" PRIu64,
              cases, size);
        if (table_end > 20) {
            std::vector<uint8_t> head(want.begin(), want.begin() + table_end - 1);
            CHECK(wc_packed_size(head.data(), head.size(), &size) == WC_ERR_INVALID, "case %d: size of a cut table", cases);
        }
        int L = 0, Vg = -1;
        CHECK(wc_payload_packed(want.data(), 20, &L, &Vg) == WC_OK && Vg == V, "case %d: payload_packed V %d", cases, Vg);
        CHECK(wc_payload_packed(pay.data(), 20, &L, &Vg) == WC_OK && Vg == 0, "case %d: a standard header", cases);
        // unpack into exactly 20 + 8 n bytes, and refuse a cut unit and a short output
        std::vector<uint8_t> back(quant.size(), 0xA5);
        w = 77;
        rc = wc_unpack_unit(want.data(), want.size(), back.data(), back.size(), &w);
        CHECK(rc == WC_OK && w == quant.size() && back == quant, "case %d: unpack rc %d", cases, rc);
        if (V == 4) CHECK(back == pay, "case %d: V = 4 is not lossless", cases);
        if (want.size() > 20) {
            std::vector<uint8_t> cut(want.begin(), want.end() - 1);
            CHECK(wc_unpack_unit(cut.data(), cut.size(), back.data(), back.size(), &w) == WC_ERR_INVALID,
                  "case %d: unpack of a cut unit", cases);
            std::vector<uint8_t> small(quant.size() - 1, 0xA5);
            CHECK(wc_unpack_unit(want.data(), want.size(), small.data(), small.size(), &w) == WC_ERR_INVALID,
                  "case %d: unpack into a short buffer", cases);
        }
        // the quantised payload packs to the same bytes
        std::vector<uint8_t> again(want.size(), 0xA5);
        rc = wc_pack_unit(quant.data(), quant.size(), V, again.data(), again.size(), &w);
        CHECK(rc == WC_OK && again == want, "case %d: packing the quantised payload", cases);
        ++cases;
    }

    uint8_t h[20] = {};
    size_t w = 0;
    uint64_t s = 0;
    int L, V;
    CHECK(wc_pack_unit(nullptr, 20, 3, h, 20, &w) == WC_ERR_INVALID, "null payload");
    CHECK(wc_pack_unit(h, 20, 3, nullptr, 20, &w) == WC_ERR_INVALID, "null out");
    CHECK(wc_pack_unit(h, 20, 3, h, 20, nullptr) == WC_ERR_INVALID, "null written");
    CHECK(wc_pack_unit(h, 19, 3, h, 20, &w) == WC_ERR_INVALID, "short header");
    CHECK(wc_unpack_unit(nullptr, 20, h, 20, &w) == WC_ERR_INVALID, "unpack: null");
    CHECK(wc_packed_size(h, 19, &s) == WC_ERR_INVALID && wc_packed_size(h, 20, nullptr) == WC_ERR_INVALID, "size: args");
    CHECK(wc_payload_packed(h, 19, &L, &V) == WC_ERR_INVALID && wc_payload_packed(h, 20, nullptr, &V) == WC_ERR_INVALID,
          "payload_packed: args");
    CHECK(wc_pack_value(0x7F7FFFFFu, 2) == 0x7F7F0000u && wc_pack_value(0x3FFFFFFFu, 3) == 0x40000000u, "q");
    const int32_t minhdr[5] = {1, 1, 1, INT32_MIN, 0};
    CHECK(wc_payload_packed((const uint8_t*)minhdr, 20, &L, &V) == WC_ERR_FORMAT, "tag INT32_MIN");
    wc_unit u[2] = {{0, 8, 8, 8, 0}, {0, 0, 4, 4, 0}};
    CHECK(wc_packed_bound(u, 2, 3, &s) == WC_OK && s == 4 + ((20 + 8 + 31 * 64 + 3 * 512 + 4 + 7) / 8 * 8) + 24,
          "bound %" PRIu64, s);
    CHECK(wc_packed_bound(u, 2, 1, &s) == WC_ERR_INVALID && wc_packed_bound(nullptr, 2, 3, &s) == WC_ERR_INVALID, "bound: args");

    // dimensions whose product wraps to a small number in 64 bits: 2^30 * 2^30 * 16 = 2^64
    for (int32_t tag : {-49, 0}) {
        std::vector<uint8_t> wrap(20, 0);
        put32(wrap, 0, 1u << 30), put32(wrap, 4, 1u << 30), put32(wrap, 8, 16), put32(wrap, 12, (uint32_t)tag);
        check_claimed_packed(wrap, "wrapping dimensions", tag);
        put32(wrap, 8, 0);  // no cells: a good header
        check_claimed_packed(wrap, "no cells", tag);
    }
    int units = 0, corruptions = 0;
    for (uint64_t seed = 1; seed <= 3; ++seed) fuzz(seed, units, corruptions);
    std::printf("fuzz: %d units, %d corruptions; %d packed units accepted, %d refused\n", units, corruptions, accepted,
                refused);
    std::printf("%d cases, %d checks, %d failed\n", cases, checks, failed);
    return failed ? 1 : 0;
}
