// test_pack.cpp — the packed payload format's host rule (csrc/wc_packrule.cpp with
// wc_packfmt.h, linked alone: plain C++ without the HIP runtime), built with
// ASan + UBSan by `make packsan`.
//
//   test_pack TABLE
// TABLE (text, written by tests/test_pack_cpu.py from the numpy restatement), one
// case per line:
//   V len payload(hex) packed(hex) quantised(hex)
// Every buffer is a heap allocation of exactly the size the call may touch.
// Prints "<cases> cases, <checks> checks, <failed> failed"; exit status 0 only
// if none failed.
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

    std::printf("%d cases, %d checks, %d failed\n", cases, checks, failed);
    return failed ? 1 : 0;
}
