// test_maxerr.cpp — wc_maxerr_select (csrc/wc_maxerrrule.cpp, linked alone: plain
// C++ without the HIP runtime), built plain by `make maxerrtest` and with ASan +
// UBSan by `make maxerrsan`.
//
//   test_maxerr TABLE
// TABLE (text, written by tests/test_maxerr_rule_program.py from the numpy
// restatement), one case per line:
//   W H D L dtype E(hex bits of the double) bstar thresh(hex bits) err(hex bits of the double)
//   then W*H*D coefficients (hex bits) and W*H*D cells (hex bits of the float or the double)
// Every buffer is a heap allocation of exactly the size the call may touch.
// Prints "<cases> cases, <checks> checks, <failed> failed"; exit status 0 only
// if none failed.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "wavelet_amd.h"

static int failed = 0, checks = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        ++checks;                              \
        if (!(cond)) {                         \
            ++failed;                          \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
        }                                      \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_maxerr TABLE\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int W, H, D, L, dtype, cases = 0;
    uint64_t ebits, want_err;
    uint32_t want_b, want_thr;
    while (std::fscanf(f, "%d %d %d %d %d %" SCNx64 " %" SCNu32 " %" SCNx32 " %" SCNx64, &W, &H, &D, &L, &dtype, &ebits,
                       &want_b, &want_thr, &want_err) == 9) {
        if (L < 1 || L > WC_MAX_LEVELS || W < 0 || H < 0 || D < 0 || (dtype != WC_F32 && dtype != WC_F64)) {
            std::fprintf(stderr, "table: bad case %d\n", cases);
            return 2;
        }
        const size_t n = (size_t)W * H * D;
        std::vector<float> flat(n);
        for (size_t i = 0; i < n; ++i) {
            uint32_t b;
            if (std::fscanf(f, "%" SCNx32, &b) != 1) return 2;
            std::memcpy(&flat[i], &b, 4);
        }
        std::vector<unsigned char> cells(n * (dtype == WC_F64 ? 8 : 4));
        for (size_t i = 0; i < n; ++i) {
            uint64_t b;
            if (std::fscanf(f, "%" SCNx64, &b) != 1) return 2;
            if (dtype == WC_F64) {
                std::memcpy(&cells[8 * i], &b, 8);
            } else {
                const uint32_t b32 = (uint32_t)b;
                std::memcpy(&cells[4 * i], &b32, 4);
            }
        }
        double E;
        std::memcpy(&E, &ebits, 8);
        float thr = -7.0f;
        double err = -7.0;
        uint32_t bstar = 0xdeadbeefu;
        const int rc = wc_maxerr_select(flat.data(), cells.data(), dtype, W, H, D, L, E, &thr, &err, &bstar);
        CHECK(rc == WC_OK, "case %d: rc %d", cases, rc);
        uint32_t tb;
        uint64_t eb;
        std::memcpy(&tb, &thr, 4);
        std::memcpy(&eb, &err, 8);
        CHECK(bstar == want_b, "case %d (%dx%dx%d L %d): b* %u, want %u", cases, W, H, D, L, bstar, want_b);
        CHECK(tb == want_thr, "case %d: thresh %08x, want %08x", cases, tb, want_thr);
        CHECK(eb == want_err, "case %d: err %016" PRIx64 ", want %016" PRIx64, cases, eb, want_err);
        CHECK(bstar == 0u || err <= E, "case %d: err above the bound at b* %u", cases, bstar);
        // nullable outputs, each alone
        uint32_t b2 = 0;
        CHECK(wc_maxerr_select(flat.data(), cells.data(), dtype, W, H, D, L, E, nullptr, nullptr, &b2) == WC_OK &&
                  b2 == want_b,
              "case %d: b* alone", cases);
        ++cases;
    }
    std::fclose(f);
    // refusals: nothing is written
    {
        std::vector<float> flat(8, 1.0f), cells(8, 1.0f);
        float thr = -7.0f;
        double err = -7.0;
        uint32_t b = 77u;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 2, 2, 2, 1, nan, &thr, &err, &b) == WC_ERR_INVALID,
              "NaN bound accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 2, 2, 2, 1, -1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "negative bound accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 2, 2, 2, 0, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "level 0 accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 2, 2, 2, 5, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "level 5 accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 2, 2, 2, 2, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "2x2x2 at L = 2 accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), WC_F32, 1, 2, 4, 1, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "odd dimension accepted");
        CHECK(wc_maxerr_select(nullptr, cells.data(), WC_F32, 2, 2, 2, 1, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "null flat accepted");
        CHECK(wc_maxerr_select(flat.data(), cells.data(), 99, 2, 2, 2, 1, 1.0, &thr, &err, &b) == WC_ERR_INVALID,
              "dtype 99 accepted");
        CHECK(thr == -7.0f && err == -7.0 && b == 77u, "a refused call wrote an output");
        // a unit without cells: thresh 0.0f, err 0.0, b* 0
        CHECK(wc_maxerr_select(nullptr, nullptr, WC_F32, 0, 4, 4, 1, 1.0, &thr, &err, &b) == WC_OK && thr == 0.0f &&
                  err == 0.0 && b == 0u,
              "unit without cells");
    }
    std::printf("%d cases, %d checks, %d failed\n", cases, checks, failed);
    return failed || cases == 0 ? 1 : 0;
}
