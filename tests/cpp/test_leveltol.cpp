// test_leveltol.cpp — wc_tol_levels_threshold (csrc/wc_leveltolrule.cpp, linked
// alone: plain C++ without the HIP runtime) on tables of counts, built with
// ASan + UBSan by `make leveltolsan`.
//
//   test_leveltol TABLE
// TABLE (text, written by tests/test_leveltol_cpu.py from the numpy
// restatement), one case per line:
//   L N tol_bits(hex u64) bound_bits(hex u64) thresh_bits(hex u32) x L  nnz  (index count) x nnz
// index = (l - 1) * WC_HIST_BINS + b.  Every thresh_l and the bound must match
// bit for bit.  Then the argument checks: null pointers, a NaN or negative
// tolerance and levels outside 1..WC_MAX_LEVELS give WC_ERR_INVALID and write
// nothing; a null bound is allowed.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static uint32_t fbits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static uint64_t dbits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_leveltol TABLE\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int L, cases = 0;
    uint64_t N, tolb, boundb;
    while (std::fscanf(f, "%d %" SCNu64 " %" SCNx64 " %" SCNx64, &L, &N, &tolb, &boundb) == 4) {
        if (L < 1 || L > WC_MAX_LEVELS) {
            std::fprintf(stderr, "table: bad L %d\n", L);
            return 2;
        }
        uint32_t want[WC_MAX_LEVELS];
        for (int l = 0; l < L; ++l)
            if (std::fscanf(f, "%" SCNx32, &want[l]) != 1) return 2;
        size_t nnz;
        if (std::fscanf(f, "%zu", &nnz) != 1) return 2;
        // exactly L x WC_HIST_BINS counts and exactly L thresholds: an access past either is a heap overflow
        std::vector<uint64_t> counts((size_t)L * WC_HIST_BINS, 0);
        for (size_t i = 0; i < nnz; ++i) {
            uint64_t idx, cnt;
            if (std::fscanf(f, "%" SCNu64 " %" SCNu64, &idx, &cnt) != 2 || idx >= counts.size()) return 2;
            counts[idx] = cnt;
        }
        double tol;
        std::memcpy(&tol, &tolb, 8);
        std::vector<float> thresh(L, -7.0f);
        double bound = -7.0;
        const int rc = wc_tol_levels_threshold(counts.data(), L, N, tol, thresh.data(), &bound);
        CHECK(rc == WC_OK, "case %d: rc %d", cases, rc);
        for (int l = 0; l < L; ++l)
            CHECK(fbits(thresh[l]) == want[l], "case %d (L %d tol %g): thresh_%d %08x, want %08x", cases, L, tol, l + 1,
                  fbits(thresh[l]), want[l]);
        CHECK(dbits(bound) == boundb, "case %d (L %d tol %g): bound %a, want bits %016" PRIx64, cases, L, tol, bound,
              boundb);
        std::vector<float> again(L, -7.0f);
        CHECK(wc_tol_levels_threshold(counts.data(), L, N, tol, again.data(), nullptr) == WC_OK, "null bound");
        CHECK(std::memcmp(again.data(), thresh.data(), 4 * (size_t)L) == 0, "case %d: thresholds differ without bound",
              cases);
        ++cases;
    }
    std::fclose(f);

    std::vector<uint64_t> ones((size_t)WC_MAX_LEVELS * WC_HIST_BINS, 1);
    float t[WC_MAX_LEVELS] = {-7.0f, -7.0f, -7.0f, -7.0f};
    double b = -7.0;
    const uint64_t n = ones.size();
    CHECK(wc_tol_levels_threshold(nullptr, 2, n, 1.0, t, &b) == WC_ERR_INVALID, "null counts");
    CHECK(wc_tol_levels_threshold(ones.data(), 2, n, 1.0, nullptr, &b) == WC_ERR_INVALID, "null thresh");
    CHECK(wc_tol_levels_threshold(ones.data(), 2, n, std::nan(""), t, &b) == WC_ERR_INVALID, "NaN tol");
    CHECK(wc_tol_levels_threshold(ones.data(), 2, n, -1.0, t, &b) == WC_ERR_INVALID, "negative tol");
    CHECK(wc_tol_levels_threshold(ones.data(), 0, n, 1.0, t, &b) == WC_ERR_INVALID, "levels 0");
    CHECK(wc_tol_levels_threshold(ones.data(), -1, n, 1.0, t, &b) == WC_ERR_INVALID, "levels -1");
    CHECK(wc_tol_levels_threshold(ones.data(), WC_MAX_LEVELS + 1, n, 1.0, t, &b) == WC_ERR_INVALID, "levels 5");
    for (int l = 0; l < WC_MAX_LEVELS; ++l) CHECK(t[l] == -7.0f, "a refused call wrote thresh_%d", l + 1);
    CHECK(b == -7.0, "a refused call wrote bound");

    std::printf("%d cases, %d checks, %d failed\n", cases, checks, failed);
    return failed ? 1 : 0;
}
