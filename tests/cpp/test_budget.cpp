// test_budget.cpp — wc_budget_select / wc_budget_thresholds (csrc/wc_budgetrule.cpp,
// linked alone: plain C++ without the HIP runtime), built with ASan + UBSan by
// `make budgetsan`.
//
//   test_budget TABLE
// TABLE (text, written by tests/test_budget_cpu.py from the numpy restatement),
// one case per line:
//   W H D L K T(hex) kept thresh_1..thresh_L(hex bits) then W*H*D coefficients (hex bits)
// Every buffer is a heap allocation of exactly the size the call may touch.
// Prints "<cases> cases, <checks> checks, <failed> failed"; exit status 0 only
// if none failed.
#include <cinttypes>
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

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_budget TABLE\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int W, H, D, L, cases = 0;
    uint32_t K, T, kept;
    while (std::fscanf(f, "%d %d %d %d %" SCNu32 " %" SCNx32 " %" SCNu32, &W, &H, &D, &L, &K, &T, &kept) == 7) {
        if (L < 1 || L > WC_MAX_LEVELS || W < 0 || H < 0 || D < 0) {
            std::fprintf(stderr, "table: bad case %d\n", cases);
            return 2;
        }
        std::vector<uint32_t> want(L);
        for (int l = 0; l < L; ++l)
            if (std::fscanf(f, "%" SCNx32, &want[l]) != 1) return 2;
        std::vector<uint32_t> bits((size_t)W * H * D);
        for (uint32_t& b : bits)
            if (std::fscanf(f, "%" SCNx32, &b) != 1) return 2;
        std::vector<float> flat(bits.size());
        if (!bits.empty()) std::memcpy(flat.data(), bits.data(), 4 * bits.size());
        std::vector<float> thresh(L, -7.0f), again(L, -7.0f);
        uint32_t key = 0xdeadbeefu, got = 0xdeadbeefu, key2 = 0xdeadbeefu;
        const int rc = wc_budget_select(flat.data(), W, H, D, L, K, &key, thresh.data(), &got);
        CHECK(rc == WC_OK, "case %d: rc %d", cases, rc);
        CHECK(key == T, "case %d (%dx%dx%d L %d K %u): T %08x, want %08x", cases, W, H, D, L, K, key, T);
        CHECK(got == kept && got <= K, "case %d: kept %u, want %u (K %u)", cases, got, kept, K);
        CHECK(std::memcmp(thresh.data(), want.data(), 4 * (size_t)L) == 0, "case %d: thresholds differ", cases);
        CHECK(wc_budget_select(flat.data(), W, H, D, L, K, &key2, nullptr, nullptr) == WC_OK && key2 == T,
              "case %d: without thresh and kept", cases);
        CHECK(wc_budget_thresholds(T, L, again.data()) == WC_OK &&
                  std::memcmp(again.data(), want.data(), 4 * (size_t)L) == 0,
              "case %d: wc_budget_thresholds differs", cases);
        ++cases;
    }
    std::fclose(f);

    std::vector<float> ones(64, 1.0f);
    float t[WC_MAX_LEVELS] = {-7.0f, -7.0f, -7.0f, -7.0f};
    uint32_t key = 7u, kept2 = 7u;
    CHECK(wc_budget_select(nullptr, 4, 4, 4, 2, 3, &key, t, &kept2) == WC_ERR_INVALID, "null flat");
    CHECK(wc_budget_select(ones.data(), 4, 4, 4, 2, 3, nullptr, t, &kept2) == WC_ERR_INVALID, "null key");
    CHECK(wc_budget_select(ones.data(), 4, 4, 4, 0, 3, &key, t, &kept2) == WC_ERR_INVALID, "levels 0");
    CHECK(wc_budget_select(ones.data(), 4, 4, 4, WC_MAX_LEVELS + 1, 3, &key, t, &kept2) == WC_ERR_INVALID, "levels 5");
    CHECK(wc_budget_select(ones.data(), 4, 4, 4, 3, 3, &key, t, &kept2) == WC_ERR_INVALID, "8 does not divide 4");
    CHECK(wc_budget_select(ones.data(), -4, 4, 4, 1, 3, &key, t, &kept2) == WC_ERR_INVALID, "negative dims");
    CHECK(wc_budget_thresholds(1u, 2, nullptr) == WC_ERR_INVALID, "null thresh");
    CHECK(wc_budget_thresholds(1u, 0, t) == WC_ERR_INVALID, "thresholds: levels 0");
    CHECK(wc_budget_thresholds(1u, WC_MAX_LEVELS + 1, t) == WC_ERR_INVALID, "thresholds: levels 5");
    for (int l = 0; l < WC_MAX_LEVELS; ++l) CHECK(t[l] == -7.0f, "a refused call wrote thresh_%d", l + 1);
    CHECK(key == 7u && kept2 == 7u, "a refused call wrote key or kept");
    // a unit without cells: nothing is read, T = 0
    CHECK(wc_budget_select(nullptr, 0, 8, 8, 2, 5, &key, t, &kept2) == WC_OK && key == 0u && kept2 == 0u, "no cells");

    std::printf("%d cases, %d checks, %d failed\n", cases, checks, failed);
    return failed ? 1 : 0;
}
