// test_regionrule.cpp — the index map of the sub-box decode (wc_regionmap.h) and
// its host helpers (wc_regionrule.cpp: wc_region_align, wc_region_units), linked
// alone and built with ASan + UBSan (`make regionsan`):
//   test_regionrule TABLE
// TABLE (tests/test_region_cpu.py writes it from the numpy restatement), one case a line:
//   M W H D L r x0 y0 z0 nx ny nz end k (p i)*k   every flat position p of the box through the map:
//        the kept ones and their compact indices i, in order of p, and `end`
//   A W H D L x0 y0 z0 nx ny nz rc (x0 y0 z0 nx ny nz)   wc_region_align
//   U n (nx ny nz r)*n rc ext (off nx ny nz)*n            wc_region_units
// The compact array of an M case is a heap block of exactly s_x*s_y*s_z elements,
// so a kept index past it is reported by the sanitizer.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "wavelet_amd.h"
#include "wc_regionmap.h"

static bool map_case(std::istringstream& in) {
    uint32_t W, H, D, L, r, x0, y0, z0, nx, ny, nz;
    uint64_t end, k;
    in >> W >> H >> D >> L >> r >> x0 >> y0 >> z0 >> nx >> ny >> nz >> end >> k;
    std::vector<uint64_t> want(2 * k);
    for (auto& v : want) in >> v;
    if (!in) return false;
    const uint32_t w = W >> r, h = H >> r, d = D >> r, Lp = L - r;
    const uint32_t ox = x0 >> r, oy = y0 >> r, oz = z0 >> r, sx = nx >> r, sy = ny >> r, sz = nz >> r;
    if (wc::region_end(w, h, d, Lp, ox, oy, oz, sx, sy, sz, H, D) != end) return false;
    std::vector<uint32_t> compact((size_t)sx * sy * sz, 0u);
    std::vector<uint64_t> got;
    for (uint32_t I = 0; I < W; ++I)
        for (uint32_t J = 0; J < H; ++J)
            for (uint32_t K = 0; K < D; ++K) {
                if (I >= w || J >= h || K >= d) continue;
                const uint32_t lvl = wc::region_level(I, J, K, w, h, d, Lp);
                const uint32_t ix = wc::region_axis(I, w, ox, sx, lvl), iy = wc::region_axis(J, h, oy, sy, lvl),
                               iz = wc::region_axis(K, d, oz, sz, lvl);
                if ((int32_t)(ix | iy | iz) < 0) continue;
                const uint64_t p = ((uint64_t)I * H + J) * D + K, i = ((uint64_t)ix * sy + iy) * sz + iz;
                if (p >= end) return false;
                compact.data()[i] += 1u;  // a heap write: past the block is the sanitizer's to report
                got.push_back(p);
                got.push_back(i);
            }
    for (uint32_t v : compact)
        if (v != 1u) return false;  // the map is a bijection onto the compact unit
    return got == want;
}

static bool align_case(std::istringstream& in) {
    int32_t W, H, D, L, rc;
    wc_region g, want{0, 0, 0, 0, 0, 0}, got{-1, -1, -1, -1, -1, -1};
    in >> W >> H >> D >> L >> g.x0 >> g.y0 >> g.z0 >> g.nx >> g.ny >> g.nz >> rc;
    if (rc == WC_OK) in >> want.x0 >> want.y0 >> want.z0 >> want.nx >> want.ny >> want.nz;
    if (!in) return false;
    if (wc_region_align(W, H, D, L, &g, &got) != rc) return false;
    if (rc != WC_OK) return got.x0 == -1 && got.nz == -1;  // untouched
    return got.x0 == want.x0 && got.y0 == want.y0 && got.z0 == want.z0 && got.nx == want.nx && got.ny == want.ny &&
           got.nz == want.nz;
}

static bool units_case(std::istringstream& in) {
    int n, rc;
    in >> n;
    std::vector<wc_unit> units(n), out(n);
    std::vector<wc_region> regions(n);
    std::vector<int32_t> reduce(n);
    for (int i = 0; i < n; ++i) {
        regions[i] = wc_region{0, 0, 0, 0, 0, 0};
        in >> regions[i].nx >> regions[i].ny >> regions[i].nz >> reduce[i];
        units[i] = wc_unit{0, regions[i].nx, regions[i].ny, regions[i].nz, 0};
    }
    uint64_t ext = 0, want_ext = 0;
    in >> rc >> want_ext;
    if (wc_region_units(units.data(), regions.data(), reduce.data(), n, out.data(), &ext) != rc) return false;
    if (rc != WC_OK) return true;
    if (ext != want_ext) return false;
    for (int i = 0; i < n; ++i) {
        uint64_t off;
        int32_t nx, ny, nz;
        in >> off >> nx >> ny >> nz;
        if (out[i].cell_offset != off || out[i].nx != nx || out[i].ny != ny || out[i].nz != nz || out[i].reserved != 0)
            return false;
    }
    return (bool)in;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_regionrule TABLE\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    int cases = 0, failed = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char kind;
        in >> kind;
        const bool ok = kind == 'M' ? map_case(in) : kind == 'A' ? align_case(in) : kind == 'U' ? units_case(in) : false;
        ++cases;
        if (!ok) {
            ++failed;
            std::fprintf(stderr, "case %d failed: %.80s\n", cases, line.c_str());
        }
    }
    std::printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
