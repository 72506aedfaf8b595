// test_region.cpp — decompress_region of the C++ mirror (include/wavelet_amd/codec_extras.h):
//   test_region FILE.xz X0 Y0 Z0 X1 Y1 Z1 REDUCE OUT.raw
// decodes the cells [lo, hi) of FILE.xz at 1/2^REDUCE resolution, prints "W H D" of
// the result and writes its cells (x fastest) as raw fp32 to OUT.raw.  Driven by
// tests/test_gpu_region.py, which compares the cells with the Python result.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "wavelet_amd/codec_extras.h"

int main(int argc, char** argv) {
    if (argc != 10) {
        std::fprintf(stderr, "usage: test_region FILE.xz X0 Y0 Z0 X1 Y1 Z1 REDUCE OUT.raw\n");
        return 2;
    }
    const std::array<int, 3> lo{std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])};
    const std::array<int, 3> hi{std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7])};
    Box3D box = wavelet_amd::decompress_region(argv[1], lo, hi, std::atoi(argv[8]));
    std::ofstream f(argv[9], std::ios::binary);
    f.write(reinterpret_cast<const char*>(box.data()), (std::streamsize)(sizeof(float) * box.data_size()));
    if (!f) {
        std::fprintf(stderr, "cannot write %s\n", argv[9]);
        return 1;
    }
    std::printf("%zu %zu %zu\n", box.width(), box.height(), box.depth());
    return 0;
}
