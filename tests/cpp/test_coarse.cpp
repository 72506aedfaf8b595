// test_coarse.cpp — decompress_coarse of the C++ mirror (include/wavelet_amd/codec_extras.h):
//   test_coarse FILE.xz REDUCE OUT.raw
// decodes FILE.xz at 1/2^REDUCE resolution, prints "W H D" of the coarse box and
// writes its cells (x fastest) as raw fp32 to OUT.raw.  REDUCE = 0 also checks
// that the result equals decompress()'s box byte for byte.  Driven by
// tests/test_gpu_coarse.py, which compares the cells with the Python result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "wavelet_amd/codec_extras.h"
#include "wavelet_amd/decompressor.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: test_coarse FILE.xz REDUCE OUT.raw\n");
        return 2;
    }
    const int reduce = std::atoi(argv[2]);
    Box3D box = wavelet_amd::decompress_coarse(argv[1], reduce);
    if (reduce == 0) {
        Box3D full = decompress(argv[1], 0, 0, 0, 0);
        if (full.data_size() != box.data_size() ||
            std::memcmp(full.data(), box.data(), sizeof(float) * box.data_size()) != 0) {
            std::fprintf(stderr, "reduce 0 differs from decompress()\n");
            return 1;
        }
    }
    std::ofstream f(argv[3], std::ios::binary);
    f.write(reinterpret_cast<const char*>(box.data()), (std::streamsize)(sizeof(float) * box.data_size()));
    if (!f) {
        std::fprintf(stderr, "cannot write %s\n", argv[3]);
        return 1;
    }
    std::printf("%zu %zu %zu\n", box.width(), box.height(), box.depth());
    return 0;
}
