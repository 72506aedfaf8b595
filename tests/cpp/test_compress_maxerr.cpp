// test_compress_maxerr.cpp — compress_maxerr of the C++ mirror (include/wavelet_amd/codec_extras.h):
//   test_compress_maxerr IN.raw W H D NCOMP LEVELS MAXERR OUTDIR
// reads NCOMP components of a W x H x D box (raw fp32, x fastest, back to back)
// from IN.raw, calls compress_maxerr(box, {0..NCOMP-1}, LEVELS, MAXERR, 7, 1, 3,
// OUTDIR) and prints the pair count of every component.  Driven by
// tests/test_gpu_maxerr_mirror.py, which compares the files it wrote with the
// restatement's payloads.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "wavelet_amd/codec_extras.h"

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: test_compress_maxerr IN.raw W H D NCOMP LEVELS MAXERR OUTDIR\n");
        return 2;
    }
    const size_t W = std::strtoul(argv[2], nullptr, 10), H = std::strtoul(argv[3], nullptr, 10),
                 D = std::strtoul(argv[4], nullptr, 10);
    const int ncomp = std::atoi(argv[5]), levels = std::atoi(argv[6]);
    const double maxerr = std::strtod(argv[7], nullptr);
    std::ifstream f(argv[1], std::ios::binary);
    multiBox3D box;
    std::vector<int> components;
    for (int c = 0; c < ncomp; ++c) {
        Box3D b(W, H, D);
        f.read(reinterpret_cast<char*>(b.data()), (std::streamsize)(sizeof(float) * b.data_size()));
        if (!f) {
            std::fprintf(stderr, "cannot read component %d from %s\n", c, argv[1]);
            return 1;
        }
        box.push_back(std::move(b));
        components.push_back(c);
    }
    const std::vector<CompressedWavelet> out = wavelet_amd::compress_maxerr(box, components, levels, maxerr, 7, 1, 3, argv[8]);
    for (const CompressedWavelet& cw : out) std::printf("%zu\n", cw.rle_encoded.size());
    return 0;
}
