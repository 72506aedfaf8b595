// test_compress_packed.cpp — compress_packed of the C++ mirror (include/wavelet_amd/codec_extras.h):
//   test_compress_packed IN.raw W H D NCOMP KEEP VBYTES OUTDIR
// reads NCOMP components of a W x H x D box (raw fp32, x fastest, back to back)
// from IN.raw, calls compress_packed(box, {0..NCOMP-1}, KEEP, VBYTES, 7, 1, 3,
// OUTDIR), prints the pair count of every component, then reads every file back
// with decompress() and writes its cells to OUTDIR/cells-<component>.raw.  Driven
// by tests/test_gpu_pack_mirror.py, which compares files and cells with the
// restatement's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "wavelet_amd/codec_extras.h"
#include "wavelet_amd/decompressor.h"

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: test_compress_packed IN.raw W H D NCOMP KEEP VBYTES OUTDIR\n");
        return 2;
    }
    const size_t W = std::strtoul(argv[2], nullptr, 10), H = std::strtoul(argv[3], nullptr, 10),
                 D = std::strtoul(argv[4], nullptr, 10);
    const int ncomp = std::atoi(argv[5]), vbytes = std::atoi(argv[7]);
    const double keep = std::strtod(argv[6], nullptr);
    const std::string dir = argv[8];
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
    const std::vector<CompressedWavelet> out = wavelet_amd::compress_packed(box, components, keep, vbytes, 7, 1, 3, dir);
    for (const CompressedWavelet& cw : out) std::printf("%zu\n", cw.rle_encoded.size());
    for (int c = 0; c < ncomp; ++c) {
        Box3D got = decompress(dir + "/compressed-wavelet-7-1-" + std::to_string(c) + "-3.xz", 7, 1, c, 3);
        std::ofstream o(dir + "/cells-" + std::to_string(c) + ".raw", std::ios::binary);
        o.write(reinterpret_cast<const char*>(got.data()), (std::streamsize)(sizeof(float) * got.data_size()));
        if (!o || got.width() != W || got.height() != H || got.depth() != D) {
            std::fprintf(stderr, "component %d: cannot write the cells, or other dimensions\n", c);
            return 1;
        }
    }
    return 0;
}
