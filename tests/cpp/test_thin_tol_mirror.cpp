// test_thin_tol_mirror.cpp — thin_rmse / split_rmse of the C++ mirror (include/wavelet_amd/codec_extras.h):
//   test_thin_tol_mirror MODE RMSE OUT.bin IN0.bin IN1.bin ...
// reads one serialized payload per IN file (a packed unit goes through standard_payload first),
// deserializes them, calls thin_rmse(structs, RMSE) for MODE = thin, or split_rmse(structs, RMSE)
// followed by merge(base, rest) for MODE = split, and writes the results to OUT.bin, each as a uint64
// length and the serialized bytes: the thinned structs, or every base, then every rest, then every
// merged struct.  Driven by tests/test_gpu_thin_tol_mirror.py, which compares them with the
// restatement's payloads.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "wavelet_amd/codec_extras.h"
#include "wavelet_amd/decompressor.h"

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: test_thin_tol_mirror thin|split RMSE OUT.bin IN.bin...\n");
        return 2;
    }
    const std::string mode = argv[1];
    const double rmse = std::strtod(argv[2], nullptr);
    std::vector<CompressedWavelet> in;
    for (int i = 4; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (!f && bytes.empty()) {
            std::fprintf(stderr, "cannot read %s\n", argv[i]);
            return 1;
        }
        in.push_back(deserialize_compressed_wavelet(wavelet_amd::standard_payload(bytes)));
    }
    std::vector<std::vector<CompressedWavelet>> lists;
    if (mode == "thin") {
        lists.push_back(wavelet_amd::thin_rmse(in, rmse));
    } else {
        const wavelet_amd::Layers l = wavelet_amd::split_rmse(in, rmse);
        lists.push_back(l.base);
        lists.push_back(l.rest);
        lists.push_back(wavelet_amd::merge(l.base, l.rest));
    }
    std::ofstream o(argv[3], std::ios::binary);
    for (const auto& list : lists)
        for (const CompressedWavelet& cw : list) {
            const std::string s = wavelet_amd::serialize_compressed_wavelet(cw);
            const uint64_t len = s.size();
            o.write(reinterpret_cast<const char*>(&len), 8);
            o.write(s.data(), (std::streamsize)s.size());
        }
    return o ? 0 : 1;
}
