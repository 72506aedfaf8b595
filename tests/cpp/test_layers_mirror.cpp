// test_layers_mirror.cpp — split_budget / split_thresh / merge of the C++ mirror
// (include/wavelet_amd/codec_extras.h):
//   test_layers_mirror MODE VALUE OUT.bin IN0.bin IN1.bin ...
// reads one serialized payload per IN file (a packed unit goes through standard_payload first),
// deserializes them, calls split_budget(structs, VALUE) for MODE = ratio or split_thresh(structs,
// VALUE) for MODE = thresh, merges the two layers again, and writes to OUT.bin every base, then
// every rest, then every merged struct, each as a uint64 length and the serialized bytes.
// Driven by tests/test_gpu_layers_mirror.py, which compares them with the restatement's payloads.
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
        std::fprintf(stderr, "usage: test_layers_mirror ratio|thresh VALUE OUT.bin IN.bin...\n");
        return 2;
    }
    const std::string mode = argv[1];
    const double value = std::strtod(argv[2], nullptr);
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
    const wavelet_amd::Layers l =
        mode == "ratio" ? wavelet_amd::split_budget(in, value) : wavelet_amd::split_thresh(in, (float)value);
    const std::vector<CompressedWavelet> merged = wavelet_amd::merge(l.rest, l.base);
    std::ofstream o(argv[3], std::ios::binary);
    for (const std::vector<CompressedWavelet>* v : {&l.base, &l.rest, &merged})
        for (const CompressedWavelet& cw : *v) {
            const std::string s = wavelet_amd::serialize_compressed_wavelet(cw);
            const uint64_t len = s.size();
            o.write(reinterpret_cast<const char*>(&len), 8);
            o.write(s.data(), (std::streamsize)s.size());
        }
    return o ? 0 : 1;
}
