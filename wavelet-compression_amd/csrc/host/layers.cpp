// layers.cpp — split_budget, split_thresh, split_rmse and merge of the C++ mirror
// (include/wavelet_amd/codec_extras.h): CompressedWavelet structs to (base, rest)
// layers and layers back to one struct, in the compressed domain, each in one
// wc_split_budget_host / wc_split_thresh_host / wc_split_tol_host / wc_merge_host
// call.  Not in the reference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_ctx.h"
#include "wavelet_amd/codec_extras.h"
#include "wavelet_amd/decompressor.h"

namespace wavelet_amd {

namespace {

// the serialized structs back to back, each at an offset == 4 (mod 8)
struct Laid {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> offsets;
    std::vector<wc_unit> units;
};
Laid lay_out(const std::vector<CompressedWavelet>& in, const char* who) {
    const int n = static_cast<int>(in.size());
    Laid l;
    l.offsets.resize(n);
    l.units.resize(n);
    std::vector<std::string> ser(n);
    uint64_t cur = 4;
    for (int c = 0; c < n; ++c) {
        if (in[c].shape.size() != 3) fatal(std::string(who) + ": a CompressedWavelet without a 3-D shape");
        ser[c] = serialize_compressed_wavelet(in[c]);
        l.offsets[c] = cur;
        cur += (ser[c].size() + 4 + 7) / 8 * 8;
        l.units[c] = wc_unit{0, in[c].shape[0], in[c].shape[1], in[c].shape[2], 0};
    }
    l.buf.assign(cur + 8, 0);
    for (int c = 0; c < n; ++c) std::memcpy(l.buf.data() + l.offsets[c], ser[c].data(), ser[c].size());
    return l;
}

std::vector<CompressedWavelet> structs_of(const std::vector<uint8_t>& out, const std::vector<uint64_t>& off,
                                          const std::vector<uint32_t>& pairs) {
    std::vector<CompressedWavelet> res(pairs.size());
    for (size_t c = 0; c < pairs.size(); ++c) {
        res[c] = deserialize_compressed_wavelet(
            std::string(reinterpret_cast<const char*>(out.data() + off[c]), 20 + 8ull * pairs[c]));
        for (const auto& pr : res[c].rle_encoded)
            if (std::fabs((double)pr.second) > INT16_MAX) res[c].need32 = true;  // as compress()
    }
    return res;
}

Layers split(const std::vector<CompressedWavelet>& in, const double* ratio, const float* thresh,
             const double* rmse = nullptr) {
    const int n = static_cast<int>(in.size());
    if (n == 0) return {};
    const Laid l = lay_out(in, "split");
    std::vector<uint32_t> pairs(n);
    for (int c = 0; c < n && ratio; ++c) {  // as thin_budget: at most max(20, floor(4 N / ratio)) bytes
        const double N = (double)in[c].shape[0] * (double)in[c].shape[1] * (double)in[c].shape[2];
        const double bytes = std::max(20.0, std::floor(4.0 * N / *ratio));
        pairs[c] = (uint32_t)std::min((bytes - 20.0) / 8.0, 4294967295.0);
    }
    uint64_t bcap = 0, rcap = 0;
    (void)wc_split_bound(l.units.data(), n, ratio ? pairs.data() : nullptr, &bcap, &rcap);
    std::vector<uint8_t> base(bcap), rest(rcap);
    std::vector<uint64_t> boff(n + 1), roff(n + 1);
    std::vector<uint32_t> kept(n), rpairs(n);
    wc_ctx* ctx = thread_ctx();
    if (ratio) {
        check(ctx,
              wc_split_budget_host(ctx, l.buf.data(), l.offsets.data(), l.units.data(), n, nullptr, pairs.data(),
                                   base.data(), bcap, boff.data(), kept.data(), rest.data(), rcap, roff.data(),
                                   rpairs.data(), nullptr, nullptr),
              "GPU split");
    } else if (rmse) {
        const std::vector<double> tol((size_t)n, *rmse);
        check(ctx,
              wc_split_tol_host(ctx, l.buf.data(), l.offsets.data(), l.units.data(), n, nullptr, tol.data(), base.data(),
                                bcap, boff.data(), kept.data(), rest.data(), rcap, roff.data(), rpairs.data(), nullptr,
                                nullptr),
              "GPU split");
    } else {
        const std::vector<float> th((size_t)n * WC_MAX_LEVELS, *thresh);
        check(ctx,
              wc_split_thresh_host(ctx, l.buf.data(), l.offsets.data(), l.units.data(), n, nullptr, th.data(), base.data(),
                                   bcap, boff.data(), kept.data(), rest.data(), rcap, roff.data(), rpairs.data()),
              "GPU split");
    }
    return Layers{structs_of(base, boff, kept), structs_of(rest, roff, rpairs)};
}

}  // namespace

Layers split_budget(const std::vector<CompressedWavelet>& compressed, double ratio) {
    if (!(ratio > 0.0)) fatal("split_budget: the ratio must be positive");
    return split(compressed, &ratio, nullptr);
}

Layers split_thresh(const std::vector<CompressedWavelet>& compressed, float thresh) {
    if (!(thresh >= 0.0f)) fatal("split_thresh: the threshold must be >= 0");
    return split(compressed, nullptr, &thresh);
}

Layers split_rmse(const std::vector<CompressedWavelet>& compressed, double rmse) {
    if (!(rmse >= 0.0)) fatal("split_rmse: the tolerated RMSE must be >= 0");
    return split(compressed, nullptr, nullptr, &rmse);
}

std::vector<CompressedWavelet> merge(const std::vector<CompressedWavelet>& a, const std::vector<CompressedWavelet>& b) {
    if (a.size() != b.size()) fatal("merge: one struct of each layer per component");
    const int n = static_cast<int>(a.size());
    if (n == 0) return {};
    const Laid la = lay_out(a, "merge"), lb = lay_out(b, "merge");
    const uint64_t cap = wc_merge_bound(la.units.data(), n);
    std::vector<uint8_t> out(cap);
    std::vector<uint64_t> off(n + 1);
    std::vector<uint32_t> pairs(n);
    wc_ctx* ctx = thread_ctx();
    check(ctx,
          wc_merge_host(ctx, la.buf.data(), la.offsets.data(), lb.buf.data(), lb.offsets.data(), la.units.data(), n,
                        nullptr, out.data(), cap, off.data(), pairs.data()),
          "GPU merge");
    return structs_of(out, off, pairs);
}

}  // namespace wavelet_amd
