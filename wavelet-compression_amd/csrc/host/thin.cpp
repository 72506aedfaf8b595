// thin.cpp — thin_budget, thin_thresh and thin_rmse of the C++ mirror (include/wavelet_amd/codec_extras.h):
// CompressedWavelet structs to smaller ones in the compressed domain, in one
// wc_thin_budget_host / wc_thin_thresh_host / wc_thin_tol_host call.  Not in the reference.
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

std::vector<CompressedWavelet> thin(const std::vector<CompressedWavelet>& in, const double* ratio, const float* thresh,
                                    const double* rmse = nullptr) {
    const int n = static_cast<int>(in.size());
    if (n == 0) return {};
    // the serialized structs back to back, each at an offset == 4 (mod 8)
    std::vector<std::string> ser(n);
    std::vector<uint64_t> offsets(n);
    std::vector<wc_unit> units(n);
    std::vector<uint32_t> pairs(n);
    uint64_t cur = 4;
    for (int c = 0; c < n; ++c) {
        if (in[c].shape.size() != 3) fatal("thin: a CompressedWavelet without a 3-D shape");
        ser[c] = serialize_compressed_wavelet(in[c]);
        offsets[c] = cur;
        cur += (ser[c].size() + 4 + 7) / 8 * 8;
        units[c] = wc_unit{0, in[c].shape[0], in[c].shape[1], in[c].shape[2], 0};
        if (ratio) {  // as compress_budget: at most max(20, floor(4 N / ratio)) bytes, 20 of header, 8 per pair
            const double N = (double)in[c].shape[0] * (double)in[c].shape[1] * (double)in[c].shape[2];
            const double bytes = std::max(20.0, std::floor(4.0 * N / *ratio));
            pairs[c] = (uint32_t)std::min((bytes - 20.0) / 8.0, 4294967295.0);
        }
    }
    std::vector<uint8_t> buf(cur + 8, 0);
    for (int c = 0; c < n; ++c) std::memcpy(buf.data() + offsets[c], ser[c].data(), ser[c].size());
    const uint64_t cap = wc_thin_bound(units.data(), n, ratio ? pairs.data() : nullptr);
    std::vector<uint8_t> out(cap);
    std::vector<uint64_t> ooff(n + 1);
    std::vector<uint32_t> kept(n);
    wc_ctx* ctx = thread_ctx();
    if (ratio) {
        check(ctx, wc_thin_budget_host(ctx, buf.data(), offsets.data(), units.data(), n, nullptr, pairs.data(), out.data(),
                                       cap, ooff.data(), kept.data(), nullptr, nullptr),
              "GPU thinning");
    } else if (rmse) {
        const std::vector<double> tol((size_t)n, *rmse);
        check(ctx, wc_thin_tol_host(ctx, buf.data(), offsets.data(), units.data(), n, nullptr, tol.data(), out.data(), cap,
                                    ooff.data(), kept.data(), nullptr, nullptr),
              "GPU thinning");
    } else {
        const std::vector<float> th((size_t)n * WC_MAX_LEVELS, *thresh);
        check(ctx, wc_thin_thresh_host(ctx, buf.data(), offsets.data(), units.data(), n, nullptr, th.data(), out.data(),
                                       cap, ooff.data(), kept.data()),
              "GPU thinning");
    }
    std::vector<CompressedWavelet> res(n);
    for (int c = 0; c < n; ++c) {
        res[c] = deserialize_compressed_wavelet(
            std::string(reinterpret_cast<const char*>(out.data() + ooff[c]), 20 + 8ull * kept[c]));
        for (const auto& pr : res[c].rle_encoded)
            if (std::fabs((double)pr.second) > INT16_MAX) res[c].need32 = true;  // as compress()
    }
    return res;
}

}  // namespace

std::vector<CompressedWavelet> thin_budget(const std::vector<CompressedWavelet>& compressed, double ratio) {
    if (!(ratio > 0.0)) fatal("thin_budget: the ratio must be positive");
    return thin(compressed, &ratio, nullptr);
}

std::vector<CompressedWavelet> thin_thresh(const std::vector<CompressedWavelet>& compressed, float thresh) {
    if (!(thresh >= 0.0f)) fatal("thin_thresh: the threshold must be >= 0");
    return thin(compressed, nullptr, &thresh);
}

std::vector<CompressedWavelet> thin_rmse(const std::vector<CompressedWavelet>& compressed, double rmse) {
    if (!(rmse >= 0.0)) fatal("thin_rmse: the tolerated RMSE must be >= 0");
    return thin(compressed, nullptr, nullptr, &rmse);
}

}  // namespace wavelet_amd
