// decompressor.cpp — C++ mirror of the reference's decompressor
// (src/decompressor.cpp:14-255).  xz decode on the host; rle_decode and the
// inverse transform on the GPU (wc_inverse_host; wc_inverse_levels_host for
// a file of the opt-in multi-level mode, told by its header).
#include <lzma.h>

#include <cstdint>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <vector>

#include "host_ctx.h"
#include "wavelet_amd/codec_extras.h"
#include "wavelet_amd/decompressor.h"
#include "wavelet_amd/xz_pool.h"

namespace wavelet_amd {

std::vector<float> rle_decode(const std::vector<std::pair<int, float>>& rle, int total) {
    std::vector<float> out(total > 0 ? total : 0, 0.0f);
    long long idx = 0;
    for (const auto& pr : rle) {
        idx += pr.first;
        if (idx >= 0 && idx < total) out[idx++] = pr.second;
    }
    return out;
}

std::string xz_decompress(const std::string& xz) {
    // lzma_stream_decoder(UINT64_MAX, LZMA_CONCATENATED), output doubled until
    // the stream ends (src/decompressor.cpp:188-220).
    lzma_stream strm = LZMA_STREAM_INIT;
    if (lzma_stream_decoder(&strm, UINT64_MAX, LZMA_CONCATENATED) != LZMA_OK) fatal("Failed to initialize LZMA decoder.");
    std::vector<uint8_t> out(4096);
    strm.next_in = reinterpret_cast<const uint8_t*>(xz.data());
    strm.avail_in = xz.size();
    strm.next_out = out.data();
    strm.avail_out = out.size();
    for (;;) {
        const lzma_ret r = lzma_code(&strm, LZMA_FINISH);
        if (r == LZMA_STREAM_END) break;
        if (r != LZMA_OK) {
            lzma_end(&strm);
            fatal("LZMA decompression failed with code: " + std::to_string((int)r));
        }
        const size_t old = out.size();
        out.resize(old * 2);
        strm.next_out = out.data() + old;
        strm.avail_out = old;
    }
    const size_t used = out.size() - strm.avail_out;
    lzma_end(&strm);
    return std::string(reinterpret_cast<const char*>(out.data()), used);
}

static std::string read_file(const std::string& path) {
    std::error_code ec;
    const auto size = std::filesystem::file_size(path, ec);
    if (ec) fatal("Error getting file size: " + ec.message() + " " + path);
    std::ifstream f(path, std::ios::binary);
    if (!f) fatal("Failed to open file: " + path);
    std::string data(size, '\0');
    if (!f.read(data.data(), (std::streamsize)size)) fatal("Failed to read file: " + path);
    return data;
}

std::string standard_payload(std::string payload) {
    int L = 0, V = 0;
    if (payload.size() < 20 ||
        wc_payload_packed(reinterpret_cast<const uint8_t*>(payload.data()), 20, &L, &V) != WC_OK || V == 0)
        return payload;  // a standard payload, or a header the decoders refuse in their own words
    int32_t hdr[5];
    std::memcpy(hdr, payload.data(), sizeof hdr);
    uint64_t len = 0;
    if (hdr[4] < 0 || wc_packed_size(reinterpret_cast<const uint8_t*>(payload.data()), payload.size(), &len) != WC_OK ||
        len > payload.size())
        fatal("Deserialization failed: truncated or malformed packed payload");
    const wc_unit u{0, hdr[0], hdr[1], hdr[2], 0};
    std::vector<uint8_t> in(payload.size() + 8);  // one unit at offset 4 (chunks 8-byte aligned)
    std::memcpy(in.data() + 4, payload.data(), payload.size());
    const uint64_t poff = 4;
    std::vector<uint8_t> out(wc_payload_bound(&u, 1));
    uint64_t off[2] = {0, 0};
    uint32_t kept = 0;
    wc_ctx* c = thread_ctx();
    check(c, wc_unpack_host(c, in.data(), &poff, &u, 1, out.data(), out.size(), off, &kept), "GPU unpack");
    return std::string(reinterpret_cast<const char*>(out.data() + off[0]), 20 + 8ull * kept);
}

// A file's bytes after xz: the levels of a packed unit, 0 for anything else (a standard payload, or a header
// the decoders refuse in their own words).  A packed unit that is truncated or malformed exits here, as in
// standard_payload(): the packed host calls size their upload from the header and the width table.
static int packed_levels(const std::string& payload) {
    int L = 0, V = 0;
    if (payload.size() < 20 ||
        wc_payload_packed(reinterpret_cast<const uint8_t*>(payload.data()), 20, &L, &V) != WC_OK || V == 0)
        return 0;
    int32_t hdr[5];
    std::memcpy(hdr, payload.data(), sizeof hdr);
    uint64_t len = 0;
    if (hdr[4] < 0 || wc_packed_size(reinterpret_cast<const uint8_t*>(payload.data()), payload.size(), &len) != WC_OK ||
        len > payload.size())
        fatal("Deserialization failed: truncated or malformed packed payload");
    return L;
}

}  // namespace wavelet_amd

using namespace wavelet_amd;

CompressedWavelet deserialize_compressed_wavelet(const std::string& data) {
    CompressedWavelet cw;
    auto get = [&data](size_t off) {
        int32_t v = 0;
        if (off + 4 <= data.size()) std::memcpy(&v, data.data() + off, 4);
        return v;
    };
    cw.shape = {get(0), get(4), get(8)};
    cw.coeff_shape = {get(12)};
    const int32_t n = get(16);
    if (n < 0 || 20 + 8ull * (uint64_t)n > data.size()) fatal("Deserialization failed: truncated payload");
    cw.rle_encoded.resize(n);
    for (int32_t i = 0; i < n; ++i) {
        float v;
        std::memcpy(&v, data.data() + 24 + 8ull * i, 4);
        cw.rle_encoded[i] = {get(20 + 8ull * i), v};
    }
    return cw;
}

Box3D inverse_wavelet_decompose(std::vector<float> flat, int x, int y, int z) {
    Box3D out(x, y, z);
    if (out.data_size() == 0) return out;
    if (flat.size() < out.data_size()) fatal("inverse_wavelet_decompose: flat shorter than x*y*z");
    wc_ctx* c = thread_ctx();
    wc_unit u{0, x, y, z, 0};
    check(c, wc_inverse_flat_host(c, flat.data(), &u, 1, out.data()), "GPU inverse transform");
    return out;
}

Box3D decompress(std::string file_path, int /*time*/, int /*level*/, int /*component*/, int /*box_idx*/) {
    flush_writes(file_path);  // this file, if compress() queued it (write-behind, opt-in), is complete first
    const std::string payload = xz_decompress(read_file(file_path));
    const int packedL = packed_levels(payload);  // a packed file is decoded from its packed bytes
    if (payload.size() < 20) fatal("Deserialization failed: payload shorter than its header");
    int32_t hdr[5];
    std::memcpy(hdr, payload.data(), sizeof hdr);
    Box3D out(hdr[0] > 0 ? hdr[0] : 0, hdr[1] > 0 ? hdr[1] : 0, hdr[2] > 0 ? hdr[2] : 0);
    if (out.data_size() == 0) return out;
    // stage as one unit at offset 4 (pairs 8-byte aligned)
    std::vector<uint8_t> buf(payload.size() + 8);
    std::memcpy(buf.data() + 4, payload.data(), payload.size());
    const uint64_t off = 4;
    wc_unit u{0, hdr[0], hdr[1], hdr[2], 0};
    wc_ctx* c = thread_ctx();
    // ncoeff < 0: a multi-level payload (not the reference's format; the header carries its levels)
    if (packedL)
        check(c, wc_inverse_packed_host(c, buf.data(), &off, &u, 1, nullptr, out.data()), "GPU decompress");
    else if (hdr[3] < 0)
        check(c, wc_inverse_levels_host(c, buf.data(), &off, &u, 1, nullptr, out.data()), "GPU decompress");
    else
        check(c, wc_inverse_host(c, buf.data(), &off, &u, 1, out.data()), "GPU decompress");
    return out;
}

Box3D wavelet_amd::decompress_coarse(const std::string& file_path, int reduce) {
    flush_writes(file_path);
    const std::string payload = xz_decompress(read_file(file_path));
    const int packedL = packed_levels(payload);  // a packed file is decoded from its packed bytes
    if (payload.size() < 20) fatal("Deserialization failed: payload shorter than its header");
    int32_t hdr[5];
    std::memcpy(hdr, payload.data(), sizeof hdr);
    if (hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) fatal("Deserialization failed: negative dimensions");
    if (reduce < 0 || reduce > WC_MAX_LEVELS)
        fatal("decompress_coarse: reduce " + std::to_string(reduce) + " outside 0.." + std::to_string(WC_MAX_LEVELS));
    const wc_unit u{0, hdr[0], hdr[1], hdr[2], 0};
    const int32_t r = reduce;
    wc_unit o;
    uint64_t extent = 0;
    wc_coarse_units(&u, &r, 1, &o, &extent);
    Box3D out(o.nx, o.ny, o.nz);
    if ((uint64_t)hdr[0] * (uint64_t)hdr[1] * (uint64_t)hdr[2] == 0) return out;
    std::vector<uint8_t> buf(payload.size() + 8);
    std::memcpy(buf.data() + 4, payload.data(), payload.size());
    const uint64_t off = 4;
    wc_ctx* c = thread_ctx();
    // levels = NULL: the file's header tells them; a reduce beyond them is refused there
    if (packedL)
        check(c, wc_inverse_packed_coarse_host(c, buf.data(), &off, &u, 1, nullptr, &r, &o, out.data()),
              "GPU coarse decompress");
    else
        check(c, wc_inverse_coarse_host(c, buf.data(), &off, &u, 1, nullptr, &r, &o, out.data()), "GPU coarse decompress");
    return out;
}

Box3D wavelet_amd::decompress_region(const std::string& file_path, std::array<int, 3> lo, std::array<int, 3> hi,
                                     int reduce) {
    flush_writes(file_path);
    // a packed file is unpacked first: the direct region call measured slower than unpack + decode
    const std::string payload = standard_payload(xz_decompress(read_file(file_path)));
    if (payload.size() < 20) fatal("Deserialization failed: payload shorter than its header");
    int32_t hdr[5];
    std::memcpy(hdr, payload.data(), sizeof hdr);
    if (hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) fatal("Deserialization failed: negative dimensions");
    int L = 0;
    if (wc_payload_levels(reinterpret_cast<const uint8_t*>(payload.data()), 20, &L) != WC_OK)
        fatal("Deserialization failed: malformed payload header");
    if (reduce < 0 || reduce > L)
        fatal("decompress_region: reduce " + std::to_string(reduce) + " outside 0.." + std::to_string(L));
    const std::string box = std::to_string(hdr[0]) + "x" + std::to_string(hdr[1]) + "x" + std::to_string(hdr[2]);
    for (int a = 0; a < 3; ++a)
        if (lo[a] < 0 || hi[a] <= lo[a] || hi[a] > hdr[a])
            fatal("decompress_region: the region must be non-empty and inside the box " + box);
    const wc_region want{lo[0], lo[1], lo[2], hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    wc_region g;
    if (wc_region_align(hdr[0], hdr[1], hdr[2], L, &want, &g) != WC_OK)
        fatal("decompress_region: " + std::to_string(L) + " level(s) need W, H and D of " + box + " divisible by " +
              std::to_string(1 << L));
    const wc_unit u{0, hdr[0], hdr[1], hdr[2], 0};
    const int32_t r = reduce, lv = L;
    wc_unit o;
    uint64_t extent = 0;
    wc_region_units(&u, &g, &r, 1, &o, &extent);
    std::vector<float> cells(extent);
    std::vector<uint8_t> buf(payload.size() + 8);
    std::memcpy(buf.data() + 4, payload.data(), payload.size());
    const uint64_t off = 4;
    wc_ctx* c = thread_ctx();
    check(c, wc_inverse_region_host(c, buf.data(), &off, &u, 1, &lv, &r, &g, &o, cells.data()), "GPU region decompress");
    // the crop [lo >> r, ceil(hi / 2^r)) of the aligned region's box
    const int up = (1 << r) - 1;
    const int a0[3] = {(lo[0] >> r) - (g.x0 >> r), (lo[1] >> r) - (g.y0 >> r), (lo[2] >> r) - (g.z0 >> r)};
    const int n[3] = {((hi[0] + up) >> r) - (lo[0] >> r), ((hi[1] + up) >> r) - (lo[1] >> r),
                      ((hi[2] + up) >> r) - (lo[2] >> r)};
    Box3D out(n[0], n[1], n[2]);
    for (int z = 0; z < n[2]; ++z)
        for (int y = 0; y < n[1]; ++y)
            std::memcpy(out.data() + (size_t)n[0] * (y + (size_t)n[1] * z),
                        cells.data() + a0[0] + (size_t)o.nx * ((a0[1] + y) + (size_t)o.ny * (a0[2] + z)),
                        sizeof(float) * n[0]);
    return out;
}
