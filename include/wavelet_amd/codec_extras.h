// codec_extras.h — routines the reference keeps file-static
// (src/compressor.cpp:24-185, src/decompressor.cpp:14-30), exported here so the
// reference's unit tests can be restated against this library.
#pragma once

#include <array>
#include <string>
#include <utility>
#include <vector>

#include "box-structs.h"

namespace wavelet_amd {

// wavelet_decompose (GPU): Box3D -> flat coefficients, x slowest.
std::vector<float> wavelet_decompose(const Box3D& box);

// rle_encode over an explicit mask (host; the GPU path never materialises a mask).
std::vector<std::pair<int, float>> rle_encode(const std::vector<bool>& mask, const std::vector<float>& values);

// serialize_compressed_wavelet (host).
std::string serialize_compressed_wavelet(const CompressedWavelet& compressed);

// rle_decode (host; the GPU decode is K5 inside decompress()).
std::vector<float> rle_decode(const std::vector<std::pair<int, float>>& rle_encoded, int total_length);

// xz helpers: liblzma easy encoder preset 6 + CRC64, and the stream decoder.
std::string xz_compress(const std::string& payload);
std::string xz_decompress(const std::string& xz);

// decompress() at 1/2^reduce resolution (GPU, wc_inverse_coarse_host; not in the
// reference): the box (W, H, D) >> reduce whose cells are the means of the
// 2^reduce-cubes of decompress()'s box up to fp32 rounding, decoded from the
// low-pass corner of the file's coefficients alone.  reduce = 0 is decompress().
// The file's levels (1 for a reference-format file) must be >= reduce and
// 2^reduce must divide W, H and D; otherwise it exits with a message, as the
// other read errors do.
Box3D decompress_coarse(const std::string& file_path, int reduce);

// The cells [lo, hi) of decompress()'s box (hi exclusive, x, y, z in cells of the
// full box), or with reduce = r >= 1 the cells [lo >> r, ceil(hi / 2^r)) of
// decompress_coarse()'s (GPU, wc_inverse_region_host; not in the reference).  The
// region is rounded outward to multiples of 2^L, L the file's levels
// (wc_region_align), decoded from the coefficients it depends on alone, and
// cropped on the host; the bits are those of the crop of the full decode.  A
// region that is empty or not inside the box, dimensions that 2^L does not
// divide, or a reduce beyond the file's levels: it exits with a message, as the
// other read errors do.
Box3D decompress_region(const std::string& file_path, std::array<int, 3> lo, std::array<int, 3> hi, int reduce = 0);

// compress() with a tolerated RMSE in place of keep (GPU, wc_forward_levels_tol_host;
// not in the reference): every component of the box is transformed with the levels
// its dimensions admit, at most `levels` (wc_levels_for), and keeps what the
// per-level thresholds of the tolerance leave, so that its round-trip RMSE stays
// within `rmse` up to fp32 rounding.  Writes the usual per-box .xz files, which
// decompress() and decompress_coarse() read as they are, and returns the structs.
// A component with cells and an odd dimension has no such bound: the call exits
// with the library's message, as the other errors do.
std::vector<CompressedWavelet> compress_rmse(multiBox3D& box, std::vector<int> components, int levels, double rmse,
                                             int time, int level, int box_index, std::string compressed_dir);

// compress() with a pointwise error bound in place of keep (GPU,
// wc_forward_levels_maxerr_host; not in the reference): every component of the box is
// transformed with the levels its dimensions admit, at most `levels` (wc_levels_for),
// under the highest threshold of the mode's search whose round trip, verified on the
// device, leaves no cell further than `maxerr` from the original (a bound too tight for
// fp32 keeps every non-zero coefficient).  Writes the usual per-box .xz files, which
// decompress(), decompress_coarse() and decompress_region() read as they are, and
// returns the structs.  A component with cells and an odd dimension, or a negative or
// NaN bound, exits with the library's message, as the other errors do.
std::vector<CompressedWavelet> compress_maxerr(multiBox3D& box, std::vector<int> components, int levels, double maxerr,
                                               int time, int level, int box_index, std::string compressed_dir);

// compress() under a size budget in place of keep (GPU, wc_forward_levels_budget_host;
// not in the reference): every component of N cells is transformed with the levels
// its dimensions admit, at most `levels`, and keeps its (max(20, floor(4 N / ratio)) -
// 20) / 8 largest weighted coefficients and never more, so that its serialized
// payload (before xz) is at most 1 / ratio of its 4 N bytes, or the 20-byte header.
// Coefficients that tie at the boundary are all dropped.  Writes the usual per-box
// .xz files, which decompress(), decompress_coarse() and decompress_region() read as
// they are, and returns the structs.  A component with cells and an odd dimension
// exits with the library's message, as the other errors do.
std::vector<CompressedWavelet> compress_budget(multiBox3D& box, std::vector<int> components, int levels, double ratio,
                                               int time, int level, int box_index, std::string compressed_dir);

// Compressed structs thinned in the compressed domain (GPU, wc_thin_budget_host /
// wc_thin_thresh_host; not in the reference): what compress_budget's selection at
// `ratio`, or the test |c| > thresh on every level, leaves of the array each struct
// decodes to, without its cells or dense coefficients in between.  thin_budget's
// pair budget is compress_budget's: (max(20, floor(4 N / ratio)) - 20) / 8 for a
// component of N cells; ties at the boundary are all dropped.  A struct made with
// thresh = 0 (or a generous budget) thinned at `ratio` is byte for byte what
// compress_budget gives at `ratio` whenever it holds every candidate.  The levels come
// from coeff_shape (the header's ncoeff field).  Nothing is written to disk.  A
// non-positive ratio, or a NaN or negative thresh, exits with a message, as the other
// errors do.
std::vector<CompressedWavelet> thin_budget(const std::vector<CompressedWavelet>& compressed, double ratio);
std::vector<CompressedWavelet> thin_thresh(const std::vector<CompressedWavelet>& compressed, float thresh);

// Compressed structs thinned to a tolerated RMSE in the compressed domain (GPU,
// wc_thin_tol_host; not in the reference): compress_rmse's per-level selection on the
// array each struct decodes to.  `rmse` bounds the error this thinning ADDS (for the
// real-number transform): a struct made at rmse0 and thinned at rmse1 is within
// sqrt(rmse0^2 + rmse1^2) of the original component.  A struct that holds every
// non-zero coefficient (thresh = 0) thinned at `rmse` is byte for byte what
// compress_rmse gives at `rmse`.  Components with cells need even dimensions (the
// library's message otherwise); a NaN or negative rmse exits with a message.
std::vector<CompressedWavelet> thin_rmse(const std::vector<CompressedWavelet>& compressed, double rmse);

// Progressive layers in the compressed domain (GPU, wc_split_budget_host /
// wc_split_thresh_host / wc_merge_host; not in the reference).  split_*: base[i] is
// exactly thin_budget's / thin_thresh's struct for compressed[i]; rest[i] holds every
// other non-zero, non-NaN coefficient of it, so that merge(base, rest) is the struct
// again (byte for byte when serialized, for every struct an encoder of this project
// made).  Splitting `rest` again yields the next layer.  merge: the union of a[i]
// and b[i]; two layers of one component that hold a coefficient at the same position
// exit with the library's message.  Nothing is written to disk.
struct Layers {
    std::vector<CompressedWavelet> base, rest;
};
Layers split_budget(const std::vector<CompressedWavelet>& compressed, double ratio);
Layers split_thresh(const std::vector<CompressedWavelet>& compressed, float thresh);
Layers split_rmse(const std::vector<CompressedWavelet>& compressed, double rmse);  // base[i] = thin_rmse's struct (wc_split_tol_host)
std::vector<CompressedWavelet> merge(const std::vector<CompressedWavelet>& a, const std::vector<CompressedWavelet>& b);

// compress() whose files hold packed units (GPU, wc_pack_host after the forward; not
// a reference format, include/wavelet_amd.h "Opt-in packed payloads"): each kept
// value stored in its top `vbytes` bytes (4: lossless; 3, 2: rounded to nearest even,
// an added error of at most 2^-16 or 2^-8 of the box's norm), the runs as bit planes.
// Same file names; decompress(), decompress_coarse() and decompress_region() recognise
// such files by their headers: decompress() and decompress_coarse() decode them from their
// packed bytes (wc_inverse_packed_host, wc_inverse_packed_coarse_host: the bits of unpacking
// first, without the standard payload); decompress_region() unpacks them first
// (wc_unpack_host), the path that measured faster for a region.  The returned
// structs describe the payloads before packing.  vbytes outside 2..4 or a component
// of more than WC_PACK_MAX_CELLS cells: it exits with a message, as the other errors do.
std::vector<CompressedWavelet> compress_packed(multiBox3D& box, std::vector<int> components, double keep, int vbytes,
                                               int time, int level, int box_index, std::string compressed_dir);

// The standard payload of a file's bytes after xz: a packed unit unpacked on the GPU
// (wc_unpack_host), anything else returned as it is.
std::string standard_payload(std::string payload);

}  // namespace wavelet_amd
