"""Python mirror of the reference's codec interface, running on the HIP path.

Same names, argument meaning and error behaviour as
carsonmw3/wavelet-compression:

  compress(box, components, keep, time, level, box_index, compressed_dir)
        src/compressor.h:9-15 / src/compressor.cpp:192-297
  decompress(file_path, time, level, component, box_idx)
        src/decompressor.h:6-10 / src/decompressor.cpp:238-255
  deserialize_compressed_wavelet(data)          src/decompressor.h:14, .cpp:35-74
  inverse_wavelet_decompose(flat, x, y, z)      src/decompressor.h:18, .cpp:79-159
  calc_rmse_per_box(actual, pred, num_components) src/calc-loss.h:6-8
  calc_adj_loss(rmse, range)                    src/calc-loss.cpp:49-51
  calc_size(path)                               src/calc-loss.cpp:55-65

A Box3D is a float32 numpy array of shape (D, H, W) — x fastest in memory,
exactly Grid3D's `x + W*(y + H*z)` layout (src/grid.h:15-19).  A multiBox3D
is a list of them.  All transform / threshold / pack / unpack / RMSE work runs
in the HIP kernels; the xz stage is host-side (Python's lzma is liblzma).
"""
from __future__ import annotations

import lzma
import os
import sys
import threading
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from . import capi

# Reference: lzma_easy_encoder(&strm, 6, LZMA_CHECK_CRC64) (src/compressor.cpp:261-262)
XZ_PRESET = 6
XZ_CHECK = lzma.CHECK_CRC64


def parse_xz_preset(text: str) -> int:
    """"0".."9", optionally followed by "e" (extreme) -> lzma preset value."""
    t = str(text)
    if len(t) in (1, 2) and t[0].isdigit() and (len(t) == 1 or t[1] == "e"):
        return int(t[0]) | (lzma.PRESET_EXTREME if len(t) == 2 else 0)
    raise ValueError(f"xz preset: 0-9, optionally followed by e, not {text!r}")


def xz_preset() -> int:
    """The preset of compress(): the reference's 6, or $WCAMD_XZ_PRESET (SURVEY
    §8(f) row 1, an optional faster preset; the reference's stream decoder,
    src/decompressor.cpp:189, reads any).  The C++ host library reads the same
    variable (include/wavelet_amd/xz_pool.h)."""
    import os
    v = os.environ.get("WCAMD_XZ_PRESET")
    return XZ_PRESET if not v else parse_xz_preset(v)

_ctx_lock = threading.Lock()
_ctxs: dict = {}


def context(device: int = 0) -> capi.Context:
    """Per-(thread, device) codec context (one wc_ctx per device per host thread)."""
    key = (threading.get_ident(), device)
    with _ctx_lock:
        c = _ctxs.get(key)
        if c is None:
            c = capi.Context(device)
            _ctxs[key] = c
        return c


@dataclass
class CompressedWavelet:
    """src/box-structs.h:65-70."""
    shape: List[int] = field(default_factory=list)          # {W, H, D}
    coeff_shape: List[int] = field(default_factory=list)    # {W*H*D}
    rle_encoded: List[Tuple[int, float]] = field(default_factory=list)
    need32: bool = False

    @property
    def runs(self) -> np.ndarray:
        return np.array([r for r, _ in self.rle_encoded], np.int32)


def _box_dims(b: np.ndarray) -> Tuple[int, int, int]:
    if b.ndim != 3:
        raise ValueError("Box3D must be a 3-D array of shape (D, H, W)")
    D, H, W = b.shape
    return W, H, D


def serialize_compressed_wavelet(cw: CompressedWavelet) -> bytes:
    """src/compressor.cpp:55-80 (static there; exposed here for tests)."""
    hdr = np.array(list(cw.shape) + list(cw.coeff_shape) + [len(cw.rle_encoded)], "<i4").tobytes()
    if not cw.rle_encoded:
        return hdr
    pairs = np.empty(len(cw.rle_encoded), dtype=[("run", "<i4"), ("val", "<f4")])
    pairs["run"] = [r for r, _ in cw.rle_encoded]
    pairs["val"] = [v for _, v in cw.rle_encoded]
    return hdr + pairs.tobytes()


def deserialize_compressed_wavelet(data: bytes) -> CompressedWavelet:
    """src/decompressor.cpp:35-74: 3 dims, 1 coeff dim, pair count, pairs."""
    if len(data) < 20:
        raise ValueError("serialized wavelet shorter than its 20-byte header")
    h = np.frombuffer(data[:20], "<i4")
    nrle = int(h[4])
    if nrle < 0 or len(data) < 20 + 8 * nrle:
        raise ValueError("serialized wavelet truncated")
    pairs = np.frombuffer(data[20:20 + 8 * nrle], dtype=[("run", "<i4"), ("val", "<f4")])
    cw = CompressedWavelet(shape=[int(h[0]), int(h[1]), int(h[2])], coeff_shape=[int(h[3])],
                           rle_encoded=list(zip(pairs["run"].tolist(), pairs["val"].tolist())),
                           need32=False)
    return cw


def _pairs_need32(vals: np.ndarray) -> bool:
    # need32 = any kept |v| > INT16_MAX (src/compressor.cpp:229); never serialized
    return bool(vals.size and np.any(np.abs(vals.astype(np.float64)) > 32767))


def _laid_out(units_bytes: Sequence[bytes]):
    """The units back to back in one buffer, each at an offset == 4 (mod 8) -> (buffer, offsets)."""
    offsets = np.zeros(max(len(units_bytes), 1), np.uint64)
    cur = 4
    for i, p in enumerate(units_bytes):
        offsets[i] = cur
        cur += (len(p) + 4 + 7) // 8 * 8
    buf = np.zeros(cur + 8, np.uint8)
    for i, p in enumerate(units_bytes):
        o = int(offsets[i])
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return buf, offsets


def _header_dims(units_bytes: Sequence[bytes]) -> list:
    return [tuple(int(v) for v in np.frombuffer(p[:12], "<i4")) for p in units_bytes]


def pack_payloads(payloads: Sequence[bytes], pack: int, device: int = 0) -> List[bytes]:
    """Standard payloads -> packed units with `pack` value bytes (2, 3 or 4; not a
    reference format, include/wavelet_amd.h "Opt-in packed payloads"): one
    wc_pack_host call.  pack = 4 is lossless; 3 and 2 round every kept value to
    its top 3 or 2 bytes (an added error of at most 2^-16 or 2^-8 of the box's
    norm)."""
    if isinstance(pack, bool) or pack not in (2, 3, 4):
        raise ValueError(f"pack: 2, 3 or 4 value bytes, not {pack!r}")
    if not payloads:
        return []
    units, n, _ = capi.make_units(_header_dims(payloads))
    buf, offsets = _laid_out(payloads)
    packed, poff, pbytes = context(device).pack_host(buf, offsets, units, n, int(pack))
    return [packed[int(poff[i]):int(poff[i]) + int(pbytes[i])].tobytes() for i in range(n)]


def unpack_payloads(packed: Sequence[bytes], device: int = 0) -> List[bytes]:
    """Packed units -> standard payloads (values q(v), runs unchanged): one wc_unpack_host call."""
    if not packed:
        return []
    units, n, _ = capi.make_units(_header_dims(packed))
    buf, offsets = _laid_out(packed)
    payload, poff, kept = context(device).unpack_host(buf, offsets, units, n)
    return [capi.unit_payload(payload, poff, kept, i) for i in range(n)]


def _standard_payloads(payloads: Sequence[bytes], device: int = 0) -> List[bytes]:
    """The list with its packed units (capi.payload_packed) unpacked; a list without any is returned as it is."""
    which = _packed_indices(payloads)
    if not which:
        return list(payloads)
    out = list(payloads)
    for i, p in zip(which, unpack_payloads([payloads[i] for i in which], device)):
        out[i] = p
    return out


def _selection(dims, n, max_bytes, ratio, thresh, rmse=None):
    """thin_payloads' and split_payloads' arguments -> (pair budgets or None, n x WC_MAX_LEVELS thresholds or None,
    n tolerances or None)."""
    if sum(v is not None for v in (max_bytes, ratio, thresh, rmse)) != 1:
        raise ValueError("exactly one of max_bytes, ratio, thresh and rmse")
    if n == 0:
        return None, None, None
    pairs = th = None
    if rmse is not None:
        tol = np.full(n, float(rmse), np.float64) if np.ndim(rmse) == 0 else np.asarray(rmse, np.float64)
        if tol.shape != (n,):
            raise ValueError(f"rmse: one value or {n} values")
        if not (tol >= 0).all():
            raise ValueError("rmse: tolerances >= 0 (NaN is none)")
        return None, None, tol
    if thresh is not None:
        th = np.zeros((n, capi.WC_MAX_LEVELS), np.float32)
        if np.ndim(thresh) == 0:
            th[:] = np.float32(thresh)
        else:
            if len(thresh) != n:
                raise ValueError(f"thresh: one value or {n} rows")
            for i, row in enumerate(thresh):
                row = np.atleast_1d(np.asarray(row, np.float32))
                th[i, :min(row.size, capi.WC_MAX_LEVELS)] = row[:capi.WC_MAX_LEVELS]
                th[i, row.size:] = row[-1]
    else:
        if ratio is not None:
            if not float(ratio) > 0:
                raise ValueError(f"ratio: a positive number, not {ratio!r}")
            budget = [max(20, int(4 * W * H * D / float(ratio))) for W, H, D in dims]
        else:
            budget = [int(max_bytes)] * n if np.ndim(max_bytes) == 0 else [int(v) for v in max_bytes]
            if len(budget) != n:
                raise ValueError(f"max_bytes: one value or {n} values")
            if any(v < 20 for v in budget):
                raise ValueError("max_bytes: a payload's header alone takes 20 bytes")
        pairs = [min((v - 20) // 8, 0xFFFFFFFF) for v in budget]
    return pairs, th, None


def thin_payloads(payloads: Sequence[bytes], max_bytes=None, ratio=None, thresh=None, device: int = 0,
                  rmse=None) -> List[bytes]:
    """Payloads -> smaller payloads in the compressed domain (not in the reference;
    wc_thin_budget_host / wc_thin_thresh_host): no cell and no dense coefficient
    exists in between, and the result is what the forward's selection gives on the
    array the payload decodes to.  max_bytes (an int or one per payload) and ratio
    map to a pair budget exactly as in compress_payloads: each result keeps its
    (max_bytes - 20) // 8 largest weighted coefficients and never more (ties at the
    boundary are all dropped); ratio: max_bytes = max(20, floor(4 * N / ratio)) for
    a box of N cells.  thresh (one float >= 0, or L per payload): keeps |c| > thresh
    on every level (or thresh[i][lvl - 1]).  rmse (one value >= 0, or one per
    payload; wc_thin_tol_host): the RMSE this thinning may add, with one threshold
    per level as compress_payloads(rmse=) picks them; a payload written at rmse0
    and thinned at rmse1 is within sqrt(rmse0^2 + rmse1^2) of the original box, and
    a payload that holds every non-zero coefficient gives the bytes of
    compress_payloads(rmse=).  Boxes with cells need even dimensions.  Exactly one
    of the four.  The levels come from the headers.  Packed units are unpacked
    first; the results are standard payloads."""
    if not payloads:
        _selection([], 0, max_bytes, ratio, thresh, rmse)
        return []
    std = _standard_payloads(payloads, device)
    dims = _header_dims(std)
    units, n, _ = capi.make_units(dims)
    buf, offsets = _laid_out(std)
    pairs, th, tol = _selection(dims, n, max_bytes, ratio, thresh, rmse)
    if tol is not None:
        out, off, kept = context(device).thin_tol_host(buf, offsets, units, n, tol)[:3]
    else:
        out, off, kept = context(device).thin_host(buf, offsets, units, n, None, max_pairs=pairs, thresh=th)[:3]
    return [capi.unit_payload(out, off, kept, i) for i in range(n)]


def split_payloads(payloads: Sequence[bytes], max_bytes=None, ratio=None, thresh=None, device: int = 0, rmse=None):
    """Payloads -> (bases, rests) in the compressed domain (not in the reference;
    wc_split_budget_host / wc_split_thresh_host / wc_split_tol_host).  bases[i] is exactly what
    thin_payloads gives with the same arguments; rests[i] holds every other
    candidate of the payload (its non-zero, non-NaN coefficients), so that
    merge_payloads(bases, rests) is the payload again, byte for byte, for every
    payload an encoder of this project emitted.  Splitting rests[i] again yields the
    next layer.  Packed units are unpacked first; the results are standard payloads."""
    if not payloads:
        _selection([], 0, max_bytes, ratio, thresh, rmse)
        return [], []
    std = _standard_payloads(payloads, device)
    dims = _header_dims(std)
    units, n, _ = capi.make_units(dims)
    buf, offsets = _laid_out(std)
    pairs, th, tol = _selection(dims, n, max_bytes, ratio, thresh, rmse)
    if tol is not None:
        base, boff, kept, rest, roff, rpairs = context(device).split_tol_host(buf, offsets, units, n, tol)[:6]
    else:
        base, boff, kept, rest, roff, rpairs = context(device).split_host(buf, offsets, units, n, None, max_pairs=pairs,
                                                                          thresh=th)[:6]
    return ([capi.unit_payload(base, boff, kept, i) for i in range(n)],
            [capi.unit_payload(rest, roff, rpairs, i) for i in range(n)])


def merge_payloads(a: Sequence[bytes], b: Sequence[bytes], *more: Sequence[bytes], device: int = 0) -> List[bytes]:
    """Layers -> their union in the compressed domain (not in the reference;
    wc_merge_host): result[i] holds every pair of a[i], b[i] and more[j][i].  The
    layers of one unit must not hold a pair at the same position (WaveletError,
    WC_ERR_FORMAT).  Folds pairwise, left to right.  Packed units are unpacked first."""
    out = list(a)
    for nxt in (b,) + more:
        if len(nxt) != len(out):
            raise ValueError("merge_payloads: every argument holds one payload per unit")
        if not out:
            continue
        sa, sb = _standard_payloads(out, device), _standard_payloads(nxt, device)
        dims = _header_dims(sa)
        units, n, _ = capi.make_units(dims)
        ba, oa = _laid_out(sa)
        bb, ob = _laid_out(sb)
        res, off, pairs = context(device).merge_host(ba, oa, bb, ob, units, n, None)
        out = [capi.unit_payload(res, off, pairs, i) for i in range(n)]
    return out


def compress_payloads(boxes: Sequence[np.ndarray], keep: float, device: int = 0, levels: int = 1, rmse=None,
                      max_bytes=None, ratio=None, pack=None, maxerr=None):
    """Batched forward path: list of Box3D -> list of serialized payload bytes.

    One wc_forward_host_units call for the whole list (all units in one launch
    set, each uploaded from its own array: no packing copy on the host, as the
    C++ mirror's compress()).  levels > 1 (not a reference parameter): the
    opt-in multi-level transform, each box with the levels its dimensions admit
    (capi.levels_for); such payloads carry ncoeff = -L in their headers.
    rmse (not a reference parameter; None: the keep rule): the tolerated RMSE of
    every box, one value or one per box, in place of keep, with one threshold
    per level (wc_forward_levels_tol_host); boxes with cells need even
    dimensions.  max_bytes (not a reference parameter; an int or one per box):
    every payload is at most max_bytes long: the box keeps its (max_bytes - 20)
    // 8 largest weighted coefficients (wc_forward_levels_budget_host; ties at
    the boundary are all dropped).  ratio: max_bytes = max(20, floor(4 * N /
    ratio)) per box of N cells.  maxerr (not a reference parameter; one value or
    one per box): no cell of a box's reconstruction is further than maxerr from
    the box's cell, in the box's own dtype (float64 boxes are compared before
    narrowing); the threshold is verified on the device by the round trip
    itself (wc_forward_levels_maxerr_host); boxes with cells need even
    dimensions.  rmse, max_bytes, ratio and maxerr exclude each other.
    The payload format is the same.  pack (not a reference parameter; None, 2,
    3 or 4): applied after any of the above, the payloads are returned as packed
    units with that many value bytes (pack_payloads); max_bytes and ratio keep
    meaning the bytes of the STANDARD payload, not of the packed unit."""
    if pack is not None:
        if isinstance(pack, bool) or pack not in (2, 3, 4):
            raise ValueError(f"pack: None, 2, 3 or 4 value bytes, not {pack!r}")
        return pack_payloads(compress_payloads(boxes, keep, device, levels, rmse, max_bytes, ratio, maxerr=maxerr),
                             pack, device)
    if sum(v is not None for v in (rmse, max_bytes, ratio, maxerr)) > 1:
        raise ValueError("rmse, max_bytes, ratio and maxerr are mutually exclusive")
    dims = [_box_dims(b) for b in boxes]
    budget = None
    if ratio is not None:
        if not float(ratio) > 0:
            raise ValueError(f"ratio: a positive number, not {ratio!r}")
        budget = [max(20, int(4 * W * H * D / float(ratio))) for W, H, D in dims]
    elif max_bytes is not None:
        budget = [int(max_bytes)] * len(dims) if np.ndim(max_bytes) == 0 else [int(v) for v in max_bytes]
        if len(budget) != len(dims):
            raise ValueError(f"max_bytes: one value or {len(dims)} values")
        if any(v < 20 for v in budget):
            raise ValueError("max_bytes: a payload's header alone takes 20 bytes")
    arrs = [np.ascontiguousarray(b, np.float32) for b in boxes]
    if not 1 <= int(levels) <= capi.WC_MAX_LEVELS:
        raise ValueError(f"levels: 1..{capi.WC_MAX_LEVELS}, not {levels!r}")
    if levels > 1 or rmse is not None or budget is not None or maxerr is not None:
        units, n, extent = capi.make_units(dims)
        if maxerr is not None and any(np.asarray(b).dtype == np.float64 for b in boxes):
            arrs = [np.ascontiguousarray(b, np.float64) for b in boxes]  # the bound holds against these cells
        cells = np.zeros(max(extent, 1), arrs[0].dtype if arrs else np.float32)
        for i, a in enumerate(arrs):
            cells[units[i].cell_offset:units[i].cell_offset + a.size] = a.ravel()
        lv = [capi.levels_for(*d, levels) for d in dims]
        if maxerr is not None:
            payload, offsets, kept = context(device).forward_levels_maxerr_host(cells, units, n, lv, maxerr,
                                                                                want_rmse=False)[:3]
        elif budget is not None:
            pairs = [min((v - 20) // 8, 0xFFFFFFFF) for v in budget]
            payload, offsets, kept = context(device).forward_levels_budget_host(cells, units, n, lv, pairs,
                                                                                want_rmse=False)[:3]
        elif rmse is not None:
            payload, offsets, kept = context(device).forward_levels_tol_host(cells, units, n, lv, rmse, want_rmse=False)[:3]
        else:
            payload, offsets, kept = context(device).forward_levels_host(cells, units, n, lv, keep)
        return [capi.unit_payload(payload, offsets, kept, i) for i in range(n)]
    units, n, _ = capi.make_units(dims)
    payload, offsets, kept = context(device).forward_host_units(arrs, units, n, keep)
    return [capi.unit_payload(payload, offsets, kept, i) for i in range(n)]


def compress(box: Sequence[np.ndarray], components: Sequence[int], keep: float, time: int,
             level: int, box_index: int, compressed_dir, levels: int = 1, pack=None) -> List[CompressedWavelet]:
    """src/compressor.cpp:192-297.  box[c] is positional; components[c] (an
    AMReX header index) only names the output file.  Writes one .xz file per
    component and returns the CompressedWavelet structs.  levels (not a
    reference parameter, default 1 = the reference's codec): see
    compress_payloads; decompress() reads the levels from each file's header.
    pack (not a reference parameter; None, 2, 3 or 4): the files hold packed
    units (pack_payloads) through the same xz call and under the same names;
    decompress() recognises them.  The returned structs describe the payloads
    before packing."""
    comps = list(components)
    boxes = [box[c] for c in range(len(comps))]
    payloads = compress_payloads(boxes, keep, levels=levels)
    written = payloads if pack is None else pack_payloads(payloads, pack)
    out = []
    for c, p in enumerate(payloads):
        cw = deserialize_compressed_wavelet(p)
        cw.need32 = _pairs_need32(np.array([v for _, v in cw.rle_encoded], np.float32))
        fname = Path(compressed_dir) / f"compressed-wavelet-{time}-{level}-{comps[c]}-{box_index}.xz"
        try:
            f = open(fname, "wb")
        except OSError:
            f = None  # a failed ofstream open silently skips the file (src/compressor.cpp:256-257)
        if f is not None:
            with f:
                f.write(lzma.compress(written[c], format=lzma.FORMAT_XZ, check=XZ_CHECK, preset=xz_preset()))
        out.append(cw)
    return out


def read_compressed_payload(file_path) -> bytes:
    """xz read of src/decompressor.cpp:164-220 (errors exit, as the reference does)."""
    try:
        raw = Path(file_path).read_bytes()
    except OSError as e:
        print(f"[error] Failed to open file: {file_path} ({e})", file=sys.stderr)
        sys.exit(1)
    try:
        return lzma.decompress(raw, format=lzma.FORMAT_XZ)
    except lzma.LZMAError as e:
        print(f"[error] LZMA decompression failed: {e}", file=sys.stderr)
        sys.exit(1)


def _coarse_dims(payloads: Sequence[bytes], dims, coarsen) -> list:
    """The boxes' dims >> coarsen, after the checks that need no device: coarsen
    in 0..WC_MAX_LEVELS, no more than each payload's levels, 2^coarsen dividing
    the dims of every box with cells (ValueError naming the payload's index)."""
    if isinstance(coarsen, bool) or not isinstance(coarsen, (int, np.integer)) or not 0 <= coarsen <= capi.WC_MAX_LEVELS:
        raise ValueError(f"coarsen: an integer 0..{capi.WC_MAX_LEVELS}, not {coarsen!r}")
    r = int(coarsen)
    for i, (p, (W, H, D)) in enumerate(zip(payloads, dims)):
        nc = int(np.frombuffer(p[12:16], "<i4")[0])
        L = 1 if nc >= 0 else -nc
        if r > L:
            raise ValueError(f"payload {i}: coarsen={r} exceeds its {L} transform level(s)")
        if W * H * D and r and (W | H | D) & ((1 << r) - 1):
            raise ValueError(f"payload {i} ({W}x{H}x{D}): coarsen={r} needs W, H and D divisible by {1 << r}")
    return [(W >> r, H >> r, D >> r) for W, H, D in dims]


def _aligned_regions(payloads: Sequence[bytes], dims, region) -> tuple:
    """region = ((x0, y0, z0), (x1, y1, z1)), hi exclusive, in cells of the full
    boxes -> (lo, hi, each payload's region rounded outward to its 2^L as
    (x0, y0, z0, nx, ny, nz)), after the checks that need no device: a non-empty
    region inside every box, 2^L dividing every box's dims (ValueError)."""
    try:
        lo, hi = (tuple(int(v) for v in region[0]), tuple(int(v) for v in region[1]))
        ok = len(region) == 2 and len(lo) == 3 and len(hi) == 3
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok:
        raise ValueError(f"region: ((x0, y0, z0), (x1, y1, z1)), not {region!r}")
    if any(b <= a for a, b in zip(lo, hi)):
        raise ValueError(f"region {lo}..{hi} is empty")
    out = []
    for i, (p, (W, H, D)) in enumerate(zip(payloads, dims)):
        if any(a < 0 for a in lo) or hi[0] > W or hi[1] > H or hi[2] > D:
            raise ValueError(f"payload {i} ({W}x{H}x{D}): region {lo}..{hi} is not inside the box")
        nc = int(np.frombuffer(p[12:16], "<i4")[0])
        L = 1 if nc >= 0 else -nc
        if not 1 <= L <= capi.WC_MAX_LEVELS:
            raise ValueError(f"payload {i}: not a payload header")
        if (W | H | D) & ((1 << L) - 1):
            raise ValueError(f"payload {i} ({W}x{H}x{D}): a region decode of {L} level(s) needs W, H and D "
                             f"divisible by {1 << L}")
        out.append(capi.region_align((W, H, D), L, lo + tuple(b - a for a, b in zip(lo, hi))))
    return lo, hi, out


def decompress_payloads(payloads: Sequence[bytes], device: int = 0, coarsen: int = 0, region=None) -> List[np.ndarray]:
    """Batched inverse path: serialized payloads -> Box3D arrays (one wc_inverse_host
    call; wc_inverse_levels_host, which reads each payload's levels from its
    header, when some payload is a multi-level one: ncoeff < 0).

    coarsen = r > 0 (not a reference parameter): every box at 1/2^r resolution,
    shape (D >> r, H >> r, W >> r), each cell the mean of a 2^r-cube of the full
    box up to fp32 rounding, decoded from the low-pass corner of its
    coefficients alone (wc_inverse_coarse_host).  Works on reference-format
    payloads (one level) with r = 1 and even dims.

    region = ((x0, y0, z0), (x1, y1, z1)) (not a reference parameter): only the
    cells [lo, hi) of every box, shape (z1 - z0, y1 - y0, x1 - x0); with coarsen
    = r the cells [lo >> r, ceil(hi / 2^r)) of the coarse box.  Any region
    inside the box: it is rounded outward to multiples of 2^L (L the payload's
    levels, which must divide the box's dims), decoded from the coefficients it
    depends on alone (wc_inverse_region_host) and cropped here.  The bits are
    those of the crop of the full decode.

    Packed units (compress_payloads(pack=)) are recognised by their headers.  The
    full and the coarsen= decode read them directly from their packed bytes
    (wc_inverse_packed_host, wc_inverse_packed_coarse_host): no standard payload
    is rebuilt, and the bits are those of unpack_payloads followed by the
    standard call.  A list that mixes packed and standard payloads makes two
    calls, one per kind, and the boxes come back in list order.  With region=
    the packed units are unpacked first (wc_unpack_host): the direct region call
    measured slower than unpack + decode on the device (DESIGN.md "Packed
    decode"); capi's inverse_packed_region_host is there for a caller who wants
    the smaller footprint."""
    if region is not None:
        payloads = _standard_payloads(payloads, device)
    payloads = list(payloads)
    which = _packed_indices(payloads)
    if which and len(which) < len(payloads):
        rest = [i for i in range(len(payloads)) if i not in set(which)]
        out = [None] * len(payloads)
        for idx, packed in ((which, True), (rest, False)):
            for i, box in zip(idx, _decompress_group([payloads[i] for i in idx], device, coarsen, region, packed)):
                out[i] = box
        return out
    return _decompress_group(payloads, device, coarsen, region, bool(which))


def _packed_indices(payloads: Sequence[bytes]) -> list:
    """The indices of the list's packed units (capi.payload_packed)."""
    return [i for i, p in enumerate(payloads) if len(p) >= 20 and int(np.frombuffer(p[12:16], "<i4")[0]) < -capi.WC_MAX_LEVELS
            and capi.payload_packed(p)[1]]


def _decompress_group(payloads: Sequence[bytes], device: int, coarsen: int, region, packed: bool) -> List[np.ndarray]:
    """decompress_payloads on payloads of one kind: standard ones, or packed units (packed)."""
    dims = []
    multi = False
    heads = []  # what the checks below read of a payload: its header with the standard ncoeff field
    for p in payloads:
        h = np.frombuffer(p[:20], "<i4").copy()
        dims.append((int(h[0]), int(h[1]), int(h[2])))
        if packed:
            L = capi.payload_packed(p)[0]
            h[3] = -L if L >= 2 else int(h[0]) * int(h[1]) * int(h[2])
        heads.append(h.tobytes())
        multi |= int(h[3]) < 0
    cdims = _coarse_dims(heads, dims, coarsen)
    if region is not None:
        lo, hi, regions = _aligned_regions(heads, dims, region)
    units, n, extent = capi.make_units(dims)
    buf, offsets = _laid_out(payloads)
    ctx = context(device)
    if region is not None:
        r = int(coarsen)
        out_units, extent = capi.region_units(units, n, regions, r)
        assert not packed  # decompress_payloads unpacks first for a region
        flat = ctx.inverse_region_host(buf, offsets, units, n, r, regions, out_units, extent)
        up = (1 << r) - 1
        out = []
        for i, g in enumerate(regions):
            w, h, d = g[3] >> r, g[4] >> r, g[5] >> r
            o = out_units[i].cell_offset
            a = [(lo[k] >> r) - (g[k] >> r) for k in range(3)]
            m = [((hi[k] + up) >> r) - (lo[k] >> r) for k in range(3)]
            box = flat[o:o + w * h * d].reshape(d, h, w)
            out.append(box[a[2]:a[2] + m[2], a[1]:a[1] + m[1], a[0]:a[0] + m[0]].copy())
        return out
    if coarsen:
        out_units, extent = capi.coarse_units(units, n, int(coarsen))
        call = ctx.inverse_packed_coarse_host if packed else ctx.inverse_coarse_host
        flat = call(buf, offsets, units, n, int(coarsen), out_units, extent)
        units, dims = out_units, cdims
    elif packed:
        flat = ctx.inverse_packed_host(buf, offsets, units, n, extent)
    elif multi:
        flat = ctx.inverse_levels_host(buf, offsets, units, n, extent)
    else:
        flat = ctx.inverse_host(buf, offsets, units, n, extent)
    out = []
    for i, (W, H, D) in enumerate(dims):
        o = units[i].cell_offset
        out.append(flat[o:o + W * H * D].reshape(D, H, W).copy())
    return out


def decompress(file_path, time: int = 0, level: int = 0, component: int = 0, box_idx: int = 0,
               coarsen: int = 0, region=None) -> np.ndarray:
    """src/decompressor.cpp:238-255 (only file_path is used, as in the reference).
    coarsen, region (not reference parameters): see decompress_payloads."""
    return decompress_payloads([read_compressed_payload(file_path)], coarsen=coarsen, region=region)[0]


def inverse_wavelet_decompose(flat, x: int, y: int, z: int) -> np.ndarray:
    """src/decompressor.cpp:79-159 on the GPU: flat coefficients -> Box3D (z, y, x)."""
    f = np.ascontiguousarray(flat, np.float32)
    if f.size != x * y * z:
        raise ValueError("flat length != x*y*z")
    units, n, extent = capi.make_units([(x, y, z)])
    return context(0).inverse_flat_host(f, units, n, extent).reshape(z, y, x)


def wavelet_decompose(box: np.ndarray) -> np.ndarray:
    """src/compressor.cpp:85-185 (static there) on the GPU: Box3D -> flat coefficients."""
    W, H, D = _box_dims(box)
    units, n, extent = capi.make_units([(W, H, D)])
    return context(0).decompose_host(np.ascontiguousarray(box, np.float32).ravel(), units, n, extent)


def calc_rmse_per_box(actual: Sequence[np.ndarray], pred: Sequence[np.ndarray],
                      num_components: int) -> List[float]:
    """src/calc-loss.cpp:12-43 on the GPU (one K7 launch for all components).
    Like the reference, every component uses actual[0]'s dimensions."""
    W, H, D = _box_dims(actual[0])
    units, n, extent = capi.make_units([(W, H, D)] * num_components)
    a = np.zeros(max(extent, 1), np.float32)
    p = np.zeros(max(extent, 1), np.float32)
    for c in range(num_components):
        o = units[c].cell_offset
        a[o:o + W * H * D] = np.ascontiguousarray(actual[c], np.float32).ravel()
        p[o:o + W * H * D] = np.ascontiguousarray(pred[c], np.float32).ravel()
    return context(0).rmse_host(a, p, units, n).tolist()


def calc_adj_loss(rmse: float, value_range: float) -> float:
    """src/calc-loss.cpp:49-51."""
    return rmse / value_range


def calc_size(path) -> float:
    """src/calc-loss.cpp:55-65: total bytes of the files under path."""
    total = 0.0
    for root, _dirs, files in os.walk(path):
        for f in files:
            total += os.path.getsize(os.path.join(root, f))
    return total
