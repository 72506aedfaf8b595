"""Seeded random batches for the opt-in modes (the multi-level transform, the
reduced-resolution decode, the RMSE-tolerance mode).  TEST INFRASTRUCTURE ONLY:
shared by tests/test_modes_batches_cpu.py, which proves on the restatements
alone that every batch holds what it claims, and tests/test_gpu_modes_fuzz.py,
which runs the batches through the device and host entry points.  The fields
are test_gpu_fuzz._field's: the smooth SURVEY field, wide-range Gaussians,
constants of either sign, zeros, subnormals, NaN / +-inf / +-0 sprinkled in.

Boxes are the oracle's numpy [D, H, W] (x fastest), float64; a test narrows
them as the codec does (oracle.narrow for fp64 cells, astype for fp32)."""
import numpy as np

import levels_ref as R
from test_gpu_fuzz import _field

KEEPS = (0.999, 0.0, 1.0, 1.5)  # beside one uniform draw: the fuzz's set
LV_BLOCKS = 4096                # 2x2x2 blocks of a level's sub-box per workgroup (wc_levels.hip kLvBlocks)
MS, ES = (1, 2, 3, 5, 6, 7, 9, 12), 6
UNIT_CELLS, BATCH_CELLS = 1 << 19, 3 << 20

# (tag, dims, L): the first units of every levels batch, with that seed's random fields
PINNED = [
    ("l4_cube", (16, 16, 16), 4),          # the last level is one 2x2x2 block
    ("l4_unequal", (48, 16, 80), 4),       # unequal axes; odd hd = 5 at level 4
    ("odd_hd_3072", (128, 128, 12), 2),    # level 2: 64 x 64 x 6, hd = 3, 3072 blocks in the scalar branch
    ("odd_hd_l3", (128, 128, 24), 3),      # level 3: 32 x 32 x 6, hd = 3, after an even-hd level 2
    ("odd_hd_5120", (128, 128, 20), 2),    # level 2: 64 x 64 x 10, hd = 5, 5120 blocks: two chunks, scalar branch
    ("float2_copy", (64, 128, 36), 2),     # level 2: 32 x 64 x 18, d % 4 == 2, 4608 blocks: two chunks of 8-B copies
    ("l3_cube", (64, 64, 64), 3),          # fast transform tiles, 64 flat tiles
]
# the special units that follow them: (tag, dims, L)
SPECIALS = [("nan_first", (8, 8, 8), 2), ("inf_pair", (8, 8, 8), 2), ("minus_inf", (8, 8, 8), 2)]
SPECIAL_TAGS = tuple(t for t, _, _ in SPECIALS)


def narrow(O, box, dtype):
    """The fp32 box the codec sees for cells of `dtype`."""
    return O.narrow(box) if dtype == np.float64 else np.asarray(box).astype(np.float32)


def special_box(tag, dims, rng):
    """Gaussian cells (|x| of order 1) with the special the tag names.
    nan_first: a NaN in cell (0, 0, 0), which every level's low-pass carries to A[0].
    inf_pair: +inf in cell (4, 4, 4) and -inf in cell (6, 4, 4): two level-1 blocks
    (no NaN after one level), one 2x2x2 block of the level-2 sub-box (inf - inf there,
    off the origin: A[0] stays finite at L = 2).
    inf_block: both in the level-1 block of cells (4..5, 4..5, 4..5): NaN from the first transform on.
    plus_inf / minus_inf: that one value in a cell off the origin.
    neg_const: a constant negative box (the signed maximum is negative)."""
    W, H, D = dims
    b = rng.standard_normal((D, H, W))
    if tag == "nan_first":
        b[0, 0, 0] = np.nan
    elif tag == "inf_pair":
        b[4, 4, 4], b[4, 4, 6] = np.inf, -np.inf
    elif tag == "inf_block":
        b[4, 4, 4], b[5, 5, 5] = np.inf, -np.inf
    elif tag == "plus_inf":
        b[D // 2 + 1, 1, W - 1] = np.inf
    elif tag == "minus_inf":
        b[D // 2 + 1, 1, W - 1] = -np.inf
    elif tag == "neg_const":
        b[...] = -3.0
    else:
        raise ValueError(tag)
    return b


class LevelsBatch:
    """dims, levels, boxes (float64 [D, H, W]), offsets (cell offsets), extent,
    dtype, keep (a float32 value), tags {name: unit index} of the pinned units."""


def _axis(rng, e0):
    while True:
        v = int(rng.choice(MS)) << int(min(ES - 1, e0 + rng.integers(0, 3)))
        if v <= 128:
            return v


def levels_batch(O, seed):
    rng = np.random.default_rng(7000 + seed)
    B = LevelsBatch()
    B.seed, B.dtype = seed, (np.float64 if seed % 2 == 0 else np.float32)
    n = int(rng.integers(20, 51))
    spec = [(t, d, L) for t, d, L in PINNED + SPECIALS]
    cells = sum(d[0] * d[1] * d[2] for _, d, _ in spec)
    empties = set(int(x) for x in rng.choice(np.arange(len(spec), n), size=int(rng.integers(1, 3)), replace=False))
    while len(spec) < n:
        if len(spec) in empties:
            d = [int(rng.choice(MS)) * 2 for _ in range(3)]
            d[int(rng.integers(0, 3))] = 0
            spec.append((None, tuple(d), 1))
            continue
        if rng.random() < 0.125:  # L = 1 with odd dims
            d = tuple(int(x) for x in rng.choice([1, 3, 5, 7, 9], size=3))
        else:
            e0 = int(rng.integers(0, 5))
            d = tuple(_axis(rng, e0) for _ in range(3))
        c = d[0] * d[1] * d[2]
        room = BATCH_CELLS - cells - 64 * (n - len(spec))  # every later unit can still be a 4^3
        if c > UNIT_CELLS or c > room:
            d = tuple(max(1, x >> 2) if x % 4 == 0 else x for x in d)  # the same 2-adic mix, 1/64 of the cells
            c = d[0] * d[1] * d[2]
            if c > UNIT_CELLS or c > room:
                d, c = (4, 4, 4), 64
        cells += c
        spec.append((None, d, int(rng.integers(1, R.levels_for(*d, R.MAX_LEVELS) + 1))))
    B.dims, B.levels, B.boxes, B.offsets, B.tags = [], [], [], [], {}
    cur = 0
    for i, (tag, d, L) in enumerate(spec):
        W, H, D = d
        if tag in SPECIAL_TAGS:
            b = special_box(tag, d, rng)
        else:
            b = _field(rng, O, i, d)
        if tag:
            B.tags[tag] = i
        cur += int(rng.integers(0, 9))  # random gaps, every third unit at an odd element offset
        if i % 3 == 0 and cur % 2 == 0:
            cur += 1
        B.dims.append(d)
        B.levels.append(L)
        B.boxes.append(b)
        B.offsets.append(cur)
        cur += W * H * D
    B.extent = cur
    B.n = n
    B.keep = float(np.float32(rng.choice([rng.uniform(0.5, 0.99999), *KEEPS])))
    return B


def level_blocks(dims, l):
    """(hw, hh, hd) of level l's sub-box, l >= 2: its 2x2x2 blocks per axis."""
    return tuple(x >> l for x in dims)


def coarse_cases(O, B, rng):
    """-> (payloads, reduce, odd_at, surplus_at) of one wc_inverse_coarse batch on
    the levels batch B: every unit's payload at its levels (the keep rule with a
    keep of the fuzz's set per unit) and a random r in 0..L (0 for a unit
    without cells); then one-level oracle payloads of B's even boxes at r = 1
    and the 16^3 L4 payload at every r;
    three units keep every coefficient and carry five surplus pairs past ncoeff
    (test_gpu_coarse.surplus); odd_at: the unit whose output offset is odd."""
    from test_gpu_coarse import surplus
    pays, reduce = [], []
    finite = [i for i, b in enumerate(B.boxes) if b.size >= 64 and np.isfinite(b).all()]
    surplus_at = sorted(int(x) for x in rng.choice(finite, size=3, replace=False))
    for i, (b, L) in enumerate(zip(B.boxes, B.levels)):
        b32 = narrow(O, b, B.dtype)
        if i in surplus_at:
            p = surplus(O, R.payload(b32, L, thresh=-1.0)[0])  # |c| > -1: everything finite
        else:
            p = R.payload(b32, L, keep=float(np.float32(rng.choice([rng.uniform(0.5, 0.99999), *KEEPS]))))[0]
        pays.append(p)
        odd = (B.dims[i][0] | B.dims[i][1] | B.dims[i][2]) & 1  # L = 1 alone admits odd dims: r = 0 then
        reduce.append(int(rng.integers(0, L + 1)) if b.size and not odd else 0)
    even = [i for i, d in enumerate(B.dims) if d[0] * d[1] * d[2] and not (d[0] | d[1] | d[2]) & 1]
    for i in rng.choice(even, size=min(4, len(even)), replace=False):
        pays.append(O.compress_payload(narrow(O, B.boxes[int(i)], B.dtype), float(np.float32(0.999)))[0])
        reduce.append(1)
    for r in range(B.levels[B.tags["l4_cube"]] + 1):  # one four-level payload at every r
        pays.append(pays[B.tags["l4_cube"]])
        reduce.append(r)
    with_cells = [i for i, p in enumerate(pays) if int(np.prod(np.frombuffer(p[:12], "<i4"))) > 0]
    return pays, reduce, int(rng.choice(with_cells)), surplus_at


TOL_SIZES = (2, 4, 6, 8, 10, 12, 16, 24, 32, 40, 48, 64)
TOL_BATCH_CELLS = 1 << 21
TOL_WIDE = (2, (32, 16, 12))  # (unit, dims) of the pinned wide-range unit: Gaussian cells times 10^30


class TolBatch:
    """dims, boxes (float64 [D, H, W]), offsets, extent, dtype, tol (n doubles)."""


def tol_batch(O, seed):
    rng = np.random.default_rng(8000 + seed)
    B = TolBatch()
    B.seed, B.dtype = seed, (np.float64 if seed % 2 == 0 else np.float32)
    n = int(rng.integers(20, 61))
    # 64 flat tiles on the fast path; 12 tiles on the generic one (D % 8 != 0); a wide-range unit
    dims = [(64, 64, 64), (64, 64, 12), TOL_WIDE[1]]
    cells = sum(d[0] * d[1] * d[2] for d in dims)
    while len(dims) < n:
        d = tuple(int(x) for x in rng.choice(TOL_SIZES, size=3))
        if cells + d[0] * d[1] * d[2] > TOL_BATCH_CELLS:
            d = tuple(max(2, x // 4 * 2) for x in d)
        cells += d[0] * d[1] * d[2]
        dims.append(d)
    B.dims, B.n = dims, n
    B.boxes = [_field(rng, O, i, d) for i, d in enumerate(dims)]
    W, H, D = TOL_WIDE[1]
    B.boxes[TOL_WIDE[0]] = rng.standard_normal((D, H, W)) * 1e30  # bin sums of 8 c^2 reach 10^60 and beyond
    B.offsets, cur = [], 0
    for i, (W, H, D) in enumerate(dims):
        cur += int(rng.integers(0, 9))
        if i % 3 == 0 and cur % 2 == 0:
            cur += 1
        B.offsets.append(cur)
        cur += W * H * D
    B.extent = cur
    B.tol = []
    for b in B.boxes:
        f = narrow(O, b, B.dtype).astype(np.float64)
        f = f[np.isfinite(f)]
        rms = float(np.sqrt(np.mean(f * f))) if f.size else 0.0
        k = int(rng.integers(0, 6))
        B.tol.append(0.0 if k == 0 else np.inf if k == 1 else 10.0 ** rng.uniform(-6, 3) * rms)
    B.tol[TOL_WIDE[0]] = float(np.sqrt(np.mean(B.boxes[TOL_WIDE[0]] ** 2)))  # its RMS: the rule's S is about 10^60 N
    return B
