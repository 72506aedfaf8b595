"""Units with one long axis: pencils, slabs and lines of up to 4097 cells along
x, y or z, at the sizes where the plan (wavelet-compression_amd/csrc/wc_plan.cpp)
changes the kernel or the tile shape of a unit.  TEST INFRASTRUCTURE ONLY:
shared by tests/test_long_axis_cpu.py (which derives CLASSES again from the dims
and proves that the list holds what it claims), tests/test_gpu_long_axis.py
(which runs the list through every device and host entry point) and, for the
fast-shape units of at most PLAN_CELLS cells, tests/cpp/test_plan.cpp (same
dims, same cell offsets; the CPU test compares the two lists).

Boxes are the oracle's numpy [D, H, W] (x fastest), float64; a test narrows them
as the codec does (modes_batches.narrow)."""
import numpy as np

from test_gpu_fuzz import _field

# (tag, (W, H, D)).  The order matters: every third unit sits at an odd cell
# offset (layout), field (b) gives unit i the kind i % 8 (fuzz_box).
UNITS = [
    ("big_x", (2048, 32, 32)),        # exactly 2^21 cells: 16384-coefficient emit tiles; long x, 512 flat rows start in each
    ("big_y", (32, 2048, 32)),        # ... long y
    ("big_z", (32, 32, 2048)),        # ... long z: 32 z tiles, 8 flat rows per emit tile
    ("below_big", (2046, 32, 32)),    # 2^21 - 2048 cells: small emit tiles; W % 4 == 2
    ("s32_x", (2048, 2, 64)),         # the transform's 32 x 1 x 32 form with one block row ...
    ("s32_z", (64, 2, 2048)),         # ... long z: the row-indexed tile shrinks to one block column
    ("pencil_x", (4096, 2, 8)),        # D = 8: 1024 flat rows start inside each emit tile
    ("s32_y", (64, 34, 64)),          # ... and with 17 y tiles
    ("pencil_y", (2, 4096, 8)),
    ("pencil_z", (2, 2, 4096)),       # sparse staging with lbx = lby = 0; dense decode at either budget
    ("rix_edge_in", (2, 2, 2280)),    # 4 D + 80 = 9200 <= 9216: row-indexed at the default budget
    ("rix_edge_out", (2, 2, 2288)),   # 4 D + 80 = 9232: decodes densely
    ("rix_edge_wide", (4, 6, 2280)),  # the boundary unit with 6 one-block tiles
    ("magic_d_x", (130, 2, 1000)),    # D no power of two: the multiply form of the row division
    ("magic_d_y", (2, 130, 1000)),    # ... H = 130: the coarse corner filter's division by H
    ("magic_d_3000", (8, 8, 3000)),
    ("magic_d_200", (66, 2, 200)),
    ("lx_shrink_264", (256, 2, 264)),      # the row-indexed tile's x blocks drop from 16 to 8
    ("lx_shrink_hx513", (1026, 4, 40)),    # hx 513: an edge tile of one block column
    ("lx_shrink_hy513", (4, 1026, 24)),    # hy 513: an edge tile of one block row
    ("lx_shrink_160", (192, 6, 160)),      # D = 160: dense staging beside sparse neighbours
    ("slab_x", (320, 64, 8)),         # D = 8: two z blocks per tile, y takes the rest
    ("slab_y", (64, 320, 8)),
    ("odd_x", (2049, 3, 5)),          # generic transform, 33 x tiles, the last one the pass-through tail alone
    ("odd_y", (3, 2049, 5)),
    ("odd_z", (3, 5, 2049)),
    ("line_x", (4097, 1, 1)),         # degenerate axes
    ("line_y", (1, 4097, 1)),
    ("line_z", (1, 1, 4097)),
    ("empty", (0, 2048, 8)),          # no cells between long neighbours
    ("s32_x_odd", (2048, 2, 64)),     # the S32 shapes again at odd cell offsets: the general fast form
    ("s32_z_odd", (64, 2, 2048)),
    ("s32_y_odd", (64, 34, 64)),
]
# appended for the WC_OPT_RIX_LDS 16384 leg alone: 4 D + 80 = 16368 and 16400
RIX16K = [("rix16k_in", (2, 2, 4072)), ("rix16k_out", (2, 2, 4080))]
S32_TAGS = ("s32_x", "s32_z", "s32_y")
PLAN_CELLS = 300_000  # tests/cpp/test_plan.cpp takes the fast-shape units up to this size
MAX_CELLS = 16 << 20

# What the plan makes of each tag, as plain data (tests/test_long_axis_cpu.py
# derives it again from the dims; tests/cpp/test_plan.cpp checks the plan against it):
# fast: even W and H, D % 8 == 0, cells; sparse: sparse staging; lb: log2 of the transform
# tile in blocks (lbx, lby, lbz); big: the 16384-coefficient emit tile; net: emit tiles;
# ntx: transform tiles; rix9216 / rix16384: (ilbx, ilby) of the row-indexed inverse's tile at
# that WC_OPT_RIX_LDS and the default WC_OPT_RIX_TX 4, None where the unit decodes densely.
CLASSES = {
    "big_x": dict(fast=True, sparse=True, lb=(5, 1, 4), big=True, net=128, ntx=256, rix9216=(4, 2), rix16384=(4, 2)),
    "big_y": dict(fast=True, sparse=True, lb=(4, 2, 4), big=True, net=128, ntx=256, rix9216=(4, 2), rix16384=(4, 2)),
    "big_z": dict(fast=True, sparse=True, lb=(4, 1, 5), big=True, net=128, ntx=256, rix9216=(0, 0), rix16384=(0, 0)),
    "below_big": dict(fast=True, sparse=True, lb=(5, 1, 4), big=False, net=256, ntx=256, rix9216=(4, 2), rix16384=(4, 2)),
    "s32_x": dict(fast=True, sparse=True, lb=(5, 0, 5), big=False, net=32, ntx=32, rix9216=(4, 0), rix16384=(4, 0)),
    "s32_z": dict(fast=True, sparse=True, lb=(5, 0, 5), big=False, net=32, ntx=32, rix9216=(0, 0), rix16384=(0, 0)),
    "s32_y": dict(fast=True, sparse=True, lb=(5, 0, 5), big=False, net=17, ntx=17, rix9216=(4, 1), rix16384=(4, 1)),
    "pencil_x": dict(fast=True, sparse=False, lb=(5, 0, 2), big=False, net=8, ntx=64, rix9216=(4, 0), rix16384=(4, 0)),
    "pencil_y": dict(fast=True, sparse=False, lb=(0, 8, 2), big=False, net=8, ntx=8, rix9216=(0, 8), rix16384=(0, 8)),
    "pencil_z": dict(fast=True, sparse=True, lb=(0, 0, 5), big=False, net=2, ntx=64, rix9216=None, rix16384=None),
    "rix_edge_in": dict(fast=True, sparse=False, lb=(0, 0, 5), big=False, net=2, ntx=36, rix9216=(0, 0), rix16384=(0, 0)),
    "rix_edge_out": dict(fast=True, sparse=False, lb=(0, 0, 5), big=False, net=2, ntx=36, rix9216=None, rix16384=(0, 0)),
    "rix_edge_wide": dict(fast=True, sparse=False, lb=(1, 2, 5), big=False, net=7, ntx=36, rix9216=(0, 0), rix16384=(0, 0)),
    "magic_d_x": dict(fast=True, sparse=False, lb=(5, 0, 5), big=False, net=32, ntx=48, rix9216=(1, 0), rix16384=(2, 0)),
    "magic_d_y": dict(fast=True, sparse=False, lb=(0, 5, 5), big=False, net=32, ntx=48, rix9216=(0, 1), rix16384=(0, 2)),
    "magic_d_3000": dict(fast=True, sparse=False, lb=(2, 2, 5), big=False, net=24, ntx=47, rix9216=None, rix16384=(0, 0)),
    "magic_d_200": dict(fast=True, sparse=False, lb=(5, 0, 5), big=False, net=4, ntx=8, rix9216=(3, 0), rix16384=(4, 0)),
    "lx_shrink_264": dict(fast=True, sparse=False, lb=(5, 0, 5), big=False, net=17, ntx=20, rix9216=(3, 0), rix16384=(3, 0)),
    "lx_shrink_hx513": dict(fast=True, sparse=False, lb=(5, 0, 5), big=False, net=21, ntx=34, rix9216=(4, 1), rix16384=(4, 1)),
    "lx_shrink_hy513": dict(fast=True, sparse=False, lb=(1, 5, 4), big=False, net=13, ntx=17, rix9216=(1, 5), rix16384=(1, 6)),
    "lx_shrink_160": dict(fast=True, sparse=False, lb=(5, 0, 5), big=False, net=23, ntx=27, rix9216=(3, 0), rix16384=(4, 0)),
    "slab_x": dict(fast=True, sparse=False, lb=(5, 3, 2), big=False, net=20, ntx=20, rix9216=(4, 4), rix16384=(4, 4)),
    "slab_y": dict(fast=True, sparse=False, lb=(5, 3, 2), big=False, net=20, ntx=20, rix9216=(4, 4), rix16384=(4, 4)),
    "odd_x": dict(fast=False, sparse=False, lb=(5, 1, 2), big=False, net=4, ntx=33, rix9216=None, rix16384=None),
    "odd_y": dict(fast=False, sparse=False, lb=(1, 7, 2), big=False, net=4, ntx=9, rix9216=None, rix16384=None),
    "odd_z": dict(fast=False, sparse=False, lb=(1, 2, 5), big=False, net=4, ntx=33, rix9216=None, rix16384=None),
    "line_x": dict(fast=False, sparse=False, lb=(5, 0, 0), big=False, net=1, ntx=65, rix9216=None, rix16384=None),
    "line_y": dict(fast=False, sparse=False, lb=(0, 10, 0), big=False, net=1, ntx=3, rix9216=None, rix16384=None),
    "line_z": dict(fast=False, sparse=False, lb=(0, 0, 5), big=False, net=1, ntx=65, rix9216=None, rix16384=None),
    "empty": dict(fast=False, sparse=False, lb=(0, 8, 2), big=False, net=1, ntx=0, rix9216=None, rix16384=None),
    "rix16k_in": dict(fast=True, sparse=False, lb=(0, 0, 5), big=False, net=2, ntx=64, rix9216=None, rix16384=(0, 0)),
    "rix16k_out": dict(fast=True, sparse=False, lb=(0, 0, 5), big=False, net=2, ntx=64, rix9216=None, rix16384=None),
}
for _t in S32_TAGS:  # the same unit at an odd offset: the same plan (the S32 form is the kernel's choice, by the offset)
    CLASSES[_t + "_odd"] = CLASSES[_t]

# (dims, L) of the multi-level mode: level passes on sub-boxes such as 1024 x 8 x 8
# (work items of 4096 blocks, modes_batches.level_blocks)
LEVELS = [((2048, 16, 16), 4), ((16, 2048, 16), 4), ((16, 16, 2048), 4), ((1024, 8, 24), 3), ((8, 8, 4000), 3),
          ((64, 2, 2048), 1)]

GAP_SEED = 20260
FUZZ_SEED = 31002  # chosen so that fuzz_box puts a NEGATIVE constant on s32_x and NaN, +inf and -inf on a kind-7 unit
                   # (tests/test_long_axis_cpu.py asserts both)


def layout(units):
    """-> (cell offsets, extent): random gaps of 0-8 elements, every third unit at
    an odd element offset (test_gpu_fuzz._batch), the S32 units at an even offset
    and their _odd copies at an odd one.  The gaps of a prefix of the list do not
    depend on what follows it."""
    rng = np.random.default_rng(GAP_SEED)
    offs, cur = [], 0
    for i, (tag, (W, H, D)) in enumerate(units):
        cur += int(rng.integers(0, 9))
        if i % 3 == 0 and cur % 2 == 0:
            cur += 1
        if tag in S32_TAGS and cur % 2:
            cur += 1
        if tag.endswith("_odd") and cur % 2 == 0:
            cur += 1
        offs.append(cur)
        cur += W * H * D
    return offs, cur


def survey_box(O, i, dims):
    """Field (a): the smooth SURVEY field of the parity tests."""
    W, H, D = dims
    return O.synth_box_f64(O.unit_seed(0, 0, i, 0), (0, 0, 0), W, H, D)


def fuzz_box(O, i, dims, kind=None):
    """Field (b): test_gpu_fuzz._field with kind = i % 8, so that every kind (the
    constants of either sign, zeros, subnormals, NaN / +-inf sprinkles) lands on
    a long unit."""
    return _field(np.random.default_rng(FUZZ_SEED + i), O, i, dims, kind=i % 8 if kind is None else kind)


def boxes(O, units, which):
    make = survey_box if which == "a" else fuzz_box
    return [np.ascontiguousarray(make(O, i, d), np.float64).reshape(d[2], d[1], d[0]) for i, (_, d) in enumerate(units)]
