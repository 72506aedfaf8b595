"""The probe-tile edges of the max-error mode (wc_maxerr.hip k_maxerr_probe).  TEST
INFRASTRUCTURE ONLY: shared by tests/test_rule_fuzz_cpu.py, which proves on the
restatement alone that every shape shows the class the table claims and that a
localised unit's result hangs on its target tile, and tests/test_gpu_maxerr_fuzz.py,
which runs the units on the device.

A probe tile is TX x TY x TZ = 16 x 8 x 32 cells, 16 x 16 x 32 when the call's largest
L is 4, clipped to the unit.  SHAPES are the smallest boxes that put every admissible
clip on every axis with more than one tile on that axis, so that a clipped tile has
x0 / y0 / z0 > 0.  TABLE restates by hand, per shape and TY, the tiles per axis and the
extents of the last tile on each axis; tiles() recomputes them.

Per shape one plain unit (tol_rule.field) and one localised unit per target tile (the
first tile, the last along x, y and z, the last corner tile; the same tile once): noise
in the tile, every other cell exactly 0.0.  A tile is aligned to 2^L, so every
coefficient outside the tile's index ranges is an exact zero and every cell outside
reconstructs to 0 under any threshold: the unit's err comes from that tile alone, and a
kernel that skipped or mis-indexed it returns other bits."""
import numpy as np

from tol_rule import field

TX, TZ = 16, 32
# (dims (W, H, D), L)
SHAPES = [((18, 10, 34), 1), ((18, 18, 34), 1), ((20, 12, 36), 2), ((24, 24, 40), 3), ((40, 8, 56), 3),
          ((28, 12, 60), 2), ((30, 14, 62), 1), ((32, 16, 64), 3), ((48, 48, 48), 4), ((16, 48, 32), 4)]
# dims -> {TY: ((tiles in x, y, z), (extent of the last tile in x, y, z))}; an L = 4 shape runs under TY = 16 alone
TABLE = {
    (18, 10, 34): {8: ((2, 2, 2), (2, 2, 2)), 16: ((2, 1, 2), (2, 10, 2))},
    (18, 18, 34): {8: ((2, 3, 2), (2, 2, 2)), 16: ((2, 2, 2), (2, 2, 2))},
    (20, 12, 36): {8: ((2, 2, 2), (4, 4, 4)), 16: ((2, 1, 2), (4, 12, 4))},
    (24, 24, 40): {8: ((2, 3, 2), (8, 8, 8)), 16: ((2, 2, 2), (8, 8, 8))},
    (40, 8, 56): {8: ((3, 1, 2), (8, 8, 24)), 16: ((3, 1, 2), (8, 8, 24))},
    (28, 12, 60): {8: ((2, 2, 2), (12, 4, 28)), 16: ((2, 1, 2), (12, 12, 28))},
    (30, 14, 62): {8: ((2, 2, 2), (14, 6, 30)), 16: ((2, 1, 2), (14, 14, 30))},
    (32, 16, 64): {8: ((2, 2, 2), (16, 8, 32)), 16: ((2, 1, 2), (16, 16, 32))},
    (48, 48, 48): {16: ((3, 3, 2), (16, 16, 16))},
    (16, 48, 32): {16: ((1, 3, 1), (16, 16, 32))},
}
# The odd block counts of a last tile, dims -> (cx, cy, cz) >> (L - 1) under TY = 8: the blocks of its deepest
# level synthesis (L = 1: its level-1 blocks themselves)
ODD_BLOCKS = {(40, 8, 56): (1, 1, 3), (28, 12, 60): (3, 1, 7), (30, 14, 62): (7, 3, 15)}


def ty_of(maxl):
    return 16 if maxl == 4 else 8


def axis_tiles(n, t):
    """[(origin, extent)] of the tiles of edge t along an axis of n cells."""
    return [(o, min(t, n - o)) for o in range(0, n, t)]


def tiles(dims, ty):
    W, H, D = dims
    return axis_tiles(W, TX), axis_tiles(H, ty), axis_tiles(D, TZ)


def targets(dims, ty):
    """{name: ((x0, ex), (y0, ey), (z0, ez))} of the target tiles, each tile once under its first name."""
    xs, ys, zs = tiles(dims, ty)
    want = [("first", (0, 0, 0)), ("last_x", (len(xs) - 1, 0, 0)), ("last_y", (0, len(ys) - 1, 0)),
            ("last_z", (0, 0, len(zs) - 1)), ("corner", (len(xs) - 1, len(ys) - 1, len(zs) - 1))]
    out, seen = {}, set()
    for name, (i, j, k) in want:
        if (i, j, k) not in seen:
            seen.add((i, j, k))
            out[name] = (xs[i], ys[j], zs[k])
    return out


def inside(dims, box):
    """bool [D, H, W]: the cells of the tile box ((x0, ex), (y0, ey), (z0, ez))."""
    W, H, D = dims
    (x0, ex), (y0, ey), (z0, ez) = box
    m = np.zeros((D, H, W), bool)
    m[z0:z0 + ez, y0:y0 + ey, x0:x0 + ex] = True
    return m


class Unit:
    """name, dims, L, box (float32 [D, H, W]), tile (the target tile's box; None: the plain unit)."""

    def __init__(self, name, dims, L, box, tile):
        self.name, self.dims, self.L, self.box, self.tile = name, dims, L, box, tile


def units(ty):
    """The units of a call whose probe tile is 16 x ty x 32, in SHAPES' order."""
    out = []
    for s, (dims, L) in enumerate(SHAPES):
        if ty not in TABLE[dims]:
            continue
        W, H, D = dims
        out.append(Unit(f"{W}x{H}x{D}-L{L}", dims, L, field(s % 2, W, H, D, seed=300 + s), None))
        noise = field(1, W, H, D, seed=330 + s)
        for name, box in targets(dims, ty).items():
            b = np.where(inside(dims, box), noise, np.float32(0.0)).astype(np.float32)
            out.append(Unit(f"{W}x{H}x{D}-L{L}-{name}", dims, L, b, box))
    return out
