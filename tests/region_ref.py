"""CPU restatement of the sub-box decode (include/wavelet_amd.h, "Opt-in sub-box
decode"), built only from coarse_ref.py and levels_ref.py.  TEST INFRASTRUCTURE
ONLY: the yardstick of tests/test_region_cpu.py and tests/test_gpu_region.py;
the product never imports it.

Two parts: the definition (the reduced-resolution decode, cropped) and the long
form (the header's index map, one pair at a time, then levels_ref.inverse on the
compact array).  Regions are (x0, y0, z0, nx, ny, nz) in full-resolution cells;
boxes are the oracle's numpy [D, H, W] (x fastest).
"""
import numpy as np

import coarse_ref as C
import levels_ref as R


def align(dims, L, region):
    """The smallest region aligned to 2^L that contains `region` (an empty axis stays empty)."""
    m = (1 << L) - 1
    lo = [region[k] & ~m for k in range(3)]
    hi = [lo[k] if region[3 + k] == 0 else (region[k] + region[3 + k] + m) & ~m for k in range(3)]
    assert all(0 <= lo[k] and hi[k] <= dims[k] for k in range(3))
    return (lo[0], lo[1], lo[2], hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])


def out_dims(region, r):
    return region[3] >> r, region[4] >> r, region[5] >> r


def decode(pay, r, region):
    """The definition: coarse_ref.decode(pay, r), cropped -> box [nz >> r, ny >> r, nx >> r]."""
    x0, y0, z0 = (v >> r for v in region[:3])
    w, h, d = out_dims(region, r)
    if w * h * d == 0:
        return np.zeros((d, h, w), np.float32)
    full = C.decode(pay, r)
    return np.ascontiguousarray(full[z0:z0 + d, y0:y0 + h, x0:x0 + w])


def index_map(dims, L, r, region):
    """The header's steps 1-3 on every flat position of the box: (p, i) of the kept
    positions in order of p, i the index in the compact array; and `end` from the
    header's formula."""
    W, H, D = dims
    n = (W >> r, H >> r, D >> r)
    Lp = L - r
    o = tuple(v >> r for v in region[:3])
    s = out_dims(region, r)
    I, J, K = np.meshgrid(np.arange(W), np.arange(H), np.arange(D), indexing="ij")
    c = (I.reshape(-1), J.reshape(-1), K.reshape(-1))
    keep = (c[0] < n[0]) & (c[1] < n[1]) & (c[2] < n[2])  # step 1
    lvl = np.zeros(W * H * D, np.int64)                    # step 2
    if Lp >= 1:
        for j in range(Lp):
            lvl[(c[0] < n[0] >> j) & (c[1] < n[1] >> j) & (c[2] < n[2] >> j)] = j + 1
    idx = []
    for a in range(3):                                     # step 3
        high = (lvl >= 1) & (c[a] >= (n[a] >> lvl))
        q = np.where(high, c[a] - (n[a] >> lvl) - (o[a] >> lvl), c[a] - (o[a] >> lvl))
        keep &= (q >= 0) & (q < (s[a] >> lvl))
        idx.append(np.where(high, q + (s[a] >> lvl), q))
    p = np.nonzero(keep)[0]
    i = (idx[0][p] * s[1] + idx[1][p]) * s[2] + idx[2][p]  # step 4
    if s[0] * s[1] * s[2] == 0:
        end = 0
    else:
        last = [(n[a] >> 1) + (o[a] >> 1) + (s[a] >> 1) - 1 if Lp >= 1 else o[a] + s[a] - 1 for a in range(3)]
        end = (last[0] * H + last[1]) * D + last[2] + 1
    return p, i, end


def long_form(pay, r, region):
    """Gather the compact array from the dense flat array by the map, then the
    multi-level inverse of an s-unit with L - r levels (or the array read as a box)."""
    (W, H, D), L, A = C.dense(pay)
    w, h, d = out_dims(region, r)
    if w * h * d == 0:
        return np.zeros((d, h, w), np.float32)
    p, i, _ = index_map((W, H, D), L, r, region)
    comp = np.zeros(w * h * d, np.float32)
    comp[i] = A.reshape(-1)[p]
    if L - r == 0:
        return np.ascontiguousarray(comp.reshape(w, h, d).transpose(2, 1, 0))
    return R.inverse(comp, w, h, d, L - r)
