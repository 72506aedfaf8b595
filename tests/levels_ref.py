"""CPU restatement of the opt-in multi-level transform (include/wavelet_amd.h,
"Opt-in multi-level transform"), built only from the oracle's one-level
routines on numpy sub-boxes: wavelet_decompose, inverse_wavelet_decompose,
threshold, threshold_rle and serialize.  TEST INFRASTRUCTURE ONLY: the
yardstick of tests/test_levels_cpu.py and tests/test_gpu_levels.py; the
product never imports it.

Boxes are the oracle's numpy [D, H, W] (x fastest); flat arrays are the
reference's x-slowest order (I*H + J)*D + K, here reshaped (W, H, D).  Level l
takes the corner flat[:w, :h, :d] as the cells S(x, y, z) of a w x h x d box,
i.e. the numpy box corner.transpose(2, 1, 0), and writes the box's flat
transform back into the corner.
"""
import numpy as np

from oracle import oracle as O

MAX_LEVELS = 4


def levels_for(W, H, D, want):
    if W <= 0 or H <= 0 or D <= 0:
        return 1
    L = 1
    while L < min(want, MAX_LEVELS) and W % (2 << L) == 0 and H % (2 << L) == 0 and D % (2 << L) == 0:
        L += 1
    return L


def decompose(box, L):
    """box [D, H, W] float32 -> the final flat array of L levels."""
    b = np.ascontiguousarray(box, np.float32)
    D, H, W = b.shape
    A = O.wavelet_decompose(b).reshape(W, H, D).copy()
    for l in range(2, L + 1):
        w, h, d = W >> (l - 1), H >> (l - 1), D >> (l - 1)
        sub = np.ascontiguousarray(A[:w, :h, :d].transpose(2, 1, 0))
        A[:w, :h, :d] = O.wavelet_decompose(sub).reshape(w, h, d)
    return A.reshape(-1)


def inverse(flat, W, H, D, L):
    """The final flat array of L levels -> box [D, H, W]."""
    A = np.ascontiguousarray(flat, np.float32).reshape(W, H, D).copy()
    for l in range(L, 1, -1):
        w, h, d = W >> (l - 1), H >> (l - 1), D >> (l - 1)
        sub = O.inverse_wavelet_decompose(np.ascontiguousarray(A[:w, :h, :d]).reshape(-1), w, h, d)  # [d, h, w]
        A[:w, :h, :d] = sub.transpose(2, 1, 0)
    return O.inverse_wavelet_decompose(A.reshape(-1), W, H, D)


def payload(box, L, keep=None, thresh=None):
    """-> (payload bytes, kept).  keep: the reference's rule on the final array
    (signed value at the first flat index of the largest |c|, times 1 - keep);
    thresh: an explicit threshold instead (|c| > thresh kept)."""
    b = np.ascontiguousarray(box, np.float32)
    D, H, W = b.shape
    if b.size == 0:
        return O.serialize(W, H, D, 0 if L == 1 else -L, [], []), 0
    flat = decompose(b, L)
    t = O.threshold(flat, keep) if thresh is None else float(np.float32(thresh))
    runs, vals = O.threshold_rle(flat, t)
    return O.serialize(W, H, D, W * H * D if L == 1 else -L, runs, vals), len(runs)


def decode(pay):
    """payload bytes -> (box [D, H, W], L)."""
    (W, H, D), nc, runs, vals = O.parse_payload(pay)
    L = 1 if nc >= 0 else -nc
    if W * H * D == 0:
        return np.zeros((D, H, W), np.float32), L
    return inverse(O.rle_decode(runs, vals, W * H * D), W, H, D, L), L
