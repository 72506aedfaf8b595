"""CPU restatement of the reduced-resolution decode (include/wavelet_amd.h,
"Opt-in reduced-resolution decode"), built only from levels_ref.py and the
oracle: parse_payload, rle_decode, a corner slice, then levels_ref.inverse or a
transpose.  TEST INFRASTRUCTURE ONLY: the yardstick of tests/test_coarse_cpu.py
and tests/test_gpu_coarse.py; the product never imports it.

Boxes are the oracle's numpy [D, H, W] (x fastest); flat arrays are the
reference's x-slowest order (I*H + J)*D + K, here reshaped (W, H, D).
"""
import numpy as np

import levels_ref as R
from oracle import oracle as O


def payload_levels(pay):
    nc = int(np.frombuffer(pay[12:16], "<i4")[0])
    return 1 if nc >= 0 else -nc


def coarse_dims(W, H, D, r):
    return W >> r, H >> r, D >> r


def dense(pay):
    """payload -> ((W, H, D), L, the dense flat array A reshaped (W, H, D))."""
    (W, H, D), nc, runs, vals = O.parse_payload(pay)
    L = 1 if nc >= 0 else -nc
    return (W, H, D), L, O.rle_decode(runs, vals, W * H * D).reshape(W, H, D)


def decode(pay, r):
    """The definition: payload bytes at reduction r -> box [D >> r, H >> r, W >> r]."""
    (W, H, D), L, A = dense(pay)
    assert 0 <= r <= L
    w, h, d = coarse_dims(W, H, D, r)
    if W * H * D == 0:
        return np.zeros((d, h, w), np.float32)
    assert r == 0 or (W | H | D) & ((1 << r) - 1) == 0
    C = np.ascontiguousarray(A[:w, :h, :d])  # compact: (I*h + J)*d + K
    if r == L:
        return np.ascontiguousarray(C.transpose(2, 1, 0))  # out[z, y, x] = C(x, y, z): no arithmetic
    return R.inverse(C.reshape(-1), w, h, d, L - r)


def long_form(pay, r):
    """The full inverse's own passes l = L..r+1 on the dense A (levels_ref.inverse's
    loop, stopped early), then the corner (W, H, D) >> r read as cells."""
    (W, H, D), L, A = dense(pay)
    assert 1 <= r <= L
    A = A.copy()
    for l in range(L, r, -1):  # l >= 2: a level pass on the corner >> (l - 1)
        w, h, d = W >> (l - 1), H >> (l - 1), D >> (l - 1)
        sub = O.inverse_wavelet_decompose(np.ascontiguousarray(A[:w, :h, :d]).reshape(-1), w, h, d)  # [d, h, w]
        A[:w, :h, :d] = sub.transpose(2, 1, 0)
    w, h, d = coarse_dims(W, H, D, r)
    return np.ascontiguousarray(A[:w, :h, :d].transpose(2, 1, 0))


def block_means(box, r):
    """Mean of every 2^r-cube of box [D, H, W], in float64."""
    D, H, W = box.shape
    s = 1 << r
    return box.astype(np.float64).reshape(D // s, s, H // s, s, W // s, s).mean(axis=(1, 3, 5))
