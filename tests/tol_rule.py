"""Shared by the RMSE-tolerance tests (test_tol_cpu.py, test_gpu_tol.py): the
numpy / Python-float restatement of the selection rule that
include/wavelet_amd.h documents for wc_tol_threshold, and the test fields.

Python floats are IEEE doubles and every operation below is rounded on its
own, as the rule demands (no fused multiply-add)."""
import math

import numpy as np

HIST_BINS, HIST_SHIFT = 4096, 19
FLT_MAX = float(np.finfo(np.float32).max)
# The rule bounds the MODEL error by tol; the actual error adds the fp32
# rounding of the round trip: actual <= model + rounding (triangle inequality)
# <= tol + rounding.  MARGIN on the actual RMSE is checked at tol >= 1e-3 only,
# where MARGIN * tol >= 1e-6; FLOOR asks every test input's keep-everything
# round trip (rounding alone, fields with |x| <= 8) to stay within half of that.
MARGIN = 1e-3
FLOOR = 5e-7


def f32_from_bits(bits: int) -> float:
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def tol_rule(counts, ncoeff: int, tol: float):
    """(fp32 threshold as a Python float, model RMSE bound) for one unit's bin counts."""
    tol = float(tol)
    budget = (tol * tol) * float(ncoeff)
    S, bstar = 0.0, HIST_BINS
    for b in np.nonzero(np.asarray(counts))[0].tolist():
        hi = f32_from_bits((b + 1) << HIST_SHIFT) if b < 0xFEF else math.inf
        t = S + float(int(counts[b])) * (8.0 * (hi * hi))
        if not (t <= budget):
            bstar = b
            break
        S = t
    if bstar == 0:
        thresh = 0.0
    elif bstar >= 0xFF0:
        thresh = FLT_MAX
    else:
        thresh = f32_from_bits((bstar << HIST_SHIFT) - 1)
    bound = math.sqrt(S / float(ncoeff)) if ncoeff else 0.0
    return thresh, bound


def same_bits(a: float, b: float, kind=np.float64) -> bool:
    return np.array([a], kind).tobytes() == np.array([b], kind).tobytes()


def field(kind: int, W: int, H: int, D: int, seed: int) -> np.ndarray:
    """A float32 Box3D [D, H, W] with |x| <= 8: 0 smooth + small noise, 1 uniform
    noise, 2 smooth with a sharp front, 3 constant."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    if kind == 0:
        f = 6.0 * np.sin(0.21 * x + 0.1 * seed) * np.cos(0.17 * y) * np.cos(0.13 * z) + 0.01 * rng.standard_normal((D, H, W))
    elif kind == 1:
        f = rng.uniform(-8.0, 8.0, (D, H, W))
    elif kind == 2:
        f = 3.0 * np.tanh(2.0 * (x + y + z - 0.5 * (W + H + D))) + 0.3 * np.sin(0.4 * x) + 1e-3 * rng.standard_normal((D, H, W))
    else:
        f = np.full((D, H, W), 5.0)
    return np.clip(f, -8.0, 8.0).astype(np.float32)
