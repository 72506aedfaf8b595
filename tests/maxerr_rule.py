"""CPU restatement of the pointwise (max-abs) error bound (include/wavelet_amd.h,
"Opt-in pointwise (max-abs) error bound"), composed from levels_ref.decompose /
levels_ref.inverse only.  TEST INFRASTRUCTURE ONLY: the yardstick of
tests/test_maxerr_cpu.py, tests/test_maxerr_rule_program.py and
tests/test_gpu_maxerr.py; the product never imports it.

Boxes are the oracle's numpy [D, H, W] (x fastest).  `x` is the caller's cells
in the caller's dtype (float32 or float64); the transform sees them narrowed."""
import numpy as np

import levels_ref as R

FLT_MAX = float(np.finfo(np.float32).max)
SHIFT = 19  # WC_HIST_SHIFT


def thr(b):
    """wc_tol_threshold's threshold from a first kept bin, b in 0..4095."""
    if b == 0:
        return np.float32(0.0)
    if b >= 0xFF0:
        return np.float32(FLT_MAX)
    return np.array([(b << SHIFT) - 1], np.uint32).view(np.float32)[0]


def masked(flat, t):
    """Every coefficient that is not |c| > t becomes +0.0f (strict: NaN goes)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(flat) > np.float32(t), flat, np.float32(0.0)).astype(np.float32)


def max_abs(x, r):
    """max |(double)x - (double)r| over the differences that are not NaN; 0.0 without any."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(x, np.float64).ravel() - np.asarray(r, np.float64).ravel())
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0


class Unit:
    """One unit: err(b) with a memo, so that a search and a test share the probes."""

    def __init__(self, x, flat, L):
        self.x = np.asarray(x)
        self.D, self.H, self.W = self.x.shape
        self.flat = np.ascontiguousarray(flat, np.float32)
        self.L = L
        self.memo = {}

    def recon(self, b):
        return R.inverse(masked(self.flat, thr(b)), self.W, self.H, self.D, self.L)

    def err(self, b):
        if b not in self.memo:
            self.memo[b] = max_abs(self.x, self.recon(b))
        return self.memo[b]


def search(unit, E):
    """The leading-run search, radix 16 in three passes -> b*."""
    lo = 0
    for stride in (256, 16, 1):
        j = 0
        for i in range(1, 16):
            if not unit.err(lo + i * stride) <= E:
                break
            j = i
        lo += j * stride
    return lo


def select(x, L, E, narrowed=None):
    """-> (thresh fp32, err, b*) of box x [D, H, W] at L levels under the bound E.
    narrowed: x as the transform sees it (float32; default: x.astype(float32))."""
    x = np.asarray(x)
    if x.size == 0:
        return np.float32(0.0), 0.0, 0
    b32 = np.ascontiguousarray(x.astype(np.float32) if narrowed is None else narrowed, np.float32)
    u = Unit(x, R.decompose(b32, L), L)
    b = search(u, E)
    return thr(b), u.err(b), b


def payload(x, L, E, narrowed=None):
    """-> (payload bytes, kept, thresh, err, b*): levels_ref.payload at thr(b*)."""
    x = np.asarray(x)
    t, e, b = select(x, L, E, narrowed)
    b32 = np.ascontiguousarray(x.astype(np.float32) if narrowed is None else narrowed, np.float32)
    if x.size == 0:
        pay, kept = R.payload(b32, L, thresh=0.0)
    else:
        pay, kept = R.payload(b32, L, thresh=float(t))
    return pay, kept, t, e, b
