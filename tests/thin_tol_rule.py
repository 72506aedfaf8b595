"""Shared by the tests of the tolerance forms of the compressed-domain thinning and
split (test_thin_tol_cpu.py, test_gpu_thin_tol.py, test_gpu_thin_tol_mirror.py):
the numpy restatement of the rule include/wavelet_amd.h documents for
wc_thin_tol_unit / wc_thin_tol / wc_split_tol.  TEST INFRASTRUCTURE ONLY.

The restatement goes through the dense array on purpose, where the product goes
through the pairs: thin_rule.dense (A(P)) -> leveltol_rule.level_counts (the bins
of wc_forward_levels_tol's rule on A(P), exact zeros included, NaN not counted) ->
leveltol_rule.pick (the walk, in Python floats) -> thin_rule.thin_thresh at the
thresholds it gives.  The split's rest is layers_rule's complement in canon(P)."""
import numpy as np

import layers_rule as LR
import leveltol_rule as LT
import thin_rule as TR
from tol_rule import HIST_BINS


def thresholds(pay, tol):
    """-> ([thresh_1..L] as Python floats, bound, (s*, l*) or None)."""
    W, H, D, L, _, flat = TR.dense(pay)
    if flat.size == 0:
        return LT.pick(np.zeros((L, HIST_BINS), np.uint64), L, 0, tol)
    return LT.pick(LT.level_counts(flat, W, H, D, L), L, flat.size, tol)


def thin_tol(pay, tol):
    """-> (bytes, kept, [thresh_1..L], bound, stop)."""
    th, bound, stop = thresholds(pay, tol)
    out, kept = TR.thin_thresh(pay, th)
    return out, kept, th, bound, stop


def split_tol(pay, tol):
    """-> (base, rest, kept, rest pairs, [thresh_1..L], bound)."""
    th, bound, _ = thresholds(pay, tol)
    base, rest, kept, rp = LR.split_thresh(pay, th)
    return base, rest, kept, rp, th, bound


def accepted(W, H, D, L):
    """The boxes wc_forward_levels_tol takes: 2^L divides every dimension of a unit with cells."""
    return W * H * D == 0 or all(d % (1 << L) == 0 for d in (W, H, D))


def th_bits(th, L=None):
    """float32 bit patterns of thresholds (a list of Python floats or a float32 array)."""
    t = np.asarray(th, np.float32)
    return t[:L].view(np.uint32).tolist() if L else t.view(np.uint32).tolist()


def f64_bits(x):
    return int(np.asarray(x, np.float64).reshape(1).view(np.uint64)[0])


# ---- the mixed batch of test_thin_tol_cpu.py and test_gpu_thin_tol.py (built once, left unchanged) ----------
TILE = 4096
BOX4 = (32, 16, 32)   # four pair tiles at most
BOX15 = (48, 16, 80)  # L = 4: D >> 3 = 10 and D >> 4 = 5, level boundaries inside a 16-B group
BOX72 = (64, 64, 72)  # 72 pair tiles: past WC_OPT_TOL_SOLO_TILES' default of 64 (pairs_scale.FIELDS[1])
COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)
SPECIALS = np.array([0, 0x80000000, 0x7FC00000, 0xFF800001, 0x7F800000, 0xFF800000, 1, 0x80000003], np.uint32)
_memo = {}


class Unit:
    """A payload with its tolerance; box: the float32 box [D, H, W] behind a field unit's payload (written at tol0)."""

    def __init__(self, name, dims, L, payload, tol, box=None, tol0=None):
        self.name, self.dims, self.L, self.payload, self.tol = name, dims, L, payload, float(tol)
        self.box, self.tol0 = box, tol0
        self.pairs = (len(payload) - 20) // 8
        self.N = dims[0] * dims[1] * dims[2]


def weighted_rms(pay):
    """sqrt(sum 8^lvl c^2 / N) over the finite entries of A(P): the scale a tolerance is a fraction of."""
    W, H, D, L, _, flat = TR.dense(pay)
    if flat.size == 0:
        return 0.0
    a = np.where(np.isfinite(flat), flat, np.float32(0.0)).astype(np.float64)
    w = 8.0 ** LT.level_map(W, H, D, L).reshape(-1)
    return float(np.sqrt((w * a * a).sum() / flat.size))


def _values(rng, n, specials=True):
    """n value bit patterns: distinct finite magnitudes of either sign over three decades; eight of them specials."""
    mag = np.exp(rng.permutation(n).astype(np.float64) / max(n, 1) * 7.0 - 3.5)
    v = (mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32).view(np.uint32).copy()
    if specials and n >= 16:
        v[rng.choice(n, SPECIALS.size, replace=False)] = SPECIALS
    return v


def _at(rng, N, n):
    pos = np.sort(rng.choice(N, n, replace=False)) if n else np.zeros(0, np.int64)
    return (np.diff(pos, prepend=-1) - 1).astype(np.uint32)


def zero_count_tol(pay):
    """The tolerance at which the walk passes (s, l) = (0, 1) by half a coefficient: with cnt = cnt[1][0] of A(P),
    budget = (cnt + 0.5) * 8 * hi_0^2.  One zero more in bin 0 (a NaN pair counted there, or not taken off the
    zeros) and the walk stops at (0, 1) instead."""
    W, H, D, L, _, flat = TR.dense(pay)
    cnt = int(LT.level_counts(flat, W, H, D, L)[0, 0])
    hi = LT.f32_from_bits(1 << LT.HIST_SHIFT)
    return float(np.sqrt((cnt + 0.5) * (8.0 * (hi * hi)) / flat.size)), cnt


def _units():
    import pack_rule as PR
    from tol_rule import field
    rng = np.random.default_rng(9700)
    N4 = BOX4[0] * BOX4[1] * BOX4[2]
    out = []

    def crafted(name, dims, L, runs, bits, frac):
        pay = PR.standard(*dims, L, runs, bits)
        tol = frac if frac in (0.0, np.inf) else frac * weighted_rms(pay)
        out.append(Unit(name, dims, L, pay, tol))

    for i, n in enumerate(COUNTS):
        crafted(f"n={n}", BOX4, 1 + i % 3, _at(rng, N4, n), _values(rng, n), (0.5, 0.05, 0.9)[i % 3])
    crafted("L4", (16, 16, 16), 4, _at(rng, 4096, 4096), _values(rng, 4096), 0.3)
    # the same payload at the first fraction whose walk stops at level 4
    runs, bits = _at(rng, 4096, 2000), _values(rng, 2000)
    pay = PR.standard(16, 16, 16, 4, runs, bits)
    frac = next(f for f in np.linspace(0.02, 0.98, 97) if (thresholds(pay, f * weighted_rms(pay))[2] or (0, 0))[1] == 4)
    crafted("stop-at-4", (16, 16, 16), 4, runs, bits, float(frac))
    crafted("tol=0", BOX4, 3, _at(rng, N4, 5000), _values(rng, 5000), 0.0)
    crafted("tol=inf", BOX4, 2, _at(rng, N4, 5000), _values(rng, 5000), np.inf)
    crafted("tol=inf-finite", (16, 16, 16), 4, _at(rng, 4096, 900), _values(rng, 900, specials=False), np.inf)
    crafted("empty", (0, 4, 4), 1, np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0.5)
    crafted("empty-L2", (0, 4, 4), 2, np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0.0)
    # +-0, NaN, +-inf and subnormal value bits, and five pairs past N; once at an ordinary tolerance and once
    # at the tolerance where one coefficient more in bin 0 of level 1 moves the stop
    runs = np.concatenate([_at(rng, 4096, 300), np.array([4096, 0, 7, 0x7FFFFFFF, 0], np.uint32)])
    bits = np.concatenate([_values(rng, 300), _values(rng, 5, specials=False)])
    crafted("specials", (16, 16, 16), 2, runs, bits, 0.2)
    pay = PR.standard(16, 16, 16, 2, runs, bits)
    out.append(Unit("zero-count", (16, 16, 16), 2, pay, zero_count_tol(pay)[0]))
    # field units: payloads wc_forward_levels_tol's rule wrote at 0.01 x RMS, thinned at 0.03 x RMS
    for j, (dims, L, kind) in enumerate([((16, 16, 16), 4, 0), (BOX4, 1, 1), (BOX4, 2, 2), (BOX4, 3, 0), (BOX15, 4, 2),
                                         (BOX72, 3, 0)]):
        box = field(kind, *dims, seed=170 + j).astype(np.float32)
        rms = float(np.sqrt(np.mean(box.astype(np.float64) ** 2)))
        pay = LT.payload(box, L, 0.01 * rms)[0]
        out.append(Unit(f"field-{dims[0]}x{dims[1]}x{dims[2]}-L{L}", dims, L, pay, 0.03 * rms, box, 0.01 * rms))
    return out


class Batch:
    """want[i] = thin_tol's tuple, split[i] = split_tol's."""

    def __init__(self):
        import decode_payloads as DP
        self.us = _units()
        self.n = len(self.us)
        self.dims = [u.dims for u in self.us]
        self.levels = [u.L for u in self.us]
        self.tol = np.array([u.tol for u in self.us], np.float64)
        self.want = [thin_tol(u.payload, u.tol) for u in self.us]
        self.split = []
        for u, w in zip(self.us, self.want):
            base, rest, kept, rp = LR.split_thresh(u.payload, w[2])
            assert base == w[0]
            self.split.append((base, rest, kept, rp, w[2], w[3]))
        self.buf, self.off = DP.payload_layout([u.payload for u in self.us], np.random.default_rng(9701))


def batch():
    if "batch" not in _memo:
        _memo["batch"] = Batch()
    return _memo["batch"]
