"""Shared by the tests of the progressive layers (test_layers_cpu.py,
test_gpu_layers.py, test_gpu_layers_mirror.py): the numpy restatement of the rule
include/wavelet_amd.h documents for wc_split_unit / wc_merge_unit and the device
and host forms.  TEST INFRASTRUCTURE ONLY.

Built on thin_rule (A(P), the thinning itself), decode_payloads.positions (exact
positions from the runs) and the oracle's RLE + serialize on the kept set.  A
split is thin_rule's thinning plus the complement inside canon(P); a merge is the
union of two position sets with the value bits verbatim."""
import numpy as np

import decode_payloads as DP
import thin_rule as TR
from oracle import oracle as O


class Overlap(Exception):
    """merge: both payloads hold a pair at one position below N."""


def candidates(bits):
    m = np.asarray(bits, np.uint32) & np.uint32(0x7FFFFFFF)
    return (m >= 1) & (m <= 0x7F800000)


def live_pairs(pay):
    """-> (W, H, D, ncoeff field, positions int64, value bits uint32) of the pairs below N."""
    W, H, D, _, nc, runs, bits = TR.parse(pay)
    assert runs.size == 0 or int(runs.max()) <= DP.M, "a negative run has no positions"
    pos = DP.positions(runs)
    live = pos < W * H * D  # strictly increasing: a prefix
    return W, H, D, nc, pos[live], bits[live]


def emit(W, H, D, nc, pos, bits):
    """The standard payload with these pairs (positions strictly increasing, bits verbatim)."""
    N = W * H * D
    if N == 0 or len(pos) == 0:
        return O.serialize(W, H, D, nc, [], [])
    mark = np.zeros(N, np.float32)
    mark[pos] = 1.0
    runs, _ = O.threshold_rle(mark, 0.0)  # the reference's run rule on the occupied set
    assert len(runs) == len(pos)
    return O.serialize(W, H, D, nc, runs, np.asarray(bits, np.uint32).view(np.float32))


def canon(pay):
    return TR.thin_thresh(pay, [0.0] * TR.MAX_LEVELS)[0]


def _rest(pay, base):
    W, H, D, nc, pos, bits = live_pairs(pay)
    bpos = live_pairs(base)[4]
    keep = candidates(bits) & ~np.isin(pos, bpos)
    return emit(W, H, D, nc, pos[keep], bits[keep])


def split_budget(pay, K):
    """-> (base, rest, kept, rest pairs, T, [thresh_1..L])."""
    base, kept, T, th, _ = TR.thin_budget(pay, K)
    rest = _rest(pay, base)
    return base, rest, kept, (len(rest) - 20) // 8, T, th


def split_thresh(pay, th):
    """-> (base, rest, kept, rest pairs)."""
    base, kept = TR.thin_thresh(pay, th)
    rest = _rest(pay, base)
    return base, rest, kept, (len(rest) - 20) // 8


def merge(a, b):
    Wa, Ha, Da, nca, pa, ba = live_pairs(a)
    Wb, Hb, Db, ncb, pb, bb = live_pairs(b)
    assert (Wa, Ha, Da, nca) == (Wb, Hb, Db, ncb), "merge: the headers differ"
    if np.intersect1d(pa, pb).size:
        raise Overlap
    pos = np.concatenate([pa, pb])
    order = np.argsort(pos, kind="stable")
    return emit(Wa, Ha, Da, nca, pos[order], np.concatenate([ba, bb])[order])
