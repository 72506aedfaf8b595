"""numpy restatement of the decoders' read of a packed unit (csrc/wc_packsrc.h).
TEST INFRASTRUCTURE ONLY: the yardstick of tests/test_packed_decode_cpu.py and the
corpus of tests/test_gpu_packed_decode.py; the product never imports it.

decode() follows the kernels, not pack_rule.unpack: a decode tile is 64 chunks;
chunk c of a unit sits at 20 + pad8(nch) + 8 (sum of the widths before c) + 64 V c;
only the last chunk is short (planes of ceil(m / 8) bytes, value planes of m
bytes); a tile's sum of run + 1 is taken from the planes' popcounts (the
look-back's derive path) and the sums over tiles saturate at 2^32 - 1 as Sat32
does.  Three deliberately wrong forms (`wrong=`) prove that the corpus can tell:
  "stride8"  a short last chunk's planes strided by 8 bytes, as a full chunk's
  "nopad"    the width table taken as nch bytes, without pad8
  "wrap"     the sums over tiles wrapping mod 2^32 instead of saturating
"""
import functools

import numpy as np

import decode_payloads as DP
import pack_rule as PR

TILE_CHUNKS = 64
SAT = 2 ** 32 - 1


def _plane(packed, pos, nbytes, m):
    raw = np.frombuffer(packed[pos:pos + nbytes].ljust(nbytes, b"\0"), np.uint8)  # (a wrong form may read past the unit)
    return np.unpackbits(raw, bitorder="little")[:m].astype(np.uint32)


def decode(packed, wrong=None):
    """A packed unit -> the flat array's bits (uint32[W*H*D]) as k_decode_region
    places them: pair k at (sum over earlier tiles, saturating) + (sum inside its
    tile through k) - 1 while that is below W*H*D."""
    h = np.frombuffer(packed[:20], np.int32)
    W, H, D, t, n = (int(v) for v in h)
    V = (-t) >> 4
    nc = W * H * D
    nch = (n + 63) // 64
    table = np.frombuffer(packed[20:20 + nch], np.uint8).astype(np.int64)
    body = 20 + (nch if wrong == "nopad" else PR.pad8(nch))
    before = np.concatenate([[0], np.cumsum(table)])  # widths before chunk c
    out = np.zeros(nc, np.uint32)
    prefix = 0  # the sum over the earlier tiles, as the look-back hands it on
    for t0 in range(0, nch, TILE_CHUNKS):
        runs, bits = [], []
        tile_sum = 0
        for c in range(t0, min(t0 + TILE_CHUNKS, nch)):
            m = min(64, n - 64 * c)
            w = int(table[c])
            pl = (m + 7) // 8
            pos = body + 8 * int(before[c]) + 64 * V * c
            stride = 8 if wrong == "stride8" else pl
            r = np.zeros(m, np.uint32)
            chunk_sum = m
            for b in range(w):
                plane = _plane(packed, pos + b * stride, pl, m)
                r |= plane << np.uint32(b)
                chunk_sum += int(plane.sum()) << b  # m_c + sum_b 2^b popcount(plane b)
            vs = pos + w * stride
            v = np.zeros(m, np.uint32)
            for p in range(V):
                got = np.frombuffer(packed[vs + p * m:vs + p * m + m], np.uint8).astype(np.uint32)
                v[:got.size] |= got << np.uint32(8 * (3 - p))
            runs.append(r)
            bits.append(v)
            tile_sum += chunk_sum
        runs, bits = np.concatenate(runs), np.concatenate(bits)
        incl = np.cumsum(runs.astype(np.int64) + 1)
        assert int(incl[-1]) == tile_sum or wrong  # the popcount sum is the scan's
        pos = np.minimum(prefix + incl, SAT) - 1
        keep = pos < nc
        out[pos[keep]] = bits[keep]
        prefix = (prefix + tile_sum) % 2 ** 32 if wrong == "wrap" else min(prefix + tile_sum, SAT)
    return out


def packable(u):
    """A crafted unit the packed format can express: no more pairs than cells (wc_pack refuses the rest)."""
    return len(u.runs) <= u.ncoeff


@functools.lru_cache(maxsize=None)
def corpus():
    """The packable units of decode_payloads.crafted(), in its order."""
    return tuple(u for u in DP.crafted() if packable(u))


@functools.lru_cache(maxsize=None)
def packed_corpus(V):
    """corpus() packed at V value bytes (computed once, left unchanged)."""
    return tuple(PR.pack(u.payload, V) for u in corpus())
