"""The decoders' read of a packed unit, on the CPU: the corpus the GPU tests decode
(tests/test_gpu_packed_decode.py), the numpy restatement of the read
(tests/packed_decode_ref.py) against the decoders' rule, proof that the corpus
tells three plausible mistakes apart, and the new symbols.  No GPU."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import decode_payloads as DP
import pack_rule as PR
import packed_decode_ref as R

ROOT = Path(__file__).resolve().parent.parent
SURPLUS = {"n=nc+1", "n=nc+5", "n=nc+4096", "n=nc+4097", "n=nc+8193"}
SYMBOLS = ("wc_inverse_packed", "wc_inverse_packed_coarse", "wc_inverse_packed_region",
           "wc_inverse_packed_host", "wc_inverse_packed_coarse_host", "wc_inverse_packed_region_host")


def test_the_corpus_is_the_packable_crafted_units():
    """357 of the 432 crafted units; the 75 left out are exactly those with more
    pairs than cells, which the packed format cannot express."""
    crafted, corpus = DP.crafted(), R.corpus()
    assert len(crafted) == 432 and len(corpus) == 357
    left = [u for u in crafted if u not in corpus]
    assert len(left) == 75 and all(len(u.runs) > u.ncoeff for u in left)
    assert all(len(u.runs) <= u.ncoeff for u in corpus)
    # no unit is left out for another reason: every other one packs (pack_rule.pack asserts n <= cells, runs < 2^31)
    assert len(R.packed_corpus(4)) == 357
    # every class but the five surplus ones still has a unit
    have = {u.cls for u in corpus}
    for u in corpus:
        if u.L >= 2:
            have.add(f"levels:{u.L}")
    assert have >= set(DP.ALL_CLASSES) - SURPLUS
    assert not have & SURPLUS
    # the pair counts at the edges of rounds, waves and tiles, and the width-31 overshoots
    counts = {len(u.runs) for u in corpus}
    assert counts >= set(DP.FIXED_COUNTS)
    ov = [u for u in corpus if u.cls.startswith("ov:")]
    assert {u.cls for u in ov} >= {"ov:two-waves", "ov:two-tiles", "ov:lookback"}
    assert all(31 in PR.chunk_widths(u.payload)[0] for u in ov)


def test_the_read_gives_the_rule_on_the_corpus():
    """packed_decode_ref.decode of the corpus packed at V = 4 (lossless) is rule_decode of the source."""
    for u, p in zip(R.corpus(), R.packed_corpus(4)):
        assert np.array_equal(R.decode(p), DP.rule_decode(u.runs, u.bits, u.ncoeff)), u.name


@pytest.mark.parametrize("seed", PR.FUZZ_SEEDS)
def test_all_widths(seed):
    """pack_rule.fuzz_batch: every chunk width 0..31, full and short last chunks,
    short last chunks on odd boxes; the expectation is rule_decode of pack_rule.unpack."""
    units = PR.fuzz_batch(seed)
    full, short, odd_short = set(), set(), 0
    for what, pay, _ in units:
        W, H, D, L, runs, bits = PR.parse(pay)
        widths, last = PR.chunk_widths(pay)
        if widths:
            full |= set(widths[:-1] if last < 64 else widths)
            if last < 64:
                short.add(widths[-1])
                odd_short += (W * H * D) % 2
        for V in (2, 3, 4):
            packed = PR.pack(pay, V)
            _, _, _, _, r2, b2 = PR.parse(PR.unpack(packed))
            assert np.array_equal(R.decode(packed), DP.rule_decode(r2, b2, W * H * D)), (what, V)
    assert full == set(range(32)), sorted(set(range(32)) - full)
    assert len(short) >= 16 and odd_short >= 1, (sorted(short), odd_short)


# a unit of the corpus whose cells each wrong read must change
TELLS = {
    "stride8": "sparse-rows@32x16x32/L1",  # 73 pairs: a last chunk of 9, planes of 2 bytes
    "nopad": "n=1@32x16x32/L1",            # one chunk: a table of 1 byte, padded to 8
    "wrap": "lookback@32x32x32/L1",        # two tiles whose sums pass 2^32 together
}


@pytest.mark.parametrize("wrong", sorted(TELLS))
def test_sensitivity(wrong):
    by_name = {u.name: (u, p) for u, p in zip(R.corpus(), R.packed_corpus(4))}
    u, p = by_name[TELLS[wrong]]
    want = DP.rule_decode(u.runs, u.bits, u.ncoeff)
    assert np.array_equal(R.decode(p), want)
    assert not np.array_equal(R.decode(p, wrong), want), (wrong, u.name)


def test_the_new_symbols(wc):
    """The six entry points: in the library and in capi's symbol table."""
    lib = ctypes.CDLL(str(ROOT / "wavelet-compression_amd" / "lib" / "libwavelet_amd.so"))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in wc.capi.EXPORTED, name
        assert getattr(wc.capi.load_library(), name).argtypes is not None, name
