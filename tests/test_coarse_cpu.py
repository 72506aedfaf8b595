"""Reduced-resolution decode without a GPU (include/wavelet_amd.h, "Opt-in
reduced-resolution decode"): the host-only wc_coarse_units; the CPU restatement
(coarse_ref.py) against the long form of the definition, bit for bit; the
block-mean property with its derived bound; the codec's argument errors that
surface before any device call."""
import numpy as np
import pytest

import coarse_ref as C
import levels_ref as R

SHAPES = [((16, 16, 16), 3), ((32, 32, 32), 3), ((16, 8, 24), 3), ((12, 20, 8), 2), ((8, 8, 8), 1), ((64, 64, 64), 4)]


def synth(oracle, W, H, D):
    return oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3, 1), (0, 0, 0), W, H, D))


def test_coarse_units_table(wc):
    dims = [(64, 64, 64), (12, 20, 8), (0, 5, 3), (2, 2, 2), (6, 10, 14), (16, 8, 24)]
    reduce = [2, 1, 1, 1, 0, 3]
    units, n, _ = wc.capi.make_units(dims, offsets=[7, 1000, 3, 99999, 5, 0])  # the input offsets do not matter
    out, extent = wc.capi.coarse_units(units, n, reduce)
    want_dims = [(16, 16, 16), (6, 10, 4), (0, 2, 1), (1, 1, 1), (6, 10, 14), (2, 1, 3)]
    cur = 0
    for i in range(n):
        cur = (cur + 3) // 4 * 4  # each start rounded up to 4 elements
        assert (out[i].nx, out[i].ny, out[i].nz) == want_dims[i], i
        assert out[i].cell_offset == cur and out[i].reserved == 0, i
        cur += want_dims[i][0] * want_dims[i][1] * want_dims[i][2]
    assert extent == cur
    # the unit without cells keeps its shifted dims and takes no room
    assert out[3].cell_offset == out[2].cell_offset == 4096 + 240
    # one value for all units; no units
    out, extent = wc.capi.coarse_units(units, 1, 3)
    assert (out[0].nx, out[0].ny, out[0].nz, out[0].cell_offset, extent) == (8, 8, 8, 0, 512)
    assert wc.capi.coarse_units(units, 0, [])[1] == 0
    for bad in ([-1] + reduce[1:], [5] + reduce[1:]):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.coarse_units(units, n, bad)
        assert ei.value.code == wc.capi.WC_ERR_INVALID


@pytest.mark.parametrize("dims,L", SHAPES)
def test_restatement_equals_the_long_form_and_the_block_means(oracle, dims, L):
    """The corner of the coefficient array through L - r levels is, bit for bit,
    the corner after the full inverse's passes l = L..r+1 on the dense array;
    r = 0 is levels_ref.decode.  Property: each cell is within 3 r 2^-23 max|full|
    of the mean of its 2^r-cube of the full reconstruction (one rounding of at
    most 2^-24 of a block mean per synthesis step, 3 steps per level, r levels,
    a factor 2 of margin)."""
    box = synth(oracle, *dims)
    W, H, D = dims
    for keep in (0.99, 0.999):
        pay, _ = R.payload(box, L, keep=keep)
        full, got = R.decode(pay)
        assert got == L == C.payload_levels(pay)
        assert C.decode(pay, 0).tobytes() == full.tobytes()
        top = float(np.max(np.abs(full.astype(np.float64))))
        for r in range(1, L + 1):
            coarse = C.decode(pay, r)
            assert coarse.shape == (D >> r, H >> r, W >> r)
            assert coarse.tobytes() == C.long_form(pay, r).tobytes(), (dims, L, r, keep)
            dev = float(np.max(np.abs(coarse.astype(np.float64) - C.block_means(full, r))))
            bound = 3 * r * 2.0 ** -23 * top
            print(dims, L, r, keep, "max deviation from block means", dev, "bound", bound, "of max", dev / top)
            assert dev <= bound, (dims, L, r, keep, dev, bound)


def test_corner_is_the_result_when_r_equals_L(oracle):
    """r = L runs no arithmetic: the cells are payload values or zeros, in Box3D order."""
    box = synth(oracle, 16, 8, 24)
    pay, _ = R.payload(box, 3, keep=0.99)
    (W, H, D), L, A = C.dense(pay)
    out = C.decode(pay, 3)
    for x in range(2):
        for y in range(1):
            for z in range(3):
                assert out[z, y, x] == A[x, y, z]


def test_codec_argument_errors_before_any_device_call(wc, oracle):
    from wavelet_compression_amd import codec
    box = synth(oracle, 8, 8, 8)
    one = oracle.compress_payload(box, 0.99)[0]
    three = R.payload(box, 3, keep=0.99)[0]
    odd = oracle.compress_payload(synth(oracle, 6, 5, 8), 0.99)[0]
    l2 = R.payload(synth(oracle, 12, 20, 8), 2, keep=0.99)[0]
    for bad in (-1, 5, 1.5, "1", True, None):
        with pytest.raises(ValueError, match="coarsen"):
            codec.decompress_payloads([one], coarsen=bad)
    with pytest.raises(ValueError, match=r"payload 1: coarsen=2 exceeds its 1 transform level"):
        codec.decompress_payloads([three, one], coarsen=2)
    with pytest.raises(ValueError, match=r"payload 2 \(6x5x8\): coarsen=1 needs W, H and D divisible by 2"):
        codec.decompress_payloads([three, one, odd], coarsen=1)
    with pytest.raises(ValueError, match=r"payload 0: coarsen=3 exceeds its 2 transform level"):
        codec.decompress_payloads([l2, three], coarsen=3)
