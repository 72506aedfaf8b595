"""The packed payload format on the CPU: the value rule q on crafted bits, the
host rule (wc_pack_unit, wc_unpack_unit, wc_packed_size, wc_payload_packed,
wc_packed_bound) against the numpy restatement tests/pack_rule.py byte for
byte, the derived error bound on the restatement alone, and the host rule under
ASan + UBSan in a stand-alone program.  No GPU."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as LR
import pack_rule as PR

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"
VS = (2, 3, 4)


@pytest.fixture(scope="module")
def units():
    return PR.batch("f32") + [(w + "/f64", p, f) for w, p, f in PR.batch("f64")[:6]]


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def test_value_rule_properties(wc):
    q = wc.capi.pack_value
    # ties go to even, in both directions, at both widths
    assert q(0x3F808000, 2) == 0x3F800000 and q(0x3F818000, 2) == 0x3F820000
    assert q(0x3F800080, 3) == 0x3F800000 and q(0x3F800180, 3) == 0x3F800200
    assert q(0x3F808001, 2) == 0x3F810000 and q(0x3F807FFF, 2) == 0x3F800000
    # a mantissa of all ones carries into the exponent
    assert q(0x3FFFFFFF, 2) == 0x40000000 and q(0x3FFFFFFF, 3) == 0x40000000
    assert q(0xBFFFFFFF, 2) == 0xC0000000
    # FLT_MAX stays finite: the truncation where the rounding would reach inf
    assert q(0x7F7FFFFF, 2) == 0x7F7F0000 and q(0xFF7FFFFF, 3) == 0xFF7FFF00
    assert q(0x7F7F8000, 2) == 0x7F7F0000 and q(0x7F7FFF80, 3) == 0x7F7FFF00
    # +-inf unchanged, NaNs stay NaN
    for V in VS:
        assert q(0x7F800000, V) == 0x7F800000 and q(0xFF800000, V) == 0xFF800000
        for nan in (0x7F800001, 0xFFC00000, 0x7FBFFFFF, 0x7F80FFFF, 0xFF8000FF):
            assert np.isnan(f32(q(nan, V))) and (q(nan, V) ^ nan) & 0x80000000 == 0
    # subnormals: to +-0 or to the nearest kept subnormal
    assert q(0x00000001, 2) == 0 and q(0x80000001, 2) == 0x80000000 and q(0x00000001, 3) == 0
    assert q(0x00008000, 2) == 0 and q(0x00018000, 2) == 0x00020000 and q(0x007FFFFF, 2) == 0x00800000
    # V = 4 is the identity; out-of-range value bytes leave the bits alone
    bits = np.concatenate([PR.SPECIALS, np.random.default_rng(1).integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)])
    for b in bits[:200]:
        assert q(int(b), 4) == int(b) and q(int(b), 7) == int(b)
    # the library's q is the restatement's, and q is idempotent
    for V in VS:
        want = PR.q(bits, V)
        got = np.array([q(int(b), V) for b in bits], np.uint32)
        assert (got == want).all(), V
        assert (PR.q(want, V) == want).all(), V
        assert ((want & np.uint32((1 << (8 * (4 - V))) - 1)) == 0).all(), V
    assert wc.capi.packed_tag(1, 2) == -33 and wc.capi.packed_tag(4, 4) == -68 and wc.capi.packed_tag(5, 2) == 0
    assert wc.capi.packed_tag(1, 1) == 0 and wc.capi.packed_tag(0, 3) == 0


def test_batch_shows_the_cases(units):
    """The batch the GPU test packs holds what the issue lists: the pair counts
    around a chunk and around a tile, a unit without cells, a fully kept unit
    with every width 0, a constant box, w = 31 and a chunk of mixed widths."""
    by = {w: p for w, p, _ in units}
    n = {w: int(np.frombuffer(p[16:20], np.int32)[0]) for w, p in by.items()}
    assert [n[k] for k in ("n0", "n1", "n63", "n64", "n65", "n128", "tile-1", "tile", "tile+1")] == \
        [0, 1, 63, 64, 65, 128, PR.TILE - 1, PR.TILE, PR.TILE + 1]
    assert len(by["empty"]) == 20 and n["empty"] == 0
    allp = PR.pack(by["all"], 3)
    assert n["all"] == 16 * 8 * 8 and not any(allp[20:20 + n["all"] // 64])
    assert n["const"] >= 1
    assert max(PR.pack(by["w31"], 2)[20:23]) == 31
    assert len(set(PR.pack(by["mixed"], 2)[20:23])) == 3
    assert n["64^3"] > 3 * PR.TILE  # several tiles of one unit
    assert {LR.decode(p)[1] for w, p, f in units if f} == {1, 2, 3}


def test_host_rule_equals_restatement(wc, units):
    C = wc.capi
    for what, pay, _ in units:
        W, H, D, L, runs, bits = PR.parse(pay)
        assert C.payload_packed(pay) == (L, 0), what
        for V in VS:
            want = PR.pack(pay, V)
            got = C.pack_unit(pay, V)
            assert got == want, (what, V)
            assert C.packed_size(got) == len(got) == PR.packed_size(want), (what, V)
            assert C.packed_size(got[:20 + PR.pad8((len(runs) + 63) // 64)]) == len(got), (what, V)
            assert len(got) <= PR.worst(W * H * D, V), (what, V)
            assert C.payload_packed(got) == (L, V), (what, V)
            back = C.unpack_unit(got)
            assert back == PR.unpack(want) == PR.quantise(pay, V), (what, V)
            if V == 4:
                assert back == pay, what
            assert C.pack_unit(back, V) == got, (what, V)  # packing the quantised payload again
            with pytest.raises(wc.WaveletError) as e:  # no existing reader takes a packed unit
                C.payload_levels(got[:20])
            assert e.value.code == C.WC_ERR_FORMAT


def test_slots_and_bound(wc):
    dims = [(8, 8, 8), (0, 4, 4), (32, 16, 8), (3, 5, 7), (64, 64, 64)]
    units, n, _ = wc.capi.make_units(dims)
    for V in VS:
        off, cap = PR.slot_offsets(dims, V)
        assert wc.capi.packed_bound(units, n, V) == cap
        assert all(o % 8 == 4 for o in off) and cap % 8 == 4
    with pytest.raises(wc.WaveletError):
        wc.capi.packed_bound(units, n, 5)


def test_host_rule_refusals(wc):
    C = wc.capi
    pay = PR.standard(8, 8, 8, 1, np.array([1, 2, 3], np.uint32), np.array([7, 8, 9], np.uint32))

    def code(fn, *a):
        with pytest.raises(wc.WaveletError) as e:
            fn(*a)
        return e.value.code

    assert code(C.pack_unit, pay, 1) == C.WC_ERR_INVALID and code(C.pack_unit, pay, 5) == C.WC_ERR_INVALID
    assert code(C.pack_unit, pay[:-1], 3) == C.WC_ERR_INVALID  # shorter than its header says
    neg = PR.standard(8, 8, 8, 1, np.array([1, 0x80000000, 3], np.uint32), np.array([7, 8, 9], np.uint32))
    assert code(C.pack_unit, neg, 3) == C.WC_ERR_FORMAT
    many = PR.standard(2, 2, 2, 1, np.zeros(9, np.uint32), np.zeros(9, np.uint32))
    assert code(C.pack_unit, many, 3) == C.WC_ERR_FORMAT  # nrle above the cell count
    bad = bytearray(pay)
    bad[12:16] = np.array([-5], np.int32).tobytes()
    assert code(C.pack_unit, bytes(bad), 3) == C.WC_ERR_FORMAT  # neither W*H*D nor -2..-4
    assert code(C.pack_unit, C.pack_unit(pay, 3), 3) == C.WC_ERR_FORMAT  # already packed
    odd = PR.standard(6, 8, 8, 1, np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    odd = odd[:12] + np.array([-2], np.int32).tobytes() + odd[16:]
    assert code(C.pack_unit, odd, 3) == C.WC_ERR_FORMAT  # 4 does not divide 6
    good = C.pack_unit(pay, 3)
    assert code(C.unpack_unit, pay) == C.WC_ERR_FORMAT  # a standard payload is not a packed unit
    assert code(C.unpack_unit, good[:-1]) == C.WC_ERR_INVALID
    wide = bytearray(good)
    wide[20] = 32
    assert code(C.unpack_unit, bytes(wide)) == C.WC_ERR_FORMAT and code(C.packed_size, bytes(wide)) == C.WC_ERR_FORMAT
    for t in (-32, -69, -(16 * 2 + 5), -(16 * 5 + 1), -(16 * 3)):
        tagged = good[:12] + np.array([t], np.int32).tobytes() + good[16:]
        assert code(C.unpack_unit, tagged) == C.WC_ERR_FORMAT, t
        assert code(C.payload_packed, tagged) == C.WC_ERR_FORMAT, t


def test_error_bound_on_the_restatement(units):
    """|| decode(q(p)) - decode(p) ||_2 <= 2^(s - 24) || decode(p) ||_2 per unit,
    no slack, on the finite-valued units of the batch; the restatement alone.
    No unit sits within 5 % of the bound (none had to be dropped): the largest
    share seen is printed."""
    worst = 0.0
    for what, pay, finite in units:
        if not finite:
            continue
        ref, _ = LR.decode(pay)
        norm = float(np.sqrt(np.sum(ref.astype(np.float64) ** 2)))
        for V in (2, 3):
            got, _ = LR.decode(PR.quantise(pay, V))
            err = float(np.sqrt(np.sum((got.astype(np.float64) - ref.astype(np.float64)) ** 2)))
            bound = 2.0 ** (8 * (4 - V) - 24) * norm
            assert err <= bound, (what, V, err, bound)
            if bound:
                worst = max(worst, err / bound)
                assert err <= 0.95 * bound, (what, V, err / bound)
        assert LR.decode(PR.quantise(pay, 4))[0].tobytes() == ref.tobytes()
    print(f"largest share of the bound: {worst:.3f}")


def test_host_rule_under_sanitizer(tmp_path, units):
    """wc_packrule.cpp alone in tests/cpp/test_pack.cpp, built with ASan + UBSan
    (`make packsan`), on payloads and expected packed bytes from the restatement:
    every buffer a heap allocation of exactly the size the call may touch.  Nothing
    is loaded into this process."""
    subprocess.run(["make", "-s", "-C", str(CSRC), "packsan"], check=True, timeout=600)
    lines = []
    for what, pay, _ in units:
        if len(pay) > 20 + 8 * 4096:
            continue
        for V in VS:
            lines.append(f"{V} {len(pay)} {pay.hex()} {PR.pack(pay, V).hex()} {PR.quantise(pay, V).hex()}")
    table = tmp_path / "pack_table.txt"
    table.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / "tools" / "bin" / "asan" / "test_pack"), str(table)], capture_output=True,
                       text=True, timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and f"{len(lines)} cases" in r.stdout and " 0 failed" in r.stdout, text[-4000:]


@pytest.mark.parametrize("mode", ["-c", "-estimate"])
@pytest.mark.parametrize("bad", ["pack=5", "pack=1", "pack=0", "pack=x", "pack=3x", "pack=2 3", "pack=2.5", "pack=-3"])
def test_cli_rejects_bad_pack(tmp_path, mode, bad):
    """A bad `pack=` is reported like a bad levels= ([error] Bad ...) and the run
    stops before it reads or writes anything."""
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    cli = ROOT / "wavelet-compression_amd" / "bin" / "wavelet-compression"
    r = subprocess.run([str(cli), f"datadir={data}/", "minfile=plt00010", "maxfile=plt00011", "minlevel=0", "maxlevel=0",
                        "components=temp", "keep=0.999", f"compresseddir={out}/", bad, mode], capture_output=True,
                       text=True, timeout=120)
    assert "[error] Bad pack" in r.stderr, r.stdout + r.stderr
    assert not out.exists()
