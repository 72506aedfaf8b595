"""Sub-box decode without a GPU (include/wavelet_amd.h, "Opt-in sub-box decode"):
the long form of the definition (the index map, pair by pair) against the crop
of the reduced-resolution restatement, bit for bit; `end` from the formula
against the largest gathered position; the host-only wc_region_align and
wc_region_units on tables; the codec's argument errors that surface before any
device call; the map and the two host helpers under ASan + UBSan in a
stand-alone program (tests/cpp/test_regionrule.cpp)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as R
import region_ref as G
from tol_rule import field

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"

SHAPES = [((16, 16, 16), 1), ((16, 16, 16), 2), ((16, 16, 16), 3), ((32, 16, 48), 4), ((16, 8, 24), 3),
          ((12, 20, 8), 2)]


def regions_of(dims, L):
    """At the origin, in the middle (unequal extents where the box has room), at
    the far corner, and the whole box: all aligned to 2^L."""
    m = 1 << L
    mid0 = tuple(n // 2 // m * m for n in dims)
    mid = mid0 + tuple(min(e * m, n - o) for e, n, o in zip((1, 2, 1), dims, mid0))
    return [(0, 0, 0, m, m, m), mid, tuple(n - m for n in dims) + (m, m, m), (0, 0, 0) + tuple(dims)]


@pytest.mark.parametrize("dims,L", SHAPES)
def test_long_form_equals_the_crop_and_end_is_tight(dims, L):
    W, H, D = dims
    pay = R.payload(field(L % 3, W, H, D, seed=30 + L), L, keep=0.99)[0]
    for region in regions_of(dims, L):
        for r in range(L + 1):
            want = G.decode(pay, r, region)
            got = G.long_form(pay, r, region)
            assert got.shape == want.shape == tuple(reversed(G.out_dims(region, r)))
            assert got.tobytes() == want.tobytes(), (dims, L, r, region)
            p, i, end = G.index_map(dims, L, r, region)
            w, h, d = G.out_dims(region, r)
            assert sorted(i.tolist()) == list(range(w * h * d))  # the map fills the compact array exactly once
            assert end == int(p.max()) + 1, (dims, L, r, region)
    # a region with a zero extent: nothing is kept
    p, i, end = G.index_map(dims, L, 0, (0, 0, 0, 1 << L, 0, 1 << L))
    assert p.size == 0 and end == 0


ALIGN = [  # dims, levels, want -> aligned
    ((16, 16, 16), 2, (1, 2, 3, 1, 1, 1), (0, 0, 0, 4, 4, 4)),
    ((16, 16, 16), 2, (3, 4, 5, 2, 4, 3), (0, 4, 4, 8, 4, 4)),
    ((16, 16, 16), 3, (7, 8, 15, 2, 8, 1), (0, 8, 8, 16, 8, 8)),        # clipped at the box: 16 is a multiple
    ((12, 20, 8), 2, (11, 19, 7, 1, 1, 1), (8, 16, 4, 4, 4, 4)),
    ((12, 20, 8), 1, (0, 0, 0, 12, 20, 8), (0, 0, 0, 12, 20, 8)),
    ((32, 16, 48), 4, (17, 0, 31, 0, 3, 2), (16, 0, 16, 0, 16, 32)),    # a zero extent stays empty, origin rounded down
    ((6, 10, 14), 1, (5, 9, 13, 1, 1, 1), (4, 8, 12, 2, 2, 2)),
    ((0, 8, 8), 1, (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)),              # a box without cells: the all-zero region
    ((16, 16, 16), 2, (16, 16, 16, 0, 0, 0), (16, 16, 16, 0, 0, 0)),
]
ALIGN_BAD = [
    ((16, 16, 16), 2, (-1, 0, 0, 2, 2, 2)), ((16, 16, 16), 2, (0, 0, 15, 1, 1, 2)), ((16, 16, 16), 2, (0, 0, 0, 1, -1, 1)),
    ((16, 16, 16), 0, (0, 0, 0, 1, 1, 1)), ((16, 16, 16), 5, (0, 0, 0, 1, 1, 1)), ((12, 20, 8), 3, (0, 0, 0, 1, 1, 1)),
    ((5, 4, 4), 1, (0, 0, 0, 1, 1, 1)), ((0, 8, 8), 1, (0, 0, 0, 0, 1, 1)), ((-1, 8, 8), 1, (0, 0, 0, 0, 0, 0)),
]
UNITS = [(16, 8, 0, 1), (4, 4, 4, 2), (8, 16, 24, 3), (2, 2, 2, 0), (16, 16, 16, 4), (12, 20, 8, 1)]


def packed(rows):
    cur, out = 0, []
    for nx, ny, nz, r in rows:
        cur = (cur + 3) // 4 * 4
        out.append((cur, nx >> r, ny >> r, nz >> r))
        cur += (nx >> r) * (ny >> r) * (nz >> r)
    return out, cur


def test_region_align_and_units_tables(wc):
    for dims, L, want, aligned in ALIGN:
        assert wc.capi.region_align(dims, L, want) == aligned, (dims, L, want)
        if dims[0] * dims[1] * dims[2]:
            assert G.align(dims, L, want) == aligned
    for dims, L, want in ALIGN_BAD:
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.region_align(dims, L, want)
        assert ei.value.code == wc.capi.WC_ERR_INVALID, (dims, L, want)
    n = len(UNITS)
    units, _, _ = wc.capi.make_units([(64, 64, 64)] * n)
    regions = [(0, 0, 0) + u[:3] for u in UNITS]
    out, extent = wc.capi.region_units(units, n, regions, [u[3] for u in UNITS])
    want, ext = packed(UNITS)
    assert [(o.cell_offset, o.nx, o.ny, o.nz, o.reserved) for o in out[:n]] == [w + (0,) for w in want]
    assert extent == ext
    assert out[1].cell_offset == 0 and out[2].cell_offset == 4  # the unit of a zero extent takes no room
    out, extent = wc.capi.region_units(units, n, regions)        # reduce NULL: all 0
    assert extent == packed([u[:3] + (0,) for u in UNITS])[1]
    assert wc.capi.region_units(units, 0, [])[1] == 0
    for bad_r, bad_g in (([5] + [0] * (n - 1), regions), ([-1] + [0] * (n - 1), regions),
                         ([0] * n, [(0, 0, 0, 4, -4, 4)] + regions[1:])):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.region_units(units, n, bad_g, bad_r)
        assert ei.value.code == wc.capi.WC_ERR_INVALID


def test_codec_argument_errors_need_no_device(wc):
    from wavelet_compression_amd import codec
    p2 = R.payload(field(0, 12, 20, 8, 1), 2, keep=0.99)[0]
    p1odd = R.payload(field(1, 6, 5, 8, 2), 1, keep=0.99)[0]
    for pays, kw, word in (
            ([p2], dict(region=((0, 0, 0), (13, 4, 4))), "not inside"),
            ([p2], dict(region=((-1, 0, 0), (4, 4, 4))), "not inside"),
            ([p2], dict(region=((0, 0, 8), (4, 4, 9))), "not inside"),
            ([p2], dict(region=((4, 4, 4), (4, 8, 8))), "empty"),
            ([p2], dict(region=((4, 4, 4), (8, 3, 8))), "empty"),
            ([p2], dict(region=((0, 0, 0), (4, 4))), "region:"),
            ([p2], dict(region=(0, 0, 0, 4, 4, 4)), "region:"),
            ([p1odd], dict(region=((0, 0, 0), (2, 2, 2))), "divisible by 2"),
            ([p2, p1odd], dict(region=((0, 0, 0), (2, 2, 2))), "payload 1"),
            ([p2], dict(region=((0, 0, 0), (4, 4, 4)), coarsen=3), "payload 0"),
    ):
        with pytest.raises(ValueError, match=word):
            codec.decompress_payloads(pays, **kw)


def test_map_and_host_helpers_under_sanitizer(tmp_path):
    """wc_regionmap.h and wc_regionrule.cpp alone in tests/cpp/test_regionrule.cpp,
    built with ASan + UBSan (`make regionsan`), on tables from the restatement: the
    compact array of a case is a heap block of exactly its size, so a kept index
    past it is reported.  Nothing is loaded into this process."""
    subprocess.run(["make", "-s", "-C", str(CSRC), "regionsan"], check=True, timeout=600)
    lines = []
    for dims, L in SHAPES + [((2, 2, 2), 1), ((4, 4, 4), 2)]:
        for region in regions_of(dims, L) + [(0, 0, 0, 1 << L, 0, 1 << L)]:
            for r in range(L + 1):
                p, i, end = G.index_map(dims, L, r, region)
                body = " ".join(f"{int(a)} {int(b)}" for a, b in zip(p, i))
                lines.append(f"M {dims[0]} {dims[1]} {dims[2]} {L} {r} " + " ".join(map(str, region)) +
                             f" {end} {p.size} {body}")
    for dims, L, want, aligned in ALIGN:
        lines.append(f"A {dims[0]} {dims[1]} {dims[2]} {L} " + " ".join(map(str, want)) + " 0 " +
                     " ".join(map(str, aligned)))
    for dims, L, want in ALIGN_BAD:
        lines.append(f"A {dims[0]} {dims[1]} {dims[2]} {L} " + " ".join(map(str, want)) + " 1")
    want, ext = packed(UNITS)
    lines.append(f"U {len(UNITS)} " + " ".join(" ".join(map(str, u)) for u in UNITS) + f" 0 {ext} " +
                 " ".join(" ".join(map(str, w)) for w in want))
    lines.append("U 1 4 4 4 5 1 0")
    table = tmp_path / "region_table.txt"
    table.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / "tools" / "bin" / "asan" / "test_regionrule"), str(table)], capture_output=True,
                       text=True, timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and f"{len(lines)} cases" in r.stdout and " 0 failed" in r.stdout, text[-4000:]
