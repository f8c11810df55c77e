"""tests/tools/hist_blocks.py (blocks with a wanted symbol histogram) against the oracle,
and the preconditions of every crafted case of tests/test_gpu_table_widths.py on the
oracle alone.  The builder's reported histograms must be the wanted ones and must be
what oracle/jpeg_scan.decode_coefficients plus the symboliser give back from the
oracle's own file of the same blocks.  [categorize.rs:132-151, symbol_counting.rs:55-94]"""
import os
import sys

import numpy as np
import pytest

import dmmt_jpeg
import oracle
from oracle import jpeg_scan

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import hist_blocks as hb  # noqa: E402
import table_width_cases as cases  # noqa: E402

LUMA_Q, CHROMA_Q = dmmt_jpeg.quality_tables(90)

AC_A = {(0, 1): 40, (0, 15): 3, (1, 2): 7, (15, 0): 5, (15, 14): 2, (14, 15): 1, (7, 9): 9, (3, 3): 11, (0, 8): 30}
AC_B = {(0, 2): 25, (2, 1): 6, (15, 0): 9, (5, 5): 5, (11, 12): 3}
DC_ALL = {c: 1 + (c * 5) % 7 for c in range(16)}


def _round_trip(coef, w, h, sub, ri):
    ref = oracle.encode_coefficients(coef, w, h, sub, LUMA_Q, CHROMA_Q, restart_interval=ri)
    jf, dec, pad_ok = jpeg_scan.decode_coefficients(ref)
    assert pad_ok and (jf.width, jf.height, jf.restart_interval) == (w, h, ri)
    assert np.array_equal(dec, coef)
    return jf, hb.symbolise(dec, sub, ri)


def _same(h1, h2):
    return all(np.array_equal(h1[k], h2[k]) for k in hb.HIST_NAMES)


@pytest.mark.parametrize("sub,w,h,ri", [(0, 96, 64, 0), (2, 128, 64, 0), (0, 64, 96, 5), (2, 192, 48, 1)])
def test_histograms_are_the_wanted_ones_and_the_oracles(sub, w, h, ri):
    mcus = hb.geometry(w, h, sub)
    nl = hb.layout(sub)[1]
    luma_dc = dict(DC_ALL)
    luma_dc[3] += nl * mcus - sum(luma_dc.values())
    coef, hists = hb.build(w, h, sub, AC_A, AC_B, luma_dc, [0, 7, -7, 300, -300, 9000, -9000, 1, -1],
                           restart_interval=ri, seed=sub + ri)
    assert coef.shape == (mcus * (nl + 2), 64) and coef.dtype == np.int16
    for cls, want in (("luma", AC_A), ("chroma", AC_B)):
        got = hists[cls + "_ac"]
        for r in range(16):
            for s in range(16):
                if (r, s) != (0, 0):
                    assert got[(r << 4) | s] == want.get((r, s), 0)
    assert [int(x) for x in hists["luma_dc"][:16]] == [luma_dc.get(c, 0) for c in range(16)]
    assert int(np.abs(coef[:, 0].astype(int)).max()) <= hb.MAX_DC and coef.min() >= -32767
    jf, back = _round_trip(coef, w, h, sub, ri)
    assert _same(hists, back)
    for name, key in cases.TABLES.items():  # and the file's tables hold exactly the counted symbols
        assert sorted(jf.dht[key][1]) == [s for s in range(256) if hists[name][s]]
    # the values of a category take both signs and both ends of its range
    v15 = {int(v) for v in coef[:, 1:].ravel() if abs(int(v)) >= 16384}
    assert {32767, -32767, 16384} <= v15


def test_stated_eob_count_and_pinned_blocks():
    """EOB stated: exactly that many blocks end before position 63, the others are
    filled to it; pinned blocks hold their symbols in order"""
    ac = {(0, 0): 5, (0, 1): 200, (1, 4): 60, (2, 7): 41, (15, 0): 4, (6, 15): 3, (0, 15): 2}
    total = sum(c * (16 if s == (15, 0) else s[0] + 1) for s, c in ac.items() if s != (0, 0))
    full = (total - 5 * 30) // 63
    w, h = hb.frame_for(full + 5, 0)
    pinned = {6: [(0, 15), (15, 0), (6, 15), (0, 1)], 1: [(2, 7)]}  # block 6 is luma (4:4:4: every third), 1 chroma
    coef, hists = hb.build(w, h, 0, ac, {(2, 7): 1}, [0], [3, -3], pinned=pinned, seed=9)
    assert hists["luma_ac"][0] == 5
    luma = coef[0::3]
    assert int(np.count_nonzero(luma[:, 63])) == full
    assert abs(int(coef[6, 1])) >= 16384 and abs(int(coef[6, 24])) >= 16384 and coef[6, 25] != 0
    assert np.count_nonzero(coef[6, 1:]) == 3 and np.count_nonzero(coef[1, 1:]) == 1 and coef[1, 3] != 0
    assert _same(hists, _round_trip(coef, w, h, 0, 0)[1])


def test_dc_pins_and_the_value_range():
    """a category-15 difference where it is wanted: never from a predictor of 0"""
    dc = {15: 3, 14: 20, 0: 30, 6: 43}
    pins = {1: 15, 13: 15, 39: 15}  # 4:2:0: blocks 1, 13 = MCU 2's second, 39 = MCU 6's last luma block
    coef, hists = hb.build(64, 96, 2, {(0, 1): 5}, {(0, 1): 5}, dc, [0], restart_interval=2, dc_pinned=pins, seed=4)
    assert [int(hists["luma_dc"][c]) for c in (15, 14, 0, 6)] == [3, 20, 30, 43]
    for e in pins:
        assert abs(int(coef[e, 0]) - int(coef[e - 1, 0])) >= 16384
    assert int(np.abs(coef[:, 0].astype(int)).max()) <= hb.MAX_DC
    assert _same(hists, _round_trip(coef, 64, 96, 2, 2)[1])


def test_what_the_builder_refuses():
    ok = dict(width=16, height=16, sub=0, luma_ac={(0, 1): 1}, chroma_ac={}, luma_dc=[0], chroma_dc=[0])
    hb.build(**ok)
    for bad in (dict(luma_ac={(15, 15): 1}),            # symbol 0xFF
                dict(luma_ac={(3, 0): 1}),              # no such symbol
                dict(luma_ac={(0, 16): 1}),
                dict(luma_ac={(15, 0): 1}),             # a ZRL with nothing behind it
                dict(luma_ac={(9, 1): 40}),             # more than four blocks hold
                dict(luma_ac={(0, 0): 2, (0, 1): 7}),   # two blocks cannot be filled to position 63 with 7 values
                dict(luma_dc=[16384]),                  # a DC value past +-16383
                dict(luma_dc={15: 4}),                  # category 15 from a predictor of 0
                dict(luma_dc={3: 5}),                   # five differences, four blocks
                dict(width=20), dict(height=65536 + 8), dict(sub=1),
                dict(pinned={0: [(0, 2)]}),             # a symbol the histogram does not have
                dict(pinned={12: [(0, 1)]})):           # a block outside the frame
        with pytest.raises(ValueError):
            hb.build(**{**ok, **bad})


@pytest.mark.parametrize("name", cases.NAMES)
def test_table_width_case_preconditions(name):
    """every case of tests/test_gpu_table_widths.py shows on the oracle alone what it is for"""
    case = cases.make(name)
    assert case.coef.shape[0] == cases.BLOCKS[name]
    cases.check(case, cases.reference(name))


def test_table_width_cases_cover_every_instantiation():
    """the luma and the chroma AC table of a case are of different width classes, every
    class boundary is met from both sides, and so are the sorts' (128 | 129 symbols)"""
    seen = set()
    for name in cases.NAMES:
        if name.startswith("ac-"):
            h = cases.make(name).hists
            nl, nc = (int(np.count_nonzero(h[k])) for k in ("luma_ac", "chroma_ac"))
            assert cases.width_class(nl) != cases.width_class(nc)
            seen.add((nl, name.split("-")[2]))
    for n in cases.WIDTHS:
        assert (n, "ties") in seen and (n < 2 or (n, "ties2") in seen)
        assert n < 17 or ((n, "limit") in seen and (n, "size15") in seen)
