"""The crafted-histogram cases of tests/test_gpu_table_widths.py (test infrastructure;
CPU only): frames of coefficient blocks (hist_blocks.py) whose Huffman tables have a
stated number of symbols and a stated shape of frequencies, and the preconditions
each case must show on the oracle's own file before anything is compared with it.
[length_limited.rs:37-134, symbol_counting.rs:55-94, huffman/encoder.rs:45-157]

Luma AC tables of n symbols, the first n of EOB, (0,1)..(0,15), (1,1)..(1,15), ZRL,
(2,1).. in three shapes:
  limit   a bulk of m symbols at one small count under a chain of c heavier symbols
          whose counts are 1, 2, 3, 5, 8, ... times the bulk's total weight: the
          unlimited Huffman tree is deeper than 15, so package-merge's limit binds
  ties    every symbol the same count (ties2: two counts, interleaved over the
          symbol values): symbol_counting.rs:92-94's stable order decides the file
  size15  `limit` with (0, 15) the least frequent symbol: the 16-bit code (15 plus
          symbol_counting.rs:85-90's +1) followed by 15 extra bits, the longest
          piece there is; those blocks pinned at the start, middle and end of a
          chunk of 256 blocks and inside a block of more than 384 bits
The chroma AC table is given a number of symbols of another width class."""
from __future__ import annotations

import functools
import heapq
import os
import sys
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hist_blocks as hb  # noqa: E402
import oracle  # noqa: E402
from oracle import jpeg_scan  # noqa: E402

EOB, ZRL = hb.EOB, hb.ZRL
# every usable AC symbol: EOB, the 239 (run, size) without 0xFF, ZRL after run 1
SYMBOLS = ([EOB] + [(0, s) for s in range(1, 16)] + [(1, s) for s in range(1, 16)] + [ZRL]
           + [(r, s) for r in range(2, 16) for s in range(1, 16) if (r, s) != (15, 15)])
assert len(SYMBOLS) == 241 and len(set(SYMBOLS)) == 241
WIDTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 241)
FIB = [1, 2]
while len(FIB) < 15:
    FIB.append(FIB[-1] + FIB[-2])
DC_LIST = [0, 5, -5, 100, -100, 3000, -3000, 1, -1]  # (an odd count: Cb and Cr both walk all of it)
SLOT_BITS = 384  # k_emit's slot: a block of more bits takes the re-walk (slot_copy.hpp kSlotWords * 32)


def huffman_depth(freqs) -> int:
    """depth of the unlimited Huffman tree (ties to the shallower subtree: the least depth)"""
    hp = [(int(f), 0) for f in freqs]
    heapq.heapify(hp)
    while len(hp) > 1:
        a, b = heapq.heappop(hp), heapq.heappop(hp)
        heapq.heappush(hp, (a[0] + b[0], max(a[1], b[1]) + 1))
    return hp[0][1]


def width_class(n: int) -> int:
    """tail_levels' instantiation for n symbols"""
    return 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8


def length_of(hist) -> int:
    return sum(c * (16 if s == ZRL else s[0] + 1) for s, c in hist.items() if s != EOB)


def chroma_hist(n_luma: int):
    """a chroma AC histogram of another width class than the luma table's: n - 1 symbols
    with counts 1, 2, 3, 1, ... and EOB as it comes"""
    n = {1: 100, 2: 200, 4: 20, 8: 50}[width_class(n_luma)]
    return n, {s: 1 + i % 3 for i, s in enumerate(SYMBOLS[1:n])}


@dataclass
class Case:
    name: str
    coef: np.ndarray
    width: int
    height: int
    sub: int
    hists: dict
    restart_interval: int = 0
    expect: dict = field(default_factory=dict)  # what check() asserts, see there


def _frame(luma_blocks: int, sub: int):
    nl = hb.layout(sub)[1]
    assert luma_blocks % nl == 0
    return hb.frame_for(luma_blocks // nl, sub)


def chain_hist(n: int, shape: str, unit: int):
    """the `limit` / `size15` luma histogram of n symbols: (histogram, chain length)"""
    for c in range(2, 16):
        if n - c < 2:
            break
        syms = SYMBOLS[:n]
        hist = {s: unit for s in syms[c:]}
        if shape == "size15":  # (0, 15) strictly the least frequent: lower symbol values count double
            for s in syms[c:]:
                if s != ZRL and ((s[0] << 4) | s[1]) < 0x0F:
                    hist[s] = 2 * unit
        bulk = sum(hist.values())
        weights = [bulk * f for f in FIB[:c]]
        if huffman_depth(list(hist.values()) + weights) <= 15:
            continue
        # EOB counts the blocks (none is full): the lightest chain weight that holds the rest
        rest = length_of(hist) + sum(weights)
        eob = next(w for w in weights if 62 * w >= rest)
        weights.remove(eob)
        hist[EOB] = eob
        for s, w in zip(syms[1:c], sorted(weights, reverse=True)):  # the heaviest to (0, 1)
            hist[s] = w
        return hist, c
    raise AssertionError(f"no chain makes a tree deeper than 15 with {n} symbols")


def _ac_case(name, n, shape, sub):
    nl = hb.layout(sub)[1]
    nc, chroma = chroma_hist(n)
    pinned = {}
    expect = {"luma_ac": n, "chroma_ac_class": width_class(nc)}
    if shape in ("limit", "size15"):
        hist, c = chain_hist(n, shape, 4 if shape == "size15" or sub else 1)
        expect.update(luma_ac_longest=16, luma_ac_depth_over_15=True)
        if shape == "size15":
            assert sub == 0 and hist[(0, 15)] == 4 and hist[EOB] >= 86
            # chunk 0 of the emission order: its first, a middle and its last block, and a
            # block of 61 values of the lighter chain symbols round (0, 15)
            dense = []
            for s in range(c - 1, 0, -1):
                dense += [(0, s)] * min(hist[(0, s)] // 2, 60 - len(dense))
            dense.insert(30, (0, 15))
            pinned = {0: [(0, 15), (0, 1), (0, 2)], 129: [(0, 1), (0, 15), (0, 1)], 255: [(0, 2), (0, 1), (0, 15)],
                      150: dense}
            expect.update(luma_ac_rarest=0x0F, dense_block=150, size15_blocks=sorted(pinned))
        luma_blocks = hist[EOB]
    else:
        a, b = (1, 1) if shape == "ties" else (2, 3)
        order = sorted(SYMBOLS[:n], key=lambda s: (s[0] << 4) | s[1])
        for mult in range(3, 4000):
            hist = {s: mult * (a if i % 2 == 0 else b) for i, s in enumerate(order)}
            rest = length_of(hist)
            full = max(0, (rest - 31 * hist[EOB]) // 63)
            luma_blocks = full + hist[EOB]
            if luma_blocks % nl == 0 and 2 * (luma_blocks // nl) * 55 >= length_of(chroma) + 63:
                break
        expect.update(luma_ac_counts=sorted(set(hist.values())))
    w, h = _frame(luma_blocks, sub)
    coef, hists = hb.build(w, h, sub, hist, chroma, DC_LIST, DC_LIST, pinned=pinned, seed=n)
    return Case(name, coef, w, h, sub, hists, 0, expect)


def dc_chain(rarest: int, nblocks: int = 0):
    """all 16 DC categories, 15 the least frequent (`rarest` times), each next count one
    more than the sum of all but the last before it (no ties: one Huffman tree, of
    depth 15); category 0 takes what is left of nblocks"""
    counts = [rarest, rarest + 1, rarest + 1]
    while len(counts) < 16:
        counts.append(sum(counts[:-1]) + 1)
    counts[-1] += max(0, nblocks - sum(counts))
    return {15 - i: c for i, c in enumerate(counts)}


def _dc_case(name):
    ac = {(0, 1): 2, (1, 2): 1, (0, 3): 1}  # (per block, below)
    ri = 0
    pins = {}
    if name == "dc-1-2":  # one category; two
        sub, mcus = 0, 32
        luma, chroma = {5: 32}, {0: 40, 9: 24}
        expect = {"luma_dc": 1, "chroma_dc": 2}
    elif name == "dc-12-ties16":  # twelve categories; all sixteen, every count the same
        sub, mcus = 0, 96
        luma = {c: 2 + c for c in range(11)}
        luma[11] = 96 - sum(luma.values())
        chroma = {c: 12 for c in range(16)}
        expect = {"luma_dc": 12, "chroma_dc": 16, "chroma_dc_counts": [12]}
    elif name == "dc-ties16-luma":
        sub, mcus = 2, 64
        luma, chroma = {c: 16 for c in range(16)}, {c: 4 + c for c in range(12)}
        chroma[0] += 128 - sum(chroma.values())
        expect = {"luma_dc": 16, "luma_dc_counts": [16], "chroma_dc": 12}
    elif name == "dc-fib16":  # Fibonacci counts 1, 1, 2, 3, ..., 987 over 2,583 blocks; chroma: category 15 rarest
        sub, mcus = 0, 2583
        fib = [1, 1] + FIB[1:15]
        assert len(fib) == 16 and sum(fib) == 2583
        luma = {15 - i: f for i, f in enumerate(fib)}
        chroma = dc_chain(1, 2 * mcus)
        expect = {"luma_dc": 16, "luma_dc_longest": 16, "chroma_dc": 16, "chroma_dc_longest": 16,
                  "chroma_dc_rarest": 15}
    else:  # category 15 with the 16-bit code at a chunk's end and start and in the MCU after a restart marker
        ri = int(name.rsplit("ri", 1)[1])
        sub = 2
        mcus = -(-sum(dc_chain(3).values()) // 4)
        luma, chroma = dc_chain(3, 4 * mcus), {0: mcus, 9: mcus}
        # emission blocks 43 (MCU 7, its second block), 255 (a chunk's last), 512 (a chunk's first)
        pins = {43: 15, 255: 15, 512: 15}
        expect = {"luma_dc": 16, "luma_dc_longest": 16, "luma_dc_rarest": 15, "chroma_dc": 2, "dc15_blocks": sorted(pins)}
    nl = hb.layout(sub)[1]
    w, h = hb.frame_for(mcus, sub)
    coef, hists = hb.build(w, h, sub, {s: c * nl * mcus for s, c in ac.items()}, {s: c * 2 * mcus for s, c in ac.items()},
                           luma, chroma, restart_interval=ri, dc_pinned=pins, seed=len(name))
    return Case(name, coef, w, h, sub, hists, ri, expect)


def _names():
    out = []
    for n in WIDTHS:
        out.append(f"ac-{n}-ties")
        if n >= 2:
            out.append(f"ac-{n}-ties2")
        if n >= 17:
            out += [f"ac-{n}-limit", f"ac-{n}-size15"]
    out += [f"ac-{n}-limit-420" for n in (33, 129, 241)]
    out += ["dc-1-2", "dc-12-ties16", "dc-ties16-luma", "dc-fib16", "dc-cat15-ri0", "dc-cat15-ri1", "dc-cat15-ri7"]
    return out


NAMES = _names()
# blocks per case (the tests hold the built frames against it; the largest sets the time)
BLOCKS = {
    "ac-1-ties": 24, "ac-2-ties": 24, "ac-2-ties2": 24, "ac-3-ties": 24, "ac-3-ties2": 24,
    "ac-31-ties": 24, "ac-31-ties2": 24, "ac-31-limit": 480, "ac-31-size15": 2304,
    "ac-32-ties": 24, "ac-32-ties2": 30, "ac-32-limit": 504, "ac-32-size15": 2400,
    "ac-33-ties": 81, "ac-33-ties2": 81, "ac-33-limit": 528, "ac-33-size15": 2496,
    "ac-63-ties": 87, "ac-63-ties2": 90, "ac-63-limit": 795, "ac-63-size15": 3480,
    "ac-64-ties": 87, "ac-64-ties2": 96, "ac-64-limit": 810, "ac-64-size15": 3540,
    "ac-65-ties": 30, "ac-65-ties2": 72, "ac-65-limit": 825, "ac-65-size15": 3600,
    "ac-127-ties": 90, "ac-127-ties2": 222, "ac-127-limit": 1062, "ac-127-size15": 4464,
    "ac-128-ties": 90, "ac-128-ties2": 225, "ac-128-limit": 1071, "ac-128-size15": 4500,
    "ac-129-ties": 93, "ac-129-ties2": 228, "ac-129-limit": 1080, "ac-129-size15": 4536,
    "ac-241-ties": 294, "ac-241-ties2": 735, "ac-241-limit": 1398, "ac-241-size15": 5760,
    "ac-33-limit-420": 1056, "ac-129-limit-420": 2160, "ac-241-limit-420": 2796,
    "dc-1-2": 96, "dc-12-ties16": 288, "dc-ties16-luma": 384, "dc-fib16": 7749,
    "dc-cat15-ri0": 9582, "dc-cat15-ri1": 9582, "dc-cat15-ri7": 9582,
}
assert sorted(BLOCKS) == sorted(NAMES)


@functools.lru_cache(maxsize=None)
def make(name: str) -> Case:
    if name.startswith("dc-"):
        return _dc_case(name)
    part = name.split("-")
    return _ac_case(name, int(part[1]), part[2], 2 if part[-1] == "420" else 0)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> bytes:
    """the oracle's file of the case (computed once, shared by the tests)"""
    import dmmt_jpeg
    c = make(name)
    luma, chroma = dmmt_jpeg.quality_tables(90)
    return oracle.encode_coefficients(c.coef, c.width, c.height, c.sub, luma, chroma, restart_interval=c.restart_interval)


TABLES = {"luma_dc": (0, 0), "luma_ac": (1, 1), "chroma_dc": (0, 2), "chroma_ac": (1, 3)}  # DHT class, id


def check(case: Case, ref: bytes):
    """The case's preconditions, from the oracle's file and the builder's histograms."""
    jf = jpeg_scan.parse(ref)
    ex = case.expect
    assert case.coef.shape[0] <= 24000
    for tab, key in TABLES.items():
        bits, vals = jf.dht[key]
        hist = case.hists[tab]
        present = [s for s in range(256) if hist[s]]
        assert sorted(vals) == present, f"{tab}: the file's DHT symbols are not the histogram's"
        longest = max(i + 1 for i in range(16) if bits[i])
        freqs = [int(hist[s]) for s in present]
        syms, lens = oracle.code_lengths(hist)
        assert max(lens) == longest
        if tab in ex:
            assert len(vals) == ex[tab], f"{tab}: {len(vals)} symbols, not {ex[tab]}"
        if tab + "_class" in ex:
            assert width_class(len(vals)) == ex[tab + "_class"]
        if tab + "_longest" in ex:
            assert longest == ex[tab + "_longest"], f"{tab}: longest code {longest}"
        if ex.get(tab + "_depth_over_15"):
            assert huffman_depth(freqs) > 15, f"{tab}: the unlimited tree is no deeper than 15"
        if tab + "_counts" in ex:
            assert sorted(set(freqs)) == ex[tab + "_counts"]
        if tab + "_rarest" in ex:
            assert syms[0] == ex[tab + "_rarest"] and lens[0] == 16
            if tab.endswith("_ac"):
                assert syms[0] & 15 == 15
    for e in ex.get("size15_blocks", ()):  # all four (0, 15) are where they were pinned
        assert sum(hb.category(v) == 15 for v in case.coef[e, 1:]) == 1
    for e in ex.get("dc15_blocks", ()):  # (luma blocks behind another of their MCU: the same predictor)
        assert hb.category(int(case.coef[e, 0]) - int(case.coef[e - 1, 0])) == 15
    if "dense_block" in ex:  # the pinned block's bits from the oracle's code lengths
        blk = case.coef[ex["dense_block"]]
        syms, lens = oracle.code_lengths(case.hists["luma_ac"])
        ln = dict(zip(syms, lens))
        assert np.count_nonzero(blk[1:]) == 61 and any(hb.category(v) == 15 for v in blk[1:])
        bits = sum(ln[hb.category(v)] + hb.category(v) for v in blk[1:] if v) + ln[0]
        assert bits > SLOT_BITS, f"the dense block has only {bits} bits"
