"""Coefficient blocks with a wanted symbol histogram (test infrastructure; CPU only).

`build` turns a wanted AC histogram {(run, size): count} and wanted DC differences,
per component class (luma, chroma), into emission-order zigzag int16[nblocks, 64]
for a 4:4:4 or 4:2:0 frame, and reports the exact histograms those blocks have,
counted by `symbolise`: the run/size walk, ZRL for runs of 16 or more, EOB unless
position 63 is non-zero [categorize.rs:132-151, symbol_counting.rs:55-74].  The
back halves under test (`dmmt_encode_coefficients`, the oracle's
`ref_encode_coefficients`) take such blocks directly, so a test can put any
histogram it wants in front of the Huffman table builders.

Rules the blocks keep:
  * a symbol (r, s) is r zeros and a value of category s; the values and signs vary
    over the category's range (both ends first: all-ones and all-zeros extra bits);
  * a block closes with EOB or with a symbol that lands on position 63, never with
    filler; EOB's count is a by-product (one per block that is not full) unless the
    histogram states it, and then it is met exactly or the build fails;
  * ZRL (15, 0) is 16 more zeros in front of another symbol of the histogram;
  * values stay in -32767..32767 and symbol 0xFF (15, 15) is refused: both are
    errors of the encoders, tested elsewhere;
  * DC values stay within +-16383, so every difference has category <= 15.
"""
from __future__ import annotations

import numpy as np

MAX_DC = 16383
EOB, ZRL = (0, 0), (15, 0)
HIST_NAMES = ("luma_dc", "luma_ac", "chroma_dc", "chroma_ac")


def category(v: int) -> int:
    return abs(int(v)).bit_length()


def layout(sub: int):
    """(MCU edge in pixels, luma blocks per MCU, blocks per MCU)"""
    if sub not in (0, 2):
        raise ValueError("4:4:4 (0) or 4:2:0 (2)")
    return (8, 1, 3) if sub == 0 else (16, 4, 6)


def geometry(width: int, height: int, sub: int) -> int:
    """MCUs of the frame; its sides must be multiples of the MCU and fit in 16 bits"""
    edge = layout(sub)[0]
    for v in (width, height):
        if v <= 0 or v % edge or v > 65535:
            raise ValueError(f"{width}x{height}: sides must be multiples of {edge}, at most 65535")
    return (width // edge) * (height // edge)


def frame_for(mcus: int, sub: int):
    """(width, height) of a frame of exactly `mcus` MCUs: the fewest MCU rows that divide it"""
    edge = layout(sub)[0]
    per_row = 65535 // edge
    for rows in range(-(-mcus // per_row), mcus + 1):
        if mcus % rows == 0 and rows <= per_row:
            return edge * (mcus // rows), edge * rows
    raise ValueError(f"no frame of {mcus} MCUs")


def block_class(e: int, sub: int) -> str:
    _, nl, bpm = layout(sub)
    return "luma" if e % bpm < nl else "chroma"


def class_blocks(cls: str, mcus: int, sub: int):
    """emission indices of the class's blocks, in emission order"""
    _, nl, bpm = layout(sub)
    ks = range(nl) if cls == "luma" else range(nl, bpm)
    return [m * bpm + k for m in range(mcus) for k in ks]


def symbolise(blocks, sub: int, restart_interval: int = 0):
    """The four 256-bin histograms of emission-order zigzag blocks."""
    _, nl, bpm = layout(sub)
    h = {k: np.zeros(256, np.int64) for k in HIST_NAMES}
    pred = [0, 0, 0]
    for e, blk in enumerate(np.asarray(blocks).tolist()):
        k = e % bpm
        if restart_interval and k == 0 and (e // bpm) % restart_interval == 0:
            pred = [0, 0, 0]
        comp = 0 if k < nl else k - nl + 1
        cls = "luma" if comp == 0 else "chroma"
        h[cls + "_dc"][category(blk[0] - pred[comp])] += 1
        pred[comp] = blk[0]
        ac = h[cls + "_ac"]
        run = 0
        for v in blk[1:]:
            if v == 0:
                run += 1
                continue
            while run >= 16:
                ac[0xF0] += 1
                run -= 16
            ac[(run << 4) | category(v)] += 1
            run = 0
        if blk[63] == 0:
            ac[0x00] += 1
    return h


def _length(syms) -> int:
    return sum(16 if s == ZRL else s[0] + 1 for s in syms)


def _check_hist(hist):
    out = {}
    for (r, s), c in hist.items():
        if not (0 <= r <= 15 and 0 <= s <= 15) or (s == 0 and r not in (0, 15)):
            raise ValueError(f"no such symbol: run {r}, size {s}")
        if (r, s) == (15, 15):
            raise ValueError("symbol 0xFF (run 15, size 15) is an error in the encoders")
        if c < 0 or int(c) != c:
            raise ValueError(f"count {c} of {(r, s)}")
        if c:
            out[(r, s)] = int(c)
    return out


def _exact_fill(cnt, target):
    """lengths summing to `target` out of the counts cnt[1..63], long ones first; None if there are none"""
    dead = set()

    def go(t, top):
        if t == 0:
            return []
        key = (t, top, cnt[top])  # (lengths above top are out of reach, those below untouched)
        if key in dead:
            return None
        for ln in range(min(t, top), 0, -1):
            if cnt[ln]:
                cnt[ln] -= 1
                rest = go(t - ln, ln)
                if rest is not None:
                    return [ln] + rest
                cnt[ln] += 1
        dead.add(key)
        return None

    return go(target, 63)


def _pack(hist, slots, pinned, rng, what):
    """The class's symbols in blocks: {emission index: [symbols in order]}.  slots: the
    class's emission indices; pinned: {emission index: [symbols]} taken out of hist first."""
    want = _check_hist(hist)
    eob = want.pop(EOB, None)
    out = {}
    for e, syms in pinned.items():
        syms = [tuple(s) for s in syms]
        if _length(syms) > 63 or (syms and syms[-1] == ZRL) or EOB in syms:
            raise ValueError(f"{what}: pinned block {e} does not fit a block")
        for s in syms:
            if want.get(s, 0) <= 0:
                raise ValueError(f"{what}: pinned block {e} takes {s}, which the histogram has no more of")
            want[s] -= 1
        out[e] = syms
    zrl = want.pop(ZRL, 0)
    units = [[s] for s, c in sorted(want.items()) for _ in range(c)]
    rng.shuffle(units)
    # ZRLs: 16 more zeros in front of a unit, dealt round the units while they fit
    while zrl:
        before = zrl
        for u in units:
            if zrl and _length(u) + 16 <= 63:
                u.insert(0, ZRL)
                zrl -= 1
        if zrl == before:
            raise ValueError(f"{what}: {zrl} ZRL without a symbol to stand in front of")
    by_len = {}
    for u in units:
        by_len.setdefault(_length(u), []).append(u)
    cnt = [0] * 64
    for ln, us in by_len.items():
        cnt[ln] = len(us)
    free = [e for e in slots if e not in out]
    bins = []
    n_open = len(free)
    if eob is not None:  # exactly eob blocks end with EOB: the others are filled to position 63
        n_open = eob - sum(1 for s in out.values() if _length(s) < 63)
        n_full = len(free) - n_open
        if n_open < 0 or n_full < 0:
            raise ValueError(f"{what}: {eob} EOB do not go with {len(slots)} blocks")
        for _ in range(n_full):
            lens = _exact_fill(cnt, 63)
            if lens is None:
                raise ValueError(f"{what}: no set of the remaining symbols fills a block to position 63")
            bins.append([by_len[ln].pop() for ln in lens])
    # the rest, longest first, each into the open block with the least room that takes it
    cap = 62 if eob is not None else 63
    room = [[] for _ in range(64)]  # room[r]: open blocks with r positions left
    opened = []
    for ln in range(63, 0, -1):
        for u in by_len.get(ln, []):
            r = next((r for r in range(ln, cap + 1) if room[r]), None)
            if r is None:
                if len(opened) == n_open:
                    raise ValueError(f"{what}: the symbols need more than {len(slots)} blocks")
                opened.append([])
                b, r = opened[-1], cap
            else:
                b = room[r].pop()
            b.append(u)
            room[r - ln].append(b)
    bins += opened + [[] for _ in range(n_open - len(opened))]
    order = rng.permutation(len(bins))
    for e, i in zip(free, order):
        b = bins[i]
        rng.shuffle(b)
        out[e] = [s for u in b for s in u]
    return out


class _Values:
    """values of a category: both ends with both signs first, then anything in between"""

    def __init__(self, rng):
        self.rng = rng
        self.used = [0] * 16

    def next(self, s: int) -> int:
        lo, hi = 1 << (s - 1), (1 << s) - 1
        k = self.used[s]
        self.used[s] += 1
        if k < 4:
            return (hi, -hi, lo, -lo)[k]
        v = int(self.rng.integers(lo, hi + 1))
        return v if self.rng.integers(2) else -v


def _dc_step(rng, pred: int, cat: int, nonzero: bool):
    """a difference of category cat that keeps the value within +-MAX_DC (and off 0 if
    nonzero); None if there is none"""
    if cat == 0:
        return None if nonzero and pred == 0 else 0
    lo, hi = 1 << (cat - 1), (1 << cat) - 1
    for sign in rng.permutation([1, -1]).tolist():
        a, b = lo, min(hi, MAX_DC - sign * pred)  # |d| in [a, b]: sign * pred + |d| <= MAX_DC
        if a > b:
            continue
        d = sign * int(rng.choice([a, b, int(rng.integers(a, b + 1))]))
        if nonzero and pred + d == 0:
            d = sign * (a if a != abs(d) else b)
            if pred + d == 0:
                continue
        return d
    return None


def _dc_values(spec, slots, sub, mcus, restart_interval, pins, rng, what):
    """{emission index: DC value} of one class.  spec: a list of differences, repeated
    over the class's blocks in emission order, or {category: count} over exactly the
    class's blocks, which are then ordered and signed here; pins: {emission index:
    category} out of that histogram."""
    _, nl, bpm = layout(sub)
    out = {}
    pred = {}
    pool = None
    if isinstance(spec, dict):
        if sum(spec.values()) != len(slots) or any(not 0 <= c <= 15 for c in spec):
            raise ValueError(f"{what}: the DC categories must count {len(slots)} blocks")
        pool = [c for c, k in sorted(spec.items()) for _ in range(k)]
        for c in pins.values():
            pool.remove(c)
        rng.shuffle(pool)
    elif pins:
        raise ValueError(f"{what}: DC pins go with a category histogram")
    nxt = {}  # the next block of the same component, where the predictor carries over
    last = {}
    for e in slots:
        m, k = divmod(e, bpm)
        comp = 0 if k < nl else k
        resets = restart_interval and m % restart_interval == 0 and (k == 0 or k >= nl)
        if comp in last and not resets:
            nxt[last[comp]] = e
        last[comp] = e
    for i, e in enumerate(slots):
        m, k = divmod(e, bpm)
        comp = 0 if k < nl else k
        if restart_interval and m % restart_interval == 0 and (k == 0 or k >= nl):
            pred[comp] = 0
        p = pred.get(comp, 0)
        if pool is None:
            d = int(spec[i % len(spec)])
            if category(d) > 15:
                raise ValueError(f"{what}: DC difference {d}")
        else:
            keep_off_zero = pins.get(nxt.get(e)) == 15  # a category-15 step cannot start from 0
            d = None
            if e in pins:
                d = _dc_step(rng, p, pins[e], keep_off_zero)
            else:
                for j, c in enumerate(pool):
                    d = _dc_step(rng, p, c, keep_off_zero)
                    if d is not None:
                        pool.pop(j)
                        break
            if d is None:
                raise ValueError(f"{what}: no DC difference of the wanted category fits block {e} (predictor {p})")
        if abs(p + d) > MAX_DC:
            raise ValueError(f"{what}: DC value {p + d} at block {e}")
        pred[comp] = out[e] = p + d
    return out


def build(width: int, height: int, sub: int, luma_ac, chroma_ac, luma_dc, chroma_dc, *, restart_interval: int = 0,
          pinned=None, dc_pinned=None, seed: int = 0):
    """Blocks of a width x height frame (sub 0: 4:4:4, 2: 4:2:0) with the wanted
    histograms, and the histograms they have: (int16[nblocks, 64], {name: int64[256]}
    for HIST_NAMES).

    luma_ac, chroma_ac   {(run, size): count}; (0, 0) (EOB) may be left out
    luma_dc, chroma_dc   a list of differences, repeated over the class's blocks in
                         emission order, or {category: count} over all of them
    pinned               {emission index: [(run, size), ...]}: that block holds exactly
                         these symbols of its class's histogram, in this order
    dc_pinned            {emission index: category}: that block's DC difference, out
                         of its class's category histogram
    Raises ValueError for a histogram the frame cannot hold."""
    mcus = geometry(width, height, sub)
    bpm = layout(sub)[2]
    rng = np.random.default_rng(seed)
    pinned, dc_pinned = dict(pinned or {}), dict(dc_pinned or {})
    if set(pinned) - set(range(mcus * bpm)) or set(dc_pinned) - set(range(mcus * bpm)):
        raise ValueError("a pinned block outside the frame")
    blocks = np.zeros((mcus * bpm, 64), np.int16)
    values = _Values(rng)
    for cls, ac, dc in (("luma", luma_ac, luma_dc), ("chroma", chroma_ac, chroma_dc)):
        slots = class_blocks(cls, mcus, sub)
        mine = set(slots)
        packed = _pack(ac, slots, {e: s for e, s in pinned.items() if e in mine}, rng, cls + " AC")
        dcs = _dc_values(dc, slots, sub, mcus, restart_interval, {e: c for e, c in dc_pinned.items() if e in mine},
                         rng, cls + " DC")
        for e in slots:
            blocks[e, 0] = dcs[e]
            pos = 1
            for r, s in packed[e]:
                if (r, s) == ZRL:
                    pos += 16
                    continue
                pos += r
                blocks[e, pos] = values.next(s)
                pos += 1
    hists = symbolise(blocks, sub, restart_interval)
    for cls, ac in (("luma", luma_ac), ("chroma", chroma_ac)):
        want = np.zeros(256, np.int64)
        for (r, s), c in ac.items():
            want[(r << 4) | s] = c
        got = hists[cls + "_ac"].copy()
        if EOB not in ac:
            got[0] = 0
        if not np.array_equal(got, want):
            raise AssertionError(f"{cls} AC: the blocks' histogram is not the wanted one")
    return blocks, hists
