"""The quantiser's fast and exact paths on the GPU, at the inputs where they can part
(csrc/dct_quant.hpp: quantize_col8_scaled for integer samples and the YCbCr front,
quantize_col8 for Image<f32> dots).  Every comparison is bit for bit: the front half
through encoder.forward_blocks against oracle.forward / oracle.forward_dots and
np_ref, the paths without a stage entry (YCbCr frames, surfaces) as whole files
against the composed reference.

Random images do not reach the boundary (one coefficient in millions lies within
2^-20 of a half-integer quotient), so every input here is built for it on the CPU, by
a seeded search over the free quantisation table or by refining a block's amplitude
ulp by ulp, and every test first proves with tests/quant_census.py -- from the
reference alone -- that its input got there.  Those floors are conditions, not
results: an input that misses one is a broken test, whatever the GPU returns."""
import functools

import numpy as np
import pytest

import dmmt_jpeg
import oracle
import quant_census as qc
import ycc_ref
from dmmt_jpeg import PixelFormat as PF
from oracle import np_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
S = qc.sign_patterns()


def opts(sub, luma, chroma):
    return dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(sub), 8, luma_table=luma,
                                              chroma_table=chroma)


def seeded_table(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, 256, 64)]


def pick(hit, cap, across, fill):
    """indices of the blocks at the boundary (quant_census.boundary_blocks; at most cap)
    and at least as many that are not, `fill` blocks or more, a whole number of image rows"""
    hit = np.asarray(hit).astype(int)  # (2: next to a tie or in the band, taken first; 1: just outside; 0: neither)
    yes, no = np.argsort(-hit, kind="stable")[:min(cap, int((hit > 0).sum()))], np.nonzero(hit == 0)[0]
    n = max(2 * len(yes), fill)
    n += -n % across
    idx = np.concatenate([yes, no[:n - len(yes)]])
    assert len(idx) == n, "the pool has too few blocks off the boundary"
    return np.random.default_rng(len(yes)).permutation(idx)


# ------------------------------------------------------------------ 1. integer samples, RGB path

ACROSS = 40  # blocks per image row: 320 pixels, a full 256-column tile and a ragged one


@functools.lru_cache(None)
def integer_pool(kind, coloured):
    """(n, 8, 8, 3) integer sign-pattern blocks around mid-grey, an amplitude sweep per
    pattern: grey (Y carries the coefficients), or only R sweeping (Cb and Cr do)"""
    if kind == "u16":
        mid, amps, dt = 32768, np.linspace(40, 32700, 384 if coloured else 512).astype(np.int64), np.uint16
        amps = amps + (np.arange(amps.size) * 37) % 29
    else:
        mid, amps, dt = 128, np.arange(1, 128, dtype=np.int64), np.uint8
    g = mid + (amps[None, :, None, None] * S.astype(np.int64)[:, None, :, :])  # (64, amps, 8, 8)
    g = g.reshape(-1, 8, 8)
    rgb = np.repeat(g[..., None], 3, axis=3)
    if coloured:
        rgb[..., 1:] = mid
    return rgb.astype(dt)


def maxval_of(kind):
    return 65535 if kind == "u16" else 255


def dots_of(rgb, kind):
    return rgb.astype(np.float32) / f32(maxval_of(kind))


@functools.lru_cache(None)
def integer_image(kind, coloured):
    """the searched image and table: the pool's blocks one per 8x8 of a strip give the
    4:4:4 coefficients; the table is searched on Y (grey) or on Cb and Cr (coloured)"""
    pool = integer_pool(kind, coloured)
    y, cb, cr, _ = np_ref.forward_dct(dots_of(qc.tile_blocks(pool, pool.shape[0]), kind), 0)
    if coloured:
        table = qc.search_table(np.concatenate([cb, cr]))
        hit = np.maximum(qc.boundary_blocks(cb, table), qc.boundary_blocks(cr, table))
    else:
        table = qc.search_table(y)
        hit = qc.boundary_blocks(y, table)
    rgb = qc.tile_blocks(pool[pick(hit, 1024, ACROSS, 1600)], ACROSS)
    assert rgb.shape[0] <= 512 and rgb.shape[1] <= 512
    return rgb, table


def integer_census(rgb, kind, sub, luma, chroma):
    y, cb, cr, _ = np_ref.forward_dct(dots_of(rgb, kind), sub)
    return qc.census([(y, luma), (cb, chroma), (cr, chroma)])


# floors: (B, N, positions, E).  Those of the u16 4:4:4 luma case were set before any
# input existed; the others are half of what the reference census of the searched image
# gives (u16 grey: B 48, N 11, 51 positions, E 65 with every subsampling -- the chroma of
# a grey image quantises to 0; u16 coloured: 54, 6, 44, 38; u8 grey: 22, 20, 4, 49 -- 127
# amplitudes reach few positions; u8 coloured: 54, 17, 20, 0)
INTEGER_FLOORS = {
    ("u16", "grey", 0): (30, 10, 12, 30),
    ("u16", "grey", 1): (24, 5, 25, 32),
    ("u16", "grey", 2): (24, 5, 25, 32),
    ("u16", "coloured", 0): (27, 3, 22, 19),
    ("u8", "grey", 0): (11, 10, 2, 24),
    ("u8", "grey", 1): (11, 10, 2, 24),
    ("u8", "grey", 2): (11, 10, 2, 24),
    ("u8", "coloured", 0): (27, 8, 10, 0),
}


@pytest.mark.parametrize("kind,variant,sub", list(INTEGER_FLOORS), ids=lambda v: str(v))
def test_integer_samples_at_the_band(encoder, kind, variant, sub):
    coloured = variant == "coloured"
    rgb, table = integer_image(kind, coloured)
    other = seeded_table(5)
    luma, chroma = (other, table) if coloured else (table, other)  # sQ and sQ + 64: both halves of the LDS tables
    c = integer_census(rgb, kind, sub, luma, chroma)
    print(kind, variant, sub, rgb.shape, c)
    fB, fN, fP, fE = INTEGER_FLOORS[(kind, variant, sub)]
    assert c.B >= fB and c.N >= fN and c.positions >= fP and c.E >= fE, c
    mv = maxval_of(kind)
    want = oracle.forward(rgb, mv, sub, luma, chroma)
    assert np.array_equal(np_ref.forward(rgb, mv, sub, luma, chroma), want)
    got = encoder.forward_blocks(dmmt_jpeg.Image.from_array(rgb, mv), opts(sub, luma, chroma))
    assert got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:8].tolist())


# ------------------------------------------------------------------ 2. YCbCr path

@functools.lru_cache(None)
def ycc_search():
    """8192 seeded noise blocks as exact integers s - 128, the table searched on them,
    the blocks that hit and as many that do not"""
    pool = np.random.default_rng(2024).integers(0, 256, (8192, 8, 8), dtype=np.uint8)
    coefs = np_ref.dct_blocks(pool.astype(np.float32) - f32(128.0))
    table = qc.search_table(coefs)
    return pool[pick(qc.boundary_blocks(coefs, table), 1600, 2 * YACROSS, 3000)], table


YACROSS = 60  # 480 luma columns: a full tile and a ragged one (240 chroma columns with 4:2:0)


def ycc_planes(sub):
    """Y from the searched blocks; Cb and Cr from searched blocks too (other ones per plane)"""
    blocks, table = ycc_search()
    y = qc.tile_blocks(blocks, YACROSS)
    hr, vr = ycc_ref.rates(sub)
    n = blocks.shape[0] // (hr * vr)
    cb = qc.tile_blocks(blocks[::-1][:n], YACROSS // hr)
    cr = qc.tile_blocks(np.roll(blocks, 7, axis=0)[:n], YACROSS // hr)
    assert y.shape[0] <= 512 and y.shape[1] <= 512 and cb.shape == ycc_ref.chroma_shape(y.shape[1], y.shape[0], sub)
    return y, cb, cr, table


@pytest.mark.parametrize("layout", ["I444", "NV12"])
def test_ycc_frames_at_the_band(encoder, layout):
    sub = 0 if layout == "I444" else 2
    y, cb, cr, table = ycc_planes(sub)
    yc, cbc, crc, _ = ycc_ref.forward_dct(y, cb, cr, sub)
    c = qc.census([(yc, table), (cbc, table), (crc, table)])
    print(layout, y.shape, c)
    assert c.T >= 100 and c.N >= 400 and c.B >= 200 and c.positions >= 20 and c.E >= 50, c
    o = opts(sub, table, table)
    want = ycc_ref.encode(y, cb, cr, sub, table, table)
    if layout == "I444":
        got = encoder.encode_ycc(y, cb=cb, cr=cr, options=o)
    else:
        got = encoder.encode_ycc(y, uv=np.ascontiguousarray(np.stack([cb, cr], axis=2)), options=o)
    assert got == want


@pytest.mark.parametrize("q_dc", [16, 48, 240])
def test_ycc_constant_blocks_of_every_level(encoder, q_dc):
    """a constant block's DC is 64 (s - 128) S0^2, and the f32 S0^2 is 1/8 less 4.9e-7 of
    it: 4 to 10 ulps below 8 (s - 128).  With q_DC = 16 k the quotient is that far
    below (s - 128) / 2k, a tie at every level with s - 128 an odd multiple of k (128, 42
    and 8 of the 256): closer than |Q| 2^-19, inside the band the kernel must redo, and on
    the side where the reciprocal's own error decides the rounding"""
    levels = np.arange(256, dtype=np.uint8)
    y = qc.tile_blocks(np.broadcast_to(levels[:, None, None], (256, 8, 8)).copy(), 16)
    cb, cr = y[::-1].copy(), y[:, ::-1].copy()
    table = [q_dc] + seeded_table(q_dc)[1:]
    yc, cbc, crc, _ = ycc_ref.forward_dct(y, cb, cr, 0)
    a = np.abs(qc.quotients(yc, table)[:, 0]).astype(np.float64)
    delta = np.abs(a - np.floor(a) - 0.5)
    k = q_dc // 16
    ties = sum(1 for s in range(256) if (s - 128) % k == 0 and ((s - 128) // k) % 2)
    assert ties == {16: 128, 48: 42, 240: 8}[q_dc]
    near = delta <= a * 2.0 ** -19
    print(q_dc, "near", int(near.sum()), "exact", int((delta == 0).sum()))
    assert int(near.sum()) == ties and not (delta == 0).any()  # every one of them in the band, none a tie
    assert encoder.encode_ycc(y, cb=cb, cr=cr, options=opts(0, table, table)) == ycc_ref.encode(y, cb, cr, 0, table, table)


# ------------------------------------------------------------------ 3. f32 dots refined around ties

MAGNITUDES = [0.5, 1.5, 7.5, 100.5, 2047.5, 32766.5, 32767.5, 32768.5, 4194302.5, 4194303.5]
STEPS = np.arange(-16, 17)
POSITIONS_SUB = list(range(0, 60, 3))  # 20 positions: 660 chroma blocks of 16 x 16 pixels stay inside 512 x 512


def step_ulps(a, k):
    """float32 a moved by k ulps (a is far from 0: no sign change)"""
    a = np.asarray(a, np.float32)
    return (a.view(np.int32) + np.asarray(k, np.int32) * np.where(a < 0, -1, 1).astype(np.int32)).view(np.float32)


def blue_image(amps, positions, sub, across):
    """blocks whose blue dots are amps[i] * S[positions[i]] (R = G = 0: Cb = 127.5 b has
    no offset to absorb an ulp, unlike Y), each pattern sample covering hr x vr pixels so
    that one chroma block comes from one pattern"""
    hr, vr = ycc_ref.rates(sub)
    b = (np.asarray(amps, np.float32)[:, None, None] * S[np.asarray(positions)]).astype(np.float32)
    img = qc.tile_blocks(b, across)
    img = np.repeat(np.repeat(img, vr, axis=0), hr, axis=1)
    dots = np.zeros(img.shape + (3,), np.float32)
    dots[..., 2] = img
    return dots


@functools.lru_cache(None)
def refined(mag, sign, sub):
    """dots, chroma table, and the reference's Cb quotients of the targets as (positions, 33)"""
    positions = list(range(64)) if sub == 0 else POSITIONS_SUB
    chroma = seeded_table(int(mag) % 1000 + 3)
    unit = np_ref.dct_blocks(S)[np.arange(64), np.arange(64) // 8, np.arange(64) % 8]  # response of (u, v) to its pattern
    qp = np.asarray(chroma, np.float32)[positions]
    lin = (sign * mag * qp.astype(np.float64) / (127.5 * unit[positions].astype(np.float64))).astype(np.float32)
    window = np.arange(-48, 49)
    cand = step_ulps(lin[:, None], window[None, :])  # (positions, window)
    pos_rep = np.repeat(positions, window.size)

    def cb_quotients(amps, pos_list, across):
        _, cbc, _, _ = np_ref.forward_dct(blue_image(amps, pos_list, sub, across), sub)
        p = np.asarray(pos_list)
        return cbc[np.arange(len(p)), p // 8, p % 8] / np.asarray(chroma, np.float32)[p]

    Qc = cb_quotients(cand.reshape(-1), pos_rep, window.size).reshape(len(positions), window.size)
    best = np.argmin(np.abs(np.abs(Qc.astype(np.float64)) - mag), axis=1)
    a0 = cand[np.arange(len(positions)), best]
    amps = step_ulps(a0[:, None], STEPS[None, :]).reshape(-1)
    pos_rep = np.repeat(positions, STEPS.size)
    across = 48 if sub == 0 else 30
    dots = blue_image(amps, pos_rep, sub, across)
    assert dots.shape[0] <= 512 and dots.shape[1] <= 512, dots.shape
    return dots, chroma, cb_quotients(amps, pos_rep, across).reshape(len(positions), STEPS.size)


def assert_refined_census(Q, mag):
    """every target: a coefficient next to the tie (N or T), and the rounded quotient
    changes within the run of 33 -- taken before the i16 saturation, which hides the
    change at +32767.5 and beyond 32768"""
    T, N, _, _ = qc.classes(Q)
    assert (T | N).any(axis=1).all(), (mag, np.nonzero(~(T | N).any(axis=1))[0])
    r = np_ref.round_half_away(Q)
    assert (r.min(axis=1) != r.max(axis=1)).all(), (mag, np.nonzero(r.min(axis=1) == r.max(axis=1))[0])
    assert np.all(np.abs(np.abs(Q.astype(np.float64)) - mag) <= 40 * np.spacing(f32(mag)) + 1e-5), mag


def compare_forward_dots(encoder, dots, sub, luma, chroma):
    want = oracle.forward_dots(dots, sub, luma, chroma)
    assert np.array_equal(np_ref.forward_dots(dots, sub, luma, chroma), want)
    got = encoder.forward_blocks(dmmt_jpeg.Image.from_array(dots), opts(sub, luma, chroma))
    assert got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:8].tolist())
    return want


@pytest.mark.parametrize("sign", [1, -1], ids=["pos", "neg"])
@pytest.mark.parametrize("mag", MAGNITUDES)
def test_f32_dots_refined_around_ties(encoder, mag, sign):
    dots, chroma, Q = refined(mag, sign, 0)
    assert_refined_census(Q, mag)
    compare_forward_dots(encoder, dots, 0, seeded_table(8), chroma)


@pytest.mark.parametrize("mag,sign,sub", [(7.5, 1, 2), (2047.5, -1, 1)], ids=["420", "422"])
def test_f32_dots_refined_around_ties_subsampled(encoder, mag, sign, sub):
    dots, chroma, Q = refined(mag, sign, sub)
    assert_refined_census(Q, mag)
    compare_forward_dots(encoder, dots, sub, seeded_table(8), chroma)


def encode_f32_surface(enc, dots, fmt, options):
    """one frame of float32 dots as a device surface -> its JPEG file"""
    h, w, _ = dots.shape
    if fmt == PF.PLANAR:
        hosts, pitch = [np.ascontiguousarray(dots[:, :, c]) for c in range(3)], w * 4
    else:
        hosts, pitch = [np.ascontiguousarray(dots[:, :, ::-1] if fmt == PF.BGR else dots)], w * 12
    cap = dmmt_jpeg.max_jpeg_bytes(w, h, int(options.chroma_subsampling_preset))
    ptrs = []
    try:
        for hst in hosts:
            ptrs.append(enc.malloc(hst.nbytes))
            enc.h2d(ptrs[-1], hst)
        d_out, d_len = enc.malloc(cap), enc.malloc(4)
        ptrs += [d_out, d_len]
        planes = ptrs[:3] if fmt == PF.PLANAR else ptrs[0]
        enc.encode_device_surfaces(planes, fmt, pitch, 1, w, h, options, d_out, cap, d_len, maxval=255, sample_bytes=4)
        enc.synchronize()
        n = int(np.frombuffer(enc.d2h(d_len, 4), np.uint32)[0])
        return enc.d2h(d_out, min(n, cap))
    finally:
        for p in ptrs:
            enc.free(p)


@pytest.mark.parametrize("fmt", [PF.RGB, PF.BGR, PF.PLANAR], ids=lambda f: f.name)
def test_f32_surfaces_refined_around_ties(encoder, fmt):
    dots, chroma, Q = refined(100.5, 1, 0)
    assert_refined_census(Q, 100.5)
    luma = seeded_table(8)
    h, w, _ = dots.shape
    want = oracle.encode_coefficients(oracle.forward_dots(dots, 0, luma, chroma), w, h, 0, luma, chroma)
    assert encode_f32_surface(encoder, dots, fmt, opts(0, luma, chroma)) == want


# ------------------------------------------------------------------ 4. f32 dots: range and specials

DENORM_MIN = f32(1.401298464324817e-45)


@functools.lru_cache(None)
def special_blocks():
    """(names, (n, 8, 8, 3) float32): blocks whose coefficients cross the ends of i16,
    the 2^22 limit of the fast path and 2^31, and blocks with Inf, NaN, -0.0, denormal
    and +-3e38 dots"""
    rng = np.random.default_rng(41)
    names, blocks = [], []

    def add(name, b):
        names.append(name)
        blocks.append(np.asarray(b, np.float32))

    def pattern(p, amp, grey):
        b = np.zeros((8, 8, 3), np.float32)
        if grey:
            b[...] = (f32(amp) * S[p])[..., None]  # Y carries it
        else:
            b[..., 2] = f32(amp) * S[p]            # Cb (and Cr, Y) carry it
        return b

    for p in (0, 1, 9, 63):
        for grey in (False, True):
            for k in range(0, 160, 4):  # 2^0 .. 2^39: coefficients to 1e14
                for sgn in (1, -1):
                    add(f"sweep p{p} grey{int(grey)} 2^{k / 4:g} {sgn:+d}", pattern(p, sgn * 2.0 ** (k / 4), grey))
    unit = np_ref.dct_blocks(S)[np.arange(64), np.arange(64) // 8, np.arange(64) % 8]
    for th in (32766.5, 32767.5, 32768.5, 2.0 ** 22 - 0.5, 2.0 ** 22, 2.0 ** 22 + 0.5, 2.0 ** 31, 2.0 ** 32):
        for p in (0, 10, 63):
            for e in (-3e-7, 0.0, 3e-7):
                for sgn in (1, -1):  # quotient about th with q = 16: in Cb (blue) and in Y (grey)
                    add(f"near {th:g} p{p} {e:+g} {sgn:+d} blue", pattern(p, sgn * th * 16 / (127.5 * unit[p]) * (1 + e), False))
                    add(f"near {th:g} p{p} {e:+g} {sgn:+d} grey", pattern(p, sgn * th * 16 / (255.0 * unit[p]) * (1 + e), True))
    ordinary = lambda: rng.uniform(0.0, 1.0, (8, 8, 3)).astype(np.float32)
    for name, v in (("+Inf", np.inf), ("-Inf", -np.inf), ("NaN", np.nan), ("3e38", 3e38), ("-3e38", -3e38),
                    ("-0.0", -0.0), ("1e-40", 1e-40), ("denorm_min", DENORM_MIN)):
        for ch in range(3):
            b = ordinary()
            b[rng.integers(8), rng.integers(8), ch] = v
            add(f"one {name} in channel {ch}", b)
    add("all -0.0", np.full((8, 8, 3), -0.0, np.float32))
    add("all denormal", rng.integers(-1000, 1001, (8, 8, 3)).astype(np.float32) * DENORM_MIN)
    add("+-3e38", rng.choice(np.array([3e38, -3e38], np.float32), (8, 8, 3)))
    add("all 3e38", np.full((8, 8, 3), 3e38, np.float32))
    add("Inf and -Inf", np.where(rng.integers(0, 2, (8, 8, 3)) == 1, np.inf, -np.inf))
    add("negative and above 1", rng.uniform(-4.0, 4.0, (8, 8, 3)))
    return names, np.stack(blocks)


@functools.lru_cache(None)
def specials_image():
    """every special block with an ordinary block to its right: the two share a tile,
    8-lane column groups of both sit in one wave, and with 4:2:x one chroma block"""
    _, sp = special_blocks()
    rng = np.random.default_rng(43)
    n = sp.shape[0]
    n += -n % (ACROSS // 2)
    both = rng.uniform(0.0, 1.0, (n, 2, 8, 8, 3)).astype(np.float32)
    both[:sp.shape[0], 0] = sp
    dots = qc.tile_blocks(both.reshape(-1, 8, 8, 3), ACROSS)
    assert dots.shape[0] <= 512 and dots.shape[1] <= 512, dots.shape
    return dots


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_f32_dots_range_and_specials(encoder, sub):
    dots = specials_image()
    luma, chroma = [16] * 64, ([16] * 64 if sub == 0 else seeded_table(22))  # (q = 16: special_blocks' "near" blocks)
    yc, cbc, crc, _ = np_ref.forward_dct(dots, sub)
    with np.errstate(all="ignore"):
        a = np.abs(np.concatenate([qc.quotients(yc, luma), qc.quotients(cbc, chroma), qc.quotients(crc, chroma)]))
    reach = {"NaN": int(np.isnan(a).sum()), "Inf": int(np.isinf(a).sum()),
             "i16 end .. 2^22": int(((a >= 32767.5) & (a < 2.0 ** 22)).sum()),
             "2^22 .. 2^31": int(((a >= 2.0 ** 22) & (a < 2.0 ** 31)).sum()),
             ">= 2^31, finite": int(((a >= 2.0 ** 31) & np.isfinite(a)).sum()),
             "denormal": int(((a > 0) & (a < 1.1754944e-38)).sum()),
             "just below the i16 end": int(((a >= 32000) & (a < 32767.5)).sum())}
    if sub != 0:  # (the denormal coefficients are Cb's and Cr's: averaged away with the ordinary neighbour)
        del reach["denormal"]
    print(sub, dots.shape, reach)
    assert all(v > 0 for v in reach.values()), reach
    want = compare_forward_dots(encoder, dots, sub, luma, chroma)
    assert (want == 32767).any() and (want == -32768).any()
    # the ordinary neighbours: the same as in an image without the special blocks, where no part of them is shared
    if sub == 0:
        plain = dots.copy()
        plain.reshape(-1, 8, ACROSS // 2, 2, 8, 3)[:, :, :, 0] = 0.5
        w2 = oracle.forward_dots(plain, 0, luma, chroma).reshape(-1, 2, 3, 64)
        assert np.array_equal(want.reshape(-1, 2, 3, 64)[:, 1], w2[:, 1])


def test_f32_whole_file_errors_exactly_where_the_reference_has_them(encoder):
    """the whole encode of a special block beside an ordinary one: the reference's file,
    or its CategoryOutOfRange (-101, categorize.rs:25-30: a coefficient or DC difference
    of -32768) -- on the same inputs"""
    names, sp = special_blocks()
    rng = np.random.default_rng(47)
    luma, chroma = seeded_table(31), seeded_table(32)
    take = [i for i, nm in enumerate(names) if not nm.startswith("sweep") or " p9 " in nm and "2^" in nm][::3]
    errors = files = 0
    for i in take:
        dots = np.concatenate([sp[i], rng.uniform(0.0, 1.0, (8, 8, 3)).astype(np.float32)], axis=1)
        for sub in (0, 2):
            try:
                want = oracle.encode_coefficients(oracle.forward_dots(dots, sub, luma, chroma), 16, 8, sub, luma, chroma)
            except oracle.OracleError as e:
                want = e.code
            try:
                got = encoder.encode(dmmt_jpeg.Image.from_array(dots), opts(sub, luma, chroma))
            except dmmt_jpeg.Error as e:
                got = e.code
            assert got == want, (names[i], sub, got if isinstance(got, int) else len(got))
            errors += isinstance(want, int)
            files += not isinstance(want, int)
            assert not isinstance(want, int) or want == -101, (names[i], want)
    print("errors", errors, "files", files)
    assert errors >= 10 and files >= 10


# ------------------------------------------------------------------ 5. the DCT operator

def test_dct_transform_specials_and_magnitudes(encoder):
    """dct_transform beyond uniform(-128, 127): magnitudes 1e-40 .. 1e38, zeros of both
    signs, denormals, Inf, NaN and overflow inside the butterfly, against
    oracle.dct_block; bit patterns, a NaN compared as a NaN"""
    rng = np.random.default_rng(53)
    blocks = []
    for lo, hi in ((-40, -36), (-40, 38), (30, 38), (-3, 3), (-45, -37)):
        for _ in range(12):
            mag = 10.0 ** rng.uniform(lo, hi, 64)
            blocks.append((rng.choice([-1.0, 1.0], 64) * mag).astype(np.float32))
    for k in range(0, 77, 4):  # one magnitude per block, 1e-40 .. 1e36
        blocks.append((rng.uniform(-1, 1, 64) * 10.0 ** (k - 40)).astype(np.float32))
    for v in (np.inf, -np.inf, np.nan, -0.0, 3e38, -3e38, 1e-40, DENORM_MIN):
        for _ in range(3):
            b = rng.uniform(-128, 127, 64).astype(np.float32)
            b[rng.integers(64)] = v
            blocks.append(b)
    blocks.append(np.full(64, -0.0, np.float32))
    blocks.append(np.zeros(64, np.float32))
    blocks.append(np.full(64, 3.4028234663852886e38, np.float32))
    blocks.append(rng.choice(np.array([3e38, -3e38], np.float32), 64))
    blocks.append(rng.integers(-64, 65, 64).astype(np.float32) * DENORM_MIN)
    blocks.append(rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32).view(np.float32))
    blocks = np.stack(blocks)
    want = np.stack([oracle.dct_block(b) for b in blocks])
    with np.errstate(all="ignore"):
        second = np_ref.dct_blocks(blocks.reshape(-1, 8, 8)).reshape(-1, 64)
    assert np.array_equal(np.isnan(second), np.isnan(want))
    assert np.array_equal(second.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    kinds = {"NaN": np.isnan(want).sum(), "Inf": np.isinf(want).sum(), "-0.0": ((want == 0) & np.signbit(want)).sum(),
             "denormal": ((want != 0) & (np.abs(want) < 1.1754944e-38)).sum(), "> 1e38": (np.abs(want) > 1e38).sum()}
    assert all(v > 0 for v in kinds.values()), kinds
    got = encoder.dct_transform(blocks.reshape(-1)).reshape(-1, 64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
