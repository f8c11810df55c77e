"""The two restatements on Image<f32> dots (oracle.forward_dots: cpu_ref.c,
np_ref.forward_dots: numpy) agree bit for bit on any float: normalised integers
(where both equal today's `forward`), dots outside [0, 1], dots that overflow inside
the colour conversion or the DCT (Inf - Inf = NaN quantises to 0, quantizer.rs:60
with Rust's saturating cast), Inf and NaN dots, -0.0 and denormals; the three
subsamplings at ragged sizes."""
import numpy as np
import pytest

import oracle
from oracle import np_ref

SIZES = [(9, 13), (33, 17)]  # (height, width)
FLT_DENORM_MIN = np.float32(1.401298464324817e-45)


def tables(seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(1, 256, 64)], [int(v) for v in rng.integers(1, 256, 64)]


def dots_cases(h, w, seed):
    rng = np.random.default_rng(seed)
    n = h * w * 3
    out = {}
    out["range4"] = rng.uniform(-4.0, 4.0, (h, w, 3)).astype(np.float32)
    # 3e38 * 0.299 is finite, the sums and `* 255` overflow: Inf in the planes, Inf - Inf in the DCT
    out["huge"] = rng.choice(np.array([3e38, -3e38, 0.5, 0.0], np.float32), (h, w, 3))
    # magnitudes whose coefficients cross the i16 range and 2^22 without overflowing
    out["large"] = (rng.uniform(-1.0, 1.0, (h, w, 3)) * 10.0 ** rng.uniform(0, 6, (h, w, 3))).astype(np.float32)
    sp = rng.uniform(0.0, 1.0, n).astype(np.float32)
    idx = rng.permutation(n)
    for k, v in enumerate([np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]):
        sp[idx[k]] = v
    out["specials"] = sp.reshape(h, w, 3)
    # one special alone in an otherwise ordinary image, each kind in its own block
    for name, v in (("one_pinf", np.inf), ("one_ninf", -np.inf), ("one_nan", np.nan)):
        a = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
        a[h // 2, w // 2, 1] = v
        out[name] = a
    tiny = rng.integers(-64, 65, (h, w, 3)).astype(np.float32) * FLT_DENORM_MIN
    tiny[::2, ::3] = np.float32(-0.0)
    out["denormal_and_negative_zero"] = tiny
    mixed = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    mixed[::3, ::2, 0] = np.float32(-0.0)
    mixed[1::3, ::2, 2] = np.float32(1e-40)
    out["ordinary_with_denormals"] = mixed
    return out


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("h,w", SIZES)
def test_normalised_integers_equal_forward(sub, h, w):
    rng = np.random.default_rng(100 + sub)
    lq, cq = tables(sub)
    for maxval, dt in ((255, np.uint8), (65535, np.uint16), (1023, np.uint16), (1, np.uint8)):
        rgb = rng.integers(0, maxval + 1, (h, w, 3)).astype(dt)
        dots = rgb.astype(np.float32) / np.float32(maxval)
        want = oracle.forward(rgb, maxval, sub, lq, cq)
        assert np.array_equal(oracle.forward_dots(dots, sub, lq, cq), want), maxval
        assert np.array_equal(np_ref.forward_dots(dots, sub, lq, cq), want), maxval
        assert np.array_equal(np_ref.forward(rgb, maxval, sub, lq, cq), want), maxval


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("h,w", SIZES)
def test_c_and_numpy_agree_on_any_float(sub, h, w):
    lq, cq = tables(10 + sub)
    flat1 = [1] * 64
    for name, dots in dots_cases(h, w, 1000 * sub + h).items():
        for tl, tc in ((lq, cq), (flat1, flat1)):
            a = oracle.forward_dots(dots, sub, tl, tc)
            b = np_ref.forward_dots(dots, sub, tl, tc)
            assert a.dtype == b.dtype == np.int16 and a.shape == b.shape
            assert np.array_equal(a, b), (name, int((a != b).sum()))


def test_the_special_inputs_reach_the_special_outputs():
    """so the agreement above is not between two all-zero arrays: saturation at both
    ends, NaN -> 0 next to Inf -> +-32767/8, denormals quantise to 0"""
    flat1 = [1] * 64
    c = dots_cases(33, 17, 5)
    big = oracle.forward_dots(c["large"], 0, flat1, flat1)
    assert big.max() == 32767 and big.min() == -32768
    # +-3e38 all over a block: +Inf and -Inf meet in every butterfly, every coefficient is NaN -> 0
    assert not oracle.forward_dots(c["huge"], 0, flat1, flat1)[0].any()
    # one +Inf (green): Y's DC is +Inf -> 32767, Cb's and Cr's (negative weights) -Inf -> -32768
    for name, want in (("one_pinf", [32767, -32768, -32768]), ("one_ninf", [-32768, 32767, 32767])):
        inf = oracle.forward_dots(c[name], 0, flat1, flat1)
        assert list(inf[3 * 7:3 * 7 + 3, 0]) == want, name  # (MCU 7 holds pixel (16, 8))
    one = oracle.forward_dots(c["one_nan"], 0, flat1, flat1)
    clean = c["one_nan"].copy()
    clean[33 // 2, 17 // 2, 1] = 0.5
    ref = oracle.forward_dots(clean, 0, flat1, flat1)
    changed = np.unique(np.nonzero(one != ref)[0])
    blk = (33 // 2 // 8) * 3 + (17 // 2 // 8)  # 4:4:4: blocks Y, Cb, Cr of MCU `blk`
    assert set(changed) <= {3 * blk, 3 * blk + 1, 3 * blk + 2} and len(changed) == 3
    assert not one[[3 * blk, 3 * blk + 1, 3 * blk + 2]].any()  # a NaN dot: the block's coefficients are NaN -> 0
    assert not oracle.forward_dots(c["denormal_and_negative_zero"], 2, flat1, flat1)[:, 1:].any()


def test_forward_dct_is_the_unquantised_half_of_forward_dots():
    rng = np.random.default_rng(3)
    dots = rng.uniform(-4.0, 4.0, (33, 17, 3)).astype(np.float32)
    lq, cq = tables(4)
    for sub in (0, 1, 2):
        yc, cbc, crc, wp = np_ref.forward_dct(dots, sub)
        assert yc.dtype == np.float32 and yc.shape[1:] == (8, 8)
        q = np_ref.interleave(np_ref.quantize(yc, lq).reshape(-1, 64), np_ref.quantize(cbc, cq).reshape(-1, 64),
                              np_ref.quantize(crc, cq).reshape(-1, 64), sub, wp // 8)[:, np_ref.ZIGZAG]
        assert np.array_equal(q, oracle.forward_dots(dots, sub, lq, cq))
        # and block for block the C DCT operator
        assert np.array_equal(yc[0].reshape(64).view(np.uint32),
                              oracle.dct_block(_first_luma_block(dots)).view(np.uint32))


def _first_luma_block(dots):
    r, g, b = (dots[:8, :8, i] for i in range(3))
    return np_ref.rgb_to_ycbcr(r, g, b)[0]
