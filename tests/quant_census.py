"""Where the quantiser's shortcuts can go wrong, counted from the reference alone --
TEST INFRASTRUCTURE for tests/test_gpu_quant_edges.py.

The front kernels quantise with a reciprocal and redo a lane with the division only
near a half-integer quotient (csrc/dct_quant.hpp).  Random images almost never get
there, so the tests build their inputs by a seeded search and prove with this census,
before they compare anything, that the input reaches the boundary.

For a coefficient d before quantisation (np_ref.forward_dct / ycc_ref.forward_dct)
and its step q:  Q = fl32(d / q), a = |Q| (counted only when a >= 1/4),
delta = |frac(a) - 1/2| in float64, beta = (a + 1) * 2^-20.  Classes:
  T  delta == 0                     an exact tie
  N  0 < delta <= 2 ulp(a)          next to a tie
  B  0 < delta <= 2^-20             inside the band: must take the exact path
  E  2 beta <= delta <= 16 beta     just outside it: on the fast path
(T is kept out of B so that a floor on B cannot be met by ties alone.)"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def quotients(coefs, table):
    """Q for (n, 8, 8) float32 coefficient blocks and a natural-order table of 64 steps"""
    with np.errstate(all="ignore"):
        return np.asarray(coefs, np.float32).reshape(-1, 64) / np.asarray(table, np.float32).reshape(1, 64)


def classes(Q):
    """boolean masks T, N, B, E (the shape of Q) of float32 quotients"""
    with np.errstate(all="ignore"):
        a32 = np.abs(Q.astype(np.float32))
        ok = np.isfinite(a32) & (a32 >= f32(0.25))
        a = np.where(ok, a32, f32(1.0)).astype(np.float64)
        delta = np.abs((a - np.floor(a)) - 0.5)
        ulp = np.spacing(np.where(ok, a32, f32(1.0))).astype(np.float64)
        beta = (a + 1.0) * 2.0 ** -20
    T = ok & (delta == 0)
    N = ok & (delta > 0) & (delta <= 2 * ulp)
    B = ok & (delta > 0) & (delta <= 2.0 ** -20)
    E = ok & (delta >= 2 * beta) & (delta <= 16 * beta)
    return T, N, B, E


class Census:
    def __init__(self):
        self.T = self.N = self.B = self.E = 0
        self.hit_positions = set()  # natural-order positions with a coefficient in N or B

    def add(self, coefs, table):
        """coefficients of one component with its table; returns the (n,) mask of blocks that hit N, B or T"""
        T, N, B, E = classes(quotients(coefs, table))
        self.T += int(T.sum())
        self.N += int(N.sum())
        self.B += int(B.sum())
        self.E += int(E.sum())
        self.hit_positions |= set(np.nonzero((N | B).any(axis=0))[0].tolist())
        return (T | N | B).any(axis=1)

    @property
    def positions(self):
        return len(self.hit_positions)

    def __repr__(self):
        return f"census(T={self.T}, N={self.N}, B={self.B}, E={self.E}, positions={self.positions})"


def census(components):
    """components: (coefficient blocks, table) pairs, e.g. luma with the luma table and Cb, Cr with the chroma table"""
    c = Census()
    for coefs, table in components:
        c.add(coefs, table)
    return c


def boundary_blocks(coefs, table):
    """(n,) per block: 2 with a coefficient in T, N or B, else 1 with one in E, else 0"""
    T, N, B, E = classes(quotients(coefs, table))
    return np.maximum(2 * (T | N | B).any(axis=1), E.any(axis=1).astype(int))


def search_table(coefs):
    """The table, per position the q in 3..255 that is no power of two and puts the
    most of these coefficients into N or B (the smallest such q)."""
    d = np.abs(np.asarray(coefs, np.float32).reshape(-1, 64))
    qs = np.arange(1, 256, dtype=np.float32)
    counts = np.zeros((64, 255), np.int64)
    # float32 throughout, in cache-sized pieces; N's 2 ulp(a) taken as a * 2^-22 (between 1 and 2 ulp):
    # this only ranks the candidates, the tests count with classes()
    for lo in range(0, d.shape[0], 64):
        a = d[lo:lo + 64, :, None] / qs
        fr = a - np.floor(a)
        np.subtract(fr, f32(0.5), out=fr)
        np.abs(fr, out=fr)
        near = fr <= np.maximum(a * f32(2.0 ** -22), f32(2.0 ** -20))
        near &= a >= f32(0.25)
        counts += near.sum(axis=0)
    # not a power of two: there 1/q is exact, the reciprocal's product is the quotient
    # itself and the shortcut cannot err, however close to a tie (q = 1 would win
    # most positions: the largest quotients have the widest 2 ulp)
    counts[:, [0, 1, 3, 7, 15, 31, 63, 127]] = -1
    return [int(qs[k]) for k in np.argmax(counts, axis=1)]


def sign_patterns():
    """(64, 8, 8) of +-1: the signs of the 64 DCT basis functions, pattern 8 u + v for
    vertical frequency u and horizontal v -- the block that drives coefficient (u, v) hardest"""
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)  # [freq, x]
    s = np.where(c >= 0, 1.0, -1.0)
    return (s[:, None, :, None] * s[None, :, None, :]).reshape(64, 8, 8).astype(np.float32)


def tile_blocks(blocks, across):
    """(n, 8, 8[, c]) blocks -> an image `across` blocks wide, block raster order; n must fill the rows"""
    n = blocks.shape[0]
    assert n % across == 0, (n, across)
    rest = blocks.shape[3:]
    return blocks.reshape((n // across, across, 8, 8) + rest).swapaxes(1, 2).reshape((n // across * 8, across * 8) + rest)
