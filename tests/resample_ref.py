"""numpy / Python-integer restatement of vvr_set_output_resampling as include/vvr.h defines it, written from that text and independent of the C code:
the numerators of the three filters in exact integers, the taps that are kept, the weights that sum to 16384, and the two integer passes.  Also
the same filters evaluated in float64 from the same numerators (no weight rounding, no rounding of the horizontal results), which is what the
integer pipeline is measured against and what equals torch's antialiased interpolate."""
from fractions import Fraction
from functools import lru_cache
from math import gcd

import numpy as np

REFERENCE, AREA, TRIANGLE, CUBIC = 0, 1, 2, 3
FILTERS = {"area": AREA, "triangle": TRIANGLE, "cubic": CUBIC}
MAX_TAPS = 256


def accepted(n, m):
    """the range of one axis of one plane"""
    return 1 <= n <= 8192 and 1 <= m <= 8192 and n <= 64 * m and m <= 8 * n


def numerators(filt, n, m, phi, i):
    """(first, [numerators]) of output sample i: the kept taps, Python integers"""
    g = gcd(n, m)
    n1, m1 = n // g, m // g
    S, Q = 4 * max(n1, m1), (4 * i + phi) * n1
    kept = []
    centre, reach = Q // (4 * m1), 2 * S // (4 * m1) + 3      # (every sample with N < 2 S lies within `reach` of `centre`: looked at one by one)
    for k in range(max(0, centre - reach), min(n, centre + reach + 1)):
        P = (4 * k + phi) * m1
        N = abs(P - Q)
        if filt == TRIANGLE:
            if N < S:
                kept.append((k, S - N))
        elif filt == CUBIC:
            if N < S:
                kept.append((k, 3 * N ** 3 - 5 * N * N * S + 2 * S ** 3))
            elif N < 2 * S:
                kept.append((k, -N ** 3 + 5 * N * N * S - 8 * N * S * S + 4 * S ** 3))
        else:
            lo, hi = Q - 2 * n1, Q + 2 * n1
            a = lo if k == 0 else max(lo, P - 2 * m1)
            b = hi if k == n - 1 else min(hi, P + 2 * m1)
            if b > a:
                kept.append((k, b - a))
    ks = [k for k, _ in kept]
    assert ks == list(range(ks[0], ks[0] + len(ks))), "the taps are not one run"
    if filt == AREA:
        assert sum(v for _, v in kept) == 4 * n1
    return ks[0], [v for _, v in kept]


@lru_cache(maxsize=None)
def taps(filt, n, m, phi, i):
    """(first, (weights)) of output sample i: the weights of the definition, integers that sum to 16384"""
    first, num = numerators(filt, n, m, phi, i)
    T = sum(num)
    assert T > 0
    w = [(2 * v * 16384 + T) // (2 * T) for v in num]      # (Python's // floors towards minus infinity)
    w[w.index(max(w))] += 16384 - sum(w)                    # (index: the lowest k among equals)
    return first, tuple(w)


def matrix(filt, n, m, phi, exact=False):
    """the m x n matrix of an axis: int64 weights, or with exact=True the float64 value of numerator / T"""
    M = np.zeros((m, n), np.float64 if exact else np.int64)
    for i in range(m):
        if exact:
            first, num = numerators(filt, n, m, phi, i)
            T = sum(num)
            M[i, first:first + len(num)] = [float(Fraction(v, T)) for v in num]
        else:
            first, w = taps(filt, n, m, phi, i)
            M[i, first:first + len(w)] = w
    return M


def horizontal(plane, filt, out_w, phi=2):
    """H of the definition: four fractional bits, not clipped"""
    s = np.asarray(plane).astype(np.int64)
    H = (s @ matrix(filt, s.shape[1], out_w, phi).T + 512) >> 10
    return H


def resample_plane(plane, filt, out_w, out_h, bd, phi=(2, 2)):
    """one plane: horizontally, then vertically, as the definition's two integer passes"""
    s = np.asarray(plane).astype(np.int64)
    H = horizontal(s, filt, out_w, phi[0])
    assert np.abs(s @ matrix(filt, s.shape[1], out_w, phi[0]).T).max() < 2 ** 31
    V = matrix(filt, s.shape[0], out_h, phi[1]) @ H
    assert np.abs(V).max() < 2 ** 31 - 131072
    return np.clip((V + 131072) >> 18, 0, (1 << bd) - 1).astype(np.uint16 if bd > 8 else np.uint8)


def resample(planes, filt, size, bd, col=(True, False)):
    """a 4:2:0 (or 4:0:0) frame to size = (out_w, out_h) luma samples; chroma sizes >> 1; col: the request's `collocated` as (horizontally, vertically)"""
    out = []
    for c, p in enumerate(planes):
        sh = 1 if c else 0
        phi = (1 if c and col[0] else 2, 1 if c and col[1] else 2)
        ow, oh = size[0] >> sh, size[1] >> sh
        p = np.asarray(p)
        out.append(p.astype(np.uint16 if bd > 8 else np.uint8) if (oh, ow) == p.shape else resample_plane(p, filt, ow, oh, bd, phi))
    return out


def resample_exact(plane, filt, out_w, out_h, phi=(2, 2)):
    """the same filter in float64 from the same numerators, neither weights nor intermediate results rounded, not clipped"""
    s = np.asarray(plane).astype(np.float64)
    return matrix(filt, s.shape[0], out_h, phi[1], True) @ (s @ matrix(filt, s.shape[1], out_w, phi[0], True).T)
