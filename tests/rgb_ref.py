"""numpy restatement of the RGB formats of the output queue (VVR_OUT_RGB8 / _RGB16 / _RGBF16) as include/vvr.h defines them, written from that
text and independent of the C code: chroma to the luma grid with the 4-tap chroma DCTIF at the two phases a direction has, the Q14 matrix, the
three sample types.  float_rgb gives the real-valued H.273 equations the integer matrix approximates."""
import numpy as np

# rows 0, 8, 16 and 24 of the chroma interpolation filter (H.266 table 33, 1/32 sample); test_output_rgb_host anchors the upsampler built from
# them to vvdec::rescalePlane
TAPS = {0: (0, 64, 0, 0), 8: (-4, 54, 16, -2), 16: (-4, 36, 36, -4), 24: (-2, 16, 54, -4)}
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}
DTYPES = {"rgb8": np.uint8, "rgb16": np.uint16, "rgbf16": np.float16}


def upsample_axis(a, axis, collocated):
    """twice the samples along `axis`: position i reads at 16 * i - (0 or 8) in 1/32 samples, taps clamped to the plane; sums, not normalised"""
    a = np.moveaxis(np.asarray(a, np.int64), axis, 0)
    n = a.shape[0]
    ref = 16 * np.arange(2 * n) - (0 if collocated else 8)
    integer, frac = ref >> 5, ref & 31
    out = np.zeros((2 * n,) + a.shape[1:], np.int64)
    for k in range(4):
        coef = np.array([TAPS[int(f)][k] for f in frac], np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        out += coef * a[np.clip(integer + k - 1, 0, n - 1)]
    return np.moveaxis(out, 0, axis)


def upsample(plane, bd, collocated):
    """a chroma plane at twice its size; collocated: (horizontal, vertical)"""
    sums = upsample_axis(upsample_axis(plane, 1, collocated[0]), 0, collocated[1])
    return np.clip((sums + 2048) >> 12, 0, (1 << bd) - 1)


def scales(full_range, bd, od):
    m, s = (1 << od) - 1, 1 << (bd - 8)
    if full_range:
        return m / ((1 << bd) - 1), m / ((1 << bd) - 1), 0, 1 << (bd - 1), m
    return m / (219 * s), m / (224 * s), 16 * s, 1 << (bd - 1), m


def coefficients(matrix, full_range, bd, od):
    """(cy, rv, gu, gv, bu) in Q14"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs, _, _, _ = scales(full_range, bd, od)
    q = lambda v: int(np.floor(v * 16384 + 0.5))
    return q(ys), q(2 * (1 - kr) * cs), -q(2 * kb * (1 - kb) / kg * cs), -q(2 * kr * (1 - kr) / kg * cs), q(2 * (1 - kb) * cs)


def matrix_int(y, cb, cr, matrix, full_range, bd, od):
    """integer R, G, B (int64 arrays) of samples on one grid, and the largest accumulator magnitude"""
    cy, rv, gu, gv, bu = coefficients(matrix, full_range, bd, od)
    _, _, yoff, coff, m = scales(full_range, bd, od)
    y, u, v = np.asarray(y, np.int64) - yoff, np.asarray(cb, np.int64) - coff, np.asarray(cr, np.int64) - coff
    acc = [cy * y + rv * v + 8192, cy * y + gu * u + gv * v + 8192, cy * y + bu * u + 8192]
    return [np.clip(a >> 14, 0, m) for a in acc], max(int(np.abs(a).max()) for a in acc)


def float_rgb(y, cb, cr, matrix, full_range, bd, od):
    """the real-valued equations of H.273 (unrounded), scaled to 0 .. 2^od - 1 and clipped there"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs, yoff, coff, m = scales(full_range, bd, od)
    ey, pb, pr = (np.asarray(y, np.float64) - yoff) * ys / m, (np.asarray(cb, np.float64) - coff) * cs / m, (np.asarray(cr, np.float64) - coff) * cs / m
    r, b = ey + 2 * (1 - kr) * pr, ey + 2 * (1 - kb) * pb
    g = (ey - kr * r - kb * b) / kg
    return [np.clip(c * m, 0, m) for c in (r, g, b)]


def rgb(planes, bd, fmt, matrix, full_range, collocated):
    """one 4:2:0 frame (Y, Cb, Cr; even luma sides) -> the three planes of `fmt` at the luma size"""
    y, cb, cr = planes
    od = 8 if fmt == "rgb8" else bd
    out, _ = matrix_int(y, upsample(cb, bd, collocated), upsample(cr, bd, collocated), matrix, full_range, bd, od)
    if fmt == "rgbf16":
        inv = np.float32(1) / np.float32((1 << bd) - 1)
        return [(c.astype(np.float32) * inv).astype(np.float16) for c in out]
    return [c.astype(DTYPES[fmt]) for c in out]
