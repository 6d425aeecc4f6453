"""numpy restatement of vvr_set_output_narrowing as include/vvr.h defines it, written from that text and independent of the C code: the formula,
the 2 x 2 cell and the coordinates of a sample per format - nothing else.  The planes it reduces are those of the 16-bit sibling request
(planar16, yuv444p16, yuv422p16), every sample at its column and row in its own output plane; the semi-planar interleave is
test_output_semiplanar_host.semi, the byte order of uyvy / yuy2 the one of yuv_ref.yuv (checked against it at 8 bits by the tests)."""
import numpy as np

import test_output_semiplanar_host as S

REFUSE, TRUNCATE, ROUND, DITHER = 0, 1, 2, 3
M = np.array([[0, 2], [3, 1]], np.int64)
FORMATS = ["planar8", "nv12", "yuv444p8", "yuv422p8", "uyvy", "yuy2"]
SIBLING = {"planar8": "planar16", "nv12": "planar16", "yuv444p8": "yuv444p16", "yuv422p8": "yuv422p16", "uyvy": "yuv422p16", "yuy2": "yuv422p16"}
# every mode, and DITHER at every phase
MODES = [(TRUNCATE, 0), (ROUND, 0), (DITHER, 0), (DITHER, 1), (DITHER, 2), (DITHER, 3)]


def thresholds(shape, bd, mode, phase):
    """a of every sample of a plane of `shape`: ( i, j ) are the sample's column and row in that plane"""
    s = bd - 8
    assert s in (1, 2) and mode in (TRUNCATE, ROUND, DITHER) and 0 <= phase <= 3
    j, i = np.indices(shape)
    if mode == TRUNCATE:
        return np.zeros(shape, np.int64)
    if mode == ROUND:
        return np.full(shape, 1 << (s - 1), np.int64)
    return M[(j + (phase >> 1 & 1)) & 1, (i + (phase & 1)) & 1] >> (2 - s)


def reduce(plane, bd, mode, phase):
    """byte = min( 255, ( v + a ) >> s ), v as it lies"""
    v = np.asarray(plane).astype(np.int64)
    return np.minimum(255, (v + thresholds(v.shape, bd, mode, phase)) >> (bd - 8)).astype(np.uint8)


def pack422(y, u, v, fmt):
    """bytes Cb, Y0, Cr, Y1 (uyvy) or Y0, Cb, Y1, Cr (yuy2) per pixel pair"""
    h, w = y.shape
    out = np.empty((h, 2 * w), np.uint8)
    ye, yo, ce, co = (1, 3, 0, 2) if fmt == "uyvy" else (0, 2, 1, 3)
    out[:, ye::4], out[:, yo::4], out[:, ce::4], out[:, co::4] = y[:, 0::2], y[:, 1::2], u, v
    return [out]


def narrow(planes, bd, fmt, mode, phase):
    """the planes of the sibling request of `fmt` (SIBLING: Y, Cb, Cr of that format, or Y alone in 4:0:0) -> the planes of `fmt`.  Every plane is
    reduced on its own grid: the chroma of planar8 / nv12 at its 4:2:0 coordinates - so the Cb and the Cr of nv12's pair k in row j both at
    ( k, j ) - , the chroma of yuv444p8 at ( x, y ), of yuv422p8 / uyvy / yuy2 at ( k, y ) for pixel pair k."""
    b = [reduce(p, bd, mode, phase) for p in planes]
    if fmt == "nv12":
        return S.semi(b, "nv12", 8)
    if fmt in ("uyvy", "yuy2"):
        return pack422(b[0], b[1], b[2], fmt)
    return b
