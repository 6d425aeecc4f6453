"""numpy restatement of the Y'CbCr formats at 4:4:4 and 4:2:2 of the output queue (VVR_OUT_YUV444P8 ... VVR_OUT_Y410) as include/vvr.h defines them,
written from that text and independent of the C code.  The 4:4:4 chroma planes are rgb_ref.upsample - the planes the RGB formats convert; the
4:2:2 chroma is the vertical 4-tap alone, ( sum + 32 ) >> 6, written here on its own; the stores are the table of vvr.h, v210 and y410 included."""
import numpy as np

import rgb_ref

FORMATS = ["yuv444p8", "yuv444p16", "yuv422p8", "yuv422p16", "uyvy", "yuy2", "y210", "v210", "y410"]
FULL = ("yuv444p8", "yuv444p16", "y410")                 # chroma at 4:4:4: both bits of `collocated` count
BYTES = ("yuv444p8", "yuv422p8", "uyvy", "yuy2")         # the sample as a byte: 8-bit contexts only
ONE_PLANE = ("uyvy", "yuy2", "y210", "v210", "y410")
# the chroma interpolation filter at the four phases 2:1 has (H.266 table 33, 1/32 sample)
TAPS = {0: (0, 64, 0, 0), 8: (-4, 54, 16, -2), 16: (-4, 36, 36, -4), 24: (-2, 16, 54, -4)}


def formats(bd):
    """the formats a context of `bd` bits accepts"""
    return [f for f in FORMATS if bd == 8 or f not in BYTES]


def upsample_rows(plane, bd, collocated):
    """a chroma plane on every luma row, its columns as they are: row j reads at 16 * j - (0 or 8) in 1/32 rows, the four taps at
    integer - 1 .. integer + 2 clamped to the plane, ( sum + 32 ) >> 6, clipped"""
    a = np.asarray(plane, np.int64)
    n = a.shape[0]
    out = np.empty((2 * n, a.shape[1]), np.int64)
    for j in range(2 * n):
        ref = 16 * j - (0 if collocated else 8)
        integer, taps = ref >> 5, TAPS[ref & 31]
        acc = np.zeros(a.shape[1], np.int64)
        for k in range(4):
            acc += taps[k] * a[min(max(integer + k - 1, 0), n - 1)]
        out[j] = (acc + 32) >> 6
    return np.clip(out, 0, (1 << bd) - 1)


def chroma(planes, bd, fmt, collocated):
    """Cb', Cr' of `fmt`; collocated: (horizontal, vertical)"""
    if fmt in FULL:
        return [rgb_ref.upsample(planes[k], bd, collocated) for k in (1, 2)]
    return [upsample_rows(planes[k], bd, collocated[1]) for k in (1, 2)]


def yuv(planes, bd, fmt, collocated):
    """one 4:2:0 frame (Y, Cb, Cr; even luma sides) -> the planes of `fmt` as abi.output_plane_shapes lays them out"""
    y = np.asarray(planes[0], np.int64)
    u, v = chroma(planes, bd, fmt, collocated)
    h, w = y.shape
    if fmt in ("yuv444p8", "yuv422p8", "yuv444p16", "yuv422p16"):
        dt = np.uint8 if fmt in BYTES else np.uint16
        return [y.astype(dt), u.astype(dt), v.astype(dt)]
    if fmt == "y410":
        s = 10 - bd
        return [((u << s) | (y << s) << 10 | (v << s) << 20 | 3 << 30).astype(np.uint32)]
    if fmt in ("uyvy", "yuy2", "y210"):
        s = 16 - bd if fmt == "y210" else 0
        out = np.empty((h, 2 * w), np.int64)
        ye, yo = (0, 2) if fmt != "uyvy" else (1, 3)
        ce, co = (1, 3) if fmt != "uyvy" else (0, 2)
        out[:, ye::4], out[:, yo::4], out[:, ce::4], out[:, co::4] = y[:, 0::2] << s, y[:, 1::2] << s, u << s, v << s
        return [out.astype(np.uint16 if fmt == "y210" else np.uint8)]
    assert fmt == "v210"
    s, groups = 10 - bd, (w + 5) // 6
    Y, U, V = np.zeros((h, 6 * groups), np.int64), np.zeros((h, 3 * groups), np.int64), np.zeros((h, 3 * groups), np.int64)
    Y[:, :w], U[:, :w // 2], V[:, :w // 2] = y << s, u << s, v << s        # (the fields of pixels that do not exist are 0)
    Y, U, V = Y.reshape(h, groups, 6), U.reshape(h, groups, 3), V.reshape(h, groups, 3)
    d = [U[..., 0] | Y[..., 0] << 10 | V[..., 0] << 20, Y[..., 1] | U[..., 1] << 10 | Y[..., 2] << 20,
         V[..., 1] | Y[..., 3] << 10 | U[..., 2] << 20, Y[..., 4] | V[..., 2] << 10 | Y[..., 5] << 20]
    return [np.stack(d, axis=2).reshape(h, 4 * groups).astype(np.uint32)]
