"""numpy restatement of the interleaved RGB formats of the output queue (VVR_OUT_RGBA8 / _BGRA8 / _RGB24 / _BGR24 / _RGB10A2 / _RGBA16F) and of
VVR_OUT_RGBF32 with its normalisation (vvr_set_output_normalisation), written from the text of include/vvr.h and independent of the C code.  The
arithmetic above the store is that of tests/rgb_ref.py (chroma to the luma grid, the Q14 matrix) and tests/colour_transform_ref.py (the three
stages); here are the output depth of RGB10A2, the 16 -> 10 bit reduction, the seven byte layouts and the two float32 roundings."""
import numpy as np

import colour_transform_ref as X
import rgb_ref

CODES = {"rgbf32": 36, "rgba8": 48, "bgra8": 49, "rgb24": 50, "bgr24": 51, "rgb10a2": 52, "rgba16f": 53}
FORMATS = list(CODES)
EIGHT = ("rgba8", "bgra8", "rgb24", "bgr24")      # the values VVR_OUT_RGB8 stores


def base(planes, bd, matrix, full_range, collocated, transform=None):
    """what every format of one frame shares: the chroma planes on the luma grid, and under a transform the three stage-3 values"""
    y, cb, cr = planes
    b = {"y": y, "cb": rgb_ref.upsample(cb, bd, collocated), "cr": rgb_ref.upsample(cr, bd, collocated), "bd": bd, "colour": (matrix, full_range), "e": None}
    if transform is not None:
        at_bd, _ = rgb_ref.matrix_int(y, b["cb"], b["cr"], matrix, full_range, bd, bd)
        b["e"] = X.stages(at_bd, *transform)
    return b


def values(b, fmt):
    """(R, G, B as int64 arrays, M): the integers the store of `fmt` starts from and, for the float formats, their full scale"""
    bd = b["bd"]
    if b["e"] is None:
        od = 8 if fmt in EIGHT else 10 if fmt == "rgb10a2" else bd
        return rgb_ref.matrix_int(b["y"], b["cb"], b["cr"], b["colour"][0], b["colour"][1], bd, od)[0], (1 << bd) - 1
    if fmt in EIGHT:
        return [(e + 128) // 257 for e in b["e"]], 65535
    if fmt == "rgb10a2":
        return [(e * 1023 + 32767) // 65535 for e in b["e"]], 65535      # correctly rounded: 65535 is odd, no ties
    return b["e"], 65535


def scale_bias(M, norm):
    """float32 scale and bias per channel, derived in float64 and rounded once; norm: None or (mean, std), three float32 values each"""
    if norm is None:
        return [np.float32(1.0 / M)] * 3, [np.float32(0)] * 3
    mean, std = [[float(np.float32(v)) for v in a] for a in norm]
    return [np.float32(1.0 / (float(M) * std[c])) for c in range(3)], [np.float32(-mean[c] / std[c]) for c in range(3)]


def pack(rgb, M, fmt, norm=None):
    """the planes of `fmt` as abi.output_plane_shapes shapes them"""
    r, g, b = [np.asarray(c, np.int64) for c in rgb]
    h, w = r.shape
    if fmt == "rgbf32":
        scale, bias = scale_bias(M, norm)
        out = []
        for c, v in enumerate((r, g, b)):
            t = v.astype(np.float32) * scale[c]          # one float32 multiply ...
            assert t.dtype == np.float32
            out.append(t + bias[c])                      # ... one float32 add
            assert out[-1].dtype == np.float32
        return out
    if fmt == "rgb10a2":
        return [(r | g << 10 | b << 20 | 3 << 30).astype(np.uint32)]
    if fmt == "rgba16f":
        inv = np.float32(1) / np.float32(M)
        px = np.empty((h, w, 4), np.uint16)
        for k, v in enumerate((r, g, b)):
            px[:, :, k] = (v.astype(np.float32) * inv).astype(np.float16).view(np.uint16)
        px[:, :, 3] = 0x3C00
        return [px.reshape(h, w * 4).view(np.float16)]
    order = (b, g, r) if fmt in ("bgra8", "bgr24") else (r, g, b)
    n = 4 if fmt in ("rgba8", "bgra8") else 3
    px = np.full((h, w, n), 255, np.uint8)
    for k, v in enumerate(order):
        px[:, :, k] = v
    return [px.reshape(h, w * n)]


def frame(planes, bd, fmt, matrix, full_range, collocated, transform=None, norm=None):
    """one 4:2:0 frame (Y, Cb, Cr; even luma sides) -> the planes of `fmt`"""
    rgb, M = values(base(planes, bd, matrix, full_range, collocated, transform), fmt)
    return pack(rgb, M, fmt, norm)
