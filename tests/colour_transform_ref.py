"""numpy restatement of the colour transform of the output queue (vvr_set_output_transform, include/vvr.h): the three integer stages - 1-D table,
Q14 3x3 matrix in int64, 1-D table with linear interpolation - and the three stores, written from the header's text and independent of the C code;
and the tables of vvr_output_transform_preset in float64, written from the standards: SMPTE ST 2084 / BT.2100 table 4 (PQ), BT.2100 table 5
(HLG), BT.2390 section 5.4.1 (EETF), BT.709 and BT.2020 (primaries, D65), IEC 61966-2-1 (sRGB) and BT.709 item 1.2 (OETF)."""
import numpy as np

import rgb_ref

TO_SRGB, TO_BT709, TO_LINEAR = 0, 1, 2
DTYPES = rgb_ref.DTYPES


# ---- the integer pipeline

def identity(bd=10):
    """the transform that leaves RGB16 as it is: lin[v] = v, the unit matrix, enc[i] = min( 64 i, 65535 )"""
    return np.arange(1024, dtype=np.uint16), 16384 * np.eye(3, dtype=np.int64), np.minimum(64 * np.arange(1025), 65535).astype(np.uint16)


def stages(rgb, lin, m, enc):
    """R'G'B' at od = bd (three integer arrays) -> the three stage-3 values, 0 .. 65535, as int64 arrays"""
    lin, enc, m = np.asarray(lin, np.int64), np.asarray(enc, np.int64), np.asarray(m, np.int64)
    L = [lin[np.asarray(c, np.int64)] for c in rgb]
    out = []
    for k in range(3):
        t = np.clip((m[k][0] * L[0] + m[k][1] * L[1] + m[k][2] * L[2] + 8192) >> 14, 0, 65535)
        i, f = t >> 6, t & 63
        out.append((enc[i] * (64 - f) + enc[i + 1] * f + 32) >> 6)
    return out


def store(e, fmt):
    """the stage-3 value as the format stores it"""
    if fmt == "rgb8":
        return ((e + 128) // 257).astype(np.uint8)
    if fmt == "rgb16":
        return e.astype(np.uint16)
    inv = np.float32(1) / np.float32(65535)
    return (e.astype(np.float32) * inv).astype(np.float16)


def rgb(planes, bd, fmt, matrix, full_range, collocated, transform):
    """one 4:2:0 frame -> the three planes of `fmt` under `transform` = (lin, m, enc): the Y'CbCr matrix runs at od = bd whatever the format"""
    y, cb, cr = planes
    base, _ = rgb_ref.matrix_int(y, rgb_ref.upsample(cb, bd, collocated), rgb_ref.upsample(cr, bd, collocated), matrix, full_range, bd, bd)
    return [store(e, fmt) for e in stages(base, *transform)]


def random_transform(rng, bd=10):
    """seeded random tables and a matrix with negative entries, some of them at the limits"""
    lin = rng.integers(0, 65536, 1024).astype(np.uint16)
    enc = rng.integers(0, 65536, 1025).astype(np.uint16)
    m = rng.integers(-40000, 40001, (3, 3)).astype(np.int64)
    m[rng.integers(0, 3), rng.integers(0, 3)] = 65536
    m[rng.integers(0, 3), rng.integers(0, 3)] = -65536
    return lin, m, enc


# ---- the preset, float64

M1, M2 = 2610 / 16384, 2523 / 4096 * 128
C1, C2, C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
HLG_A = 0.17883277
HLG_B = 1 - 4 * HLG_A
HLG_C = 0.5 - HLG_A * np.log(4 * HLG_A)
PRIMARIES = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)), 9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))}
D65 = (0.3127, 0.3290)


def pq_eotf(e):
    """non-linear value 0 .. 1 -> cd/m2"""
    p = np.power(np.asarray(e, np.float64), 1 / M2)
    return 10000 * np.power(np.maximum(p - C1, 0) / (C2 - C3 * p), 1 / M1)


def pq_inverse_eotf(nits):
    y = np.power(np.asarray(nits, np.float64) / 10000, M1)
    return np.power((C1 + C2 * y) / (1 + C3 * y), M2)


def eetf(e, src_peak, dst_peak):
    """BT.2390 5.4.1 on PQ values, mastering black and target black 0"""
    e = np.asarray(e, np.float64)
    lo, hi = pq_inverse_eotf(0.), pq_inverse_eotf(src_peak)
    e1 = np.clip((e - lo) / (hi - lo), 0, 1)
    max_lum = (pq_inverse_eotf(dst_peak) - lo) / (hi - lo)
    ks = 1.5 * max_lum - 0.5
    if ks < 1:
        t = np.maximum(e1 - ks, 0) / (1 - ks)
        p = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
        e2 = np.where(e1 < ks, e1, p)
    else:
        e2 = e1
    return e2 * (hi - lo) + lo


def hlg_inverse_oetf(e):
    e = np.asarray(e, np.float64)
    return np.where(e <= 0.5, e * e / 3, (np.exp((np.maximum(e, 0.5) - HLG_C) / HLG_A) + HLG_B) / 12)


def linear_light(e, transfer, src_peak, dst_peak):
    """non-linear value 0 .. 1 -> stage-1 value 0 .. 1, unrounded"""
    if transfer == 16:
        return np.minimum(pq_eotf(eetf(e, src_peak, dst_peak)) / dst_peak, 1)
    assert transfer == 18
    return hlg_inverse_oetf(e)


def oetf(x, target):
    x = np.asarray(x, np.float64)
    if target == TO_SRGB:
        return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0031308), 1 / 2.4) - 0.055)
    if target == TO_BT709:
        return np.where(x < 0.018, 4.5 * x, 1.099 * np.power(np.maximum(x, 0.018), 0.45) - 0.099)
    assert target == TO_LINEAR
    return x


def rgb_to_xyz(primaries):
    """columns: X, Y, Z of the primaries, scaled so that R = G = B = 1 is D65 with Y = 1"""
    xyz = np.array([[x / y, 1., (1 - x - y) / y] for x, y in PRIMARIES[primaries]], np.float64).T
    white = np.array([D65[0] / D65[1], 1., (1 - D65[0] - D65[1]) / D65[1]], np.float64)
    return xyz * np.linalg.solve(xyz, white)


def gamut_matrix(primaries):
    """real-valued RGB to RGB matrix from the source primaries to BT.709's"""
    if primaries == 1:
        return np.eye(3)
    return np.linalg.solve(rgb_to_xyz(1), rgb_to_xyz(primaries))


def preset(transfer, primaries, target, src_peak=1000., dst_peak=100., bd=10):
    """(lin, m, enc) as vvr_output_transform_preset defines them, from float64"""
    top = (1 << bd) - 1
    lin = np.zeros(1024, np.int64)
    lin[:top + 1] = np.floor(linear_light(np.arange(top + 1) / top, transfer, src_peak, dst_peak) * 65535 + 0.5)
    m = np.floor(gamut_matrix(primaries) * 16384 + 0.5).astype(np.int64)
    enc = np.floor(oetf(np.minimum(64 * np.arange(1025), 65535) / 65535, target) * 65535 + 0.5).astype(np.int64)
    return lin, m, enc


def float_pipeline(rgb, bd, transfer, primaries, target, src_peak=1000., dst_peak=100.):
    """R'G'B' codes at bd bits -> the real-valued result 0 .. 1 per channel: EOTF with EETF (or the inverse HLG OETF), the real-valued matrix,
    the clip, the OETF"""
    top = (1 << bd) - 1
    L = np.stack([linear_light(np.asarray(c, np.float64) / top, transfer, src_peak, dst_peak) for c in rgb])
    t = np.clip(np.tensordot(gamut_matrix(primaries), L, axes=1), 0, 1)
    return [oetf(t[k], target) for k in range(3)]
