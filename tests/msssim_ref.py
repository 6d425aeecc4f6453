"""The definition of an MS-SSIM request (vvr_msssim_submit, include/vvr.h) restated in numpy, independently of the loops in the library: both
sides clamped to L = 2^bit_depth - 1 once, at level 0; every further level the rounded mean of 2 x 2 samples, a last odd column or row dropped;
per level the 8 x 8 windows at a stride of 4 of ssim_ref (summed-area tables, int64, a division that truncates toward zero) with l, c and v
kept apart; per level and component the number of windows, the sum of c and the sum of v.  value() is vvr_compare_msssim in float64;
textbook_terms() is what the float64 check looks at."""
import numpy as np

import ssim_ref

ONE = 1 << 24
MAX_SCALES = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def halve(a):
    """the next level of `a` (int64, 2-D): ( a + b + c + d + 2 ) >> 2 over 2 x 2 samples"""
    h, w = a.shape[0] >> 1, a.shape[1] >> 1
    a = a[:2 * h, :2 * w]
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2


def pyramid(plane, bit_depth, scales, clamp_first=True):
    """`scales` levels of one plane as int64 arrays.  clamp_first=False is NOT the definition: it averages what the plane holds and clamps every
    level afterwards (what the tests show to differ)"""
    top = (1 << bit_depth) - 1
    a = np.asarray(plane).astype(np.int64)
    if clamp_first:
        a = np.minimum(a, top)
    levels = [a]
    for _ in range(scales - 1):
        levels.append(halve(levels[-1]))
    return [np.minimum(v, top) for v in levels]


def window_terms(x, y, bit_depth):
    """l, c and v of every SSIM window of one level of one component (x, y: int64 planes within 0 .. L) -> three int64 arrays of (windows_y,
    windows_x)"""
    top, c1, c2 = ssim_ref.constants(bit_depth)
    assert x.shape == y.shape and (not x.size or (int(x.max()) <= top and int(y.max()) <= top and int(x.min()) >= 0 and int(y.min()) >= 0))
    s1, s2, sxx, syy, sxy = (ssim_ref.window_sums(t) for t in (x, y, x * x, y * y, x * y))
    n = 64
    a1, b1 = 2 * s1 * s2 + c1, s1 * s1 + s2 * s2 + c1
    a2, b2 = 2 * (n * sxy - s1 * s2) + c2, (n * sxx - s1 * s1) + (n * syy - s2 * s2) + c2
    if a1.size:
        assert (a1 > 0).all() and (a1 <= b1).all() and (np.abs(a2) <= b2).all() and int(a1.max()) << 24 < 1 << 58 and int(np.abs(a2).max()) << 24 < 1 << 58
    lum, con = ssim_ref.trunc_div(a1 * ONE, b1), ssim_ref.trunc_div(a2 * ONE, b2)
    return lum, con, ssim_ref.trunc_div(lum * con, ONE)


def msssim(slot_planes, ref_planes, bit_depth, scales, clamp_first=True):
    """slot_planes, ref_planes: the window's planes, of equal shapes per component -> dict: num_components, bit_depth, scales and, as lists
    [level][component] of MAX_SCALES x 3 entries (0 beyond the scales and the components), width, height, windows_x, windows_y, windows, sum_cs,
    sum_v"""
    nc = len(slot_planes)
    names = ("width", "height", "windows_x", "windows_y", "windows", "sum_cs", "sum_v")
    out = dict(num_components=nc, bit_depth=bit_depth, scales=scales, **{n: [[0] * 3 for _ in range(MAX_SCALES)] for n in names})
    for c in range(nc):
        xs, ys = pyramid(slot_planes[c], bit_depth, scales, clamp_first), pyramid(ref_planes[c], bit_depth, scales, clamp_first)
        for k in range(scales):
            h, w = xs[k].shape
            _, con, v = window_terms(xs[k], ys[k], bit_depth)
            out["width"][k][c], out["height"][k][c] = w, h
            out["windows_x"][k][c], out["windows_y"][k][c] = ((w - 8) // 4 + 1 if w >= 8 else 0), ((h - 8) // 4 + 1 if h >= 8 else 0)
            out["windows"][k][c] = out["windows_x"][k][c] * out["windows_y"][k][c]
            assert out["windows"][k][c] == v.size
            out["sum_cs"][k][c] = sum(int(t) for t in con.ravel())
            out["sum_v"][k][c] = sum(int(t) for t in v.ravel())
    return out


def weights_for(scales):
    total = 0.
    for k in range(scales):
        total += WEIGHTS[k]
    return [WEIGHTS[k] / total for k in range(scales)]


def value(want, weights=None):
    """vvr_compare_msssim in float64: [Y, Cb, Cr, all components together]; 0 for a component that does not exist or lacks windows at a level"""
    nc, scales = want["num_components"], want["scales"]
    wt = weights_for(scales) if weights is None else [float(v) for v in weights]
    out = []
    for c in range(4):
        comps = [c] if c < 3 else list(range(nc))
        if c < 3 and (c >= nc or any(want["windows"][k][c] == 0 for k in range(scales))):
            out.append(0.)
            continue
        product = np.float64(1.)
        for k in range(scales):
            name = "sum_cs" if k < scales - 1 else "sum_v"
            total, windows = np.float64(0.), np.float64(0.)
            for q in comps:
                total += np.float64(want[name][k][q])
                windows += np.float64(want["windows"][k][q])
            m = total / (windows * np.float64(16777216.0))
            product = product * np.power(max(m, np.float64(0.)), np.float64(wt[k]))
        out.append(float(product))
    return out


def textbook_terms(x, y, bit_depth, k1, k2):
    """the contrast-structure term and SSIM of every window in float64 from means and population variances (uniform 8 x 8 window) -> two arrays"""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    ny, nx = (x.shape[0] - 8) // 4 + 1, (x.shape[1] - 8) // 4 + 1
    cs, full = np.zeros((ny, nx)), np.zeros((ny, nx))
    for j in range(ny):
        for i in range(nx):
            a, b = x[4 * j:4 * j + 8, 4 * i:4 * i + 8], y[4 * j:4 * j + 8, 4 * i:4 * i + 8]
            ma, mb = a.mean(), b.mean()
            va, vb, cov = ((a - ma) ** 2).mean(), ((b - mb) ** 2).mean(), ((a - ma) * (b - mb)).mean()
            cs[j, i] = (2 * cov + k2) / (va + vb + k2)
            full[j, i] = (2 * ma * mb + k1) / (ma * ma + mb * mb + k1) * cs[j, i]
    return cs, full


def float_msssim(x, y, bit_depth, scales):
    """MS-SSIM of one plane in float64 on an UNROUNDED pyramid (2 x 2 means without rounding), ( 0.01 L )^2 and ( 0.03 L )^2, Wang's weights
    normalised: what the integers are an approximation of"""
    top = float((1 << bit_depth) - 1)
    a, b = np.minimum(np.asarray(x).astype(np.float64), top), np.minimum(np.asarray(y).astype(np.float64), top)
    wt, product = weights_for(scales), 1.
    for k in range(scales):
        cs, full = textbook_terms(a, b, bit_depth, (0.01 * top) ** 2, (0.03 * top) ** 2)
        product *= max(float((cs if k < scales - 1 else full).mean()), 0.) ** wt[k]
        h, w = a.shape[0] >> 1, a.shape[1] >> 1
        a = (a[0:2 * h:2, 0:2 * w:2] + a[0:2 * h:2, 1:2 * w:2] + a[1:2 * h:2, 0:2 * w:2] + a[1:2 * h:2, 1:2 * w:2]) / 4
        b = (b[0:2 * h:2, 0:2 * w:2] + b[0:2 * h:2, 1:2 * w:2] + b[1:2 * h:2, 0:2 * w:2] + b[1:2 * h:2, 1:2 * w:2]) / 4
    return product
