"""The definition of an SSIM request (vvr_ssim_submit, include/vvr.h) restated in numpy, independently of the loops in the library: both sides
clamped to L = 2^bit_depth - 1, the five sums of every 8 x 8 window at a stride of 4 taken from summed-area tables, A1, B1, A2, B2 and the two
quotients in int64 (every intermediate is asserted to stay below 2^62), a division that truncates toward zero built from the floor division of
magnitudes, and the map: the smallest v over the windows of all components whose origin lies in a block of 64 x 64 luma samples, a chroma
origin ( i, j ) of a 4:2:0 picture counted in the block of ( 2 i, 2 j ).  window_values() is what the float64 textbook check looks at."""
import numpy as np

NONE = 0xffffffff
NO_WINDOW = 0x7fffffff
ONE = 1 << 24


def constants(bit_depth):
    top = (1 << bit_depth) - 1
    return top, (top * top * 4096 + 5000) // 10000, (9 * top * top * 4096 + 5000) // 10000


def trunc_div(a, b):
    """C's division on int64_t for b > 0: toward zero"""
    return np.sign(a) * (np.abs(a) // b)


def window_sums(a):
    """the sum of `a` (int64, 2-D) over every 8 x 8 window at a stride of 4 -> array of (windows_y, windows_x), possibly empty"""
    h, w = a.shape
    ny, nx = ((h - 8) // 4 + 1 if h >= 8 else 0), ((w - 8) // 4 + 1 if w >= 8 else 0)
    if not ny or not nx:
        return np.zeros((ny, nx), np.int64)
    table = np.zeros((h + 1, w + 1), np.int64)
    table[1:, 1:] = a.cumsum(axis=0).cumsum(axis=1)
    j, i = 4 * np.arange(ny)[:, None], 4 * np.arange(nx)[None, :]
    return table[j + 8, i + 8] - table[j, i + 8] - table[j + 8, i] + table[j, i]


def window_values(slot_plane, ref_plane, bit_depth):
    """v of every SSIM window of one component -> int64 array of (windows_y, windows_x)"""
    top, c1, c2 = constants(bit_depth)
    x = np.minimum(np.asarray(slot_plane).astype(np.int64), top)
    y = np.minimum(np.asarray(ref_plane).astype(np.int64), top)
    assert x.shape == y.shape
    s1, s2, sxx, syy, sxy = window_sums(x), window_sums(y), window_sums(x * x), window_sums(y * y), window_sums(x * y)
    n = 64
    a1, b1 = 2 * s1 * s2 + c1, s1 * s1 + s2 * s2 + c1
    a2, b2 = 2 * (n * sxy - s1 * s2) + c2, (n * sxx - s1 * s1) + (n * syy - s2 * s2) + c2
    if a1.size:
        assert (a1 > 0).all() and (a1 <= b1).all() and (np.abs(a2) <= b2).all() and int(a1.max()) << 24 < 1 << 58 and int(np.abs(a2).max()) << 24 < 1 << 58
    lum, con = trunc_div(a1 * ONE, b1), trunc_div(a2 * ONE, b2)
    return trunc_div(lum * con, ONE)


def ssim(slot_planes, ref_planes, bit_depth, with_map=True):
    """slot_planes, ref_planes: the window's planes, of equal shapes per component -> dict of per-component lists and the map"""
    nc = len(slot_planes)
    out = dict(num_components=nc, bit_depth=bit_depth, width=[], height=[], windows_x=[], windows_y=[], windows=[], sum=[], min=[], min_x=[], min_y=[])
    h0, w0 = slot_planes[0].shape
    blocks = np.full(((h0 + 63) // 64, (w0 + 63) // 64), NO_WINDOW, np.int64)
    for c in range(nc):
        v = window_values(slot_planes[c], ref_planes[c], bit_depth)
        h, w = slot_planes[c].shape
        out["width"].append(w)
        out["height"].append(h)
        out["windows_x"].append(v.shape[1] if v.size else (w - 8) // 4 + 1 if w >= 8 else 0)
        out["windows_y"].append(v.shape[0] if v.size else (h - 8) // 4 + 1 if h >= 8 else 0)
        out["windows"].append(int(v.size))
        if not v.size:
            out["sum"].append(0)
            out["min"].append(NO_WINDOW)
            out["min_x"].append(NONE)
            out["min_y"].append(NONE)
            continue
        out["sum"].append(sum(int(t) for t in v.ravel()))
        at = int(np.argmin(v.ravel()))            # (the first of equals)
        out["min"].append(int(v.ravel()[at]))
        out["min_x"].append(4 * (at % v.shape[1]))
        out["min_y"].append(4 * (at // v.shape[1]))
        per_block = 8 if c and nc == 3 else 16      # window origins per block and direction
        for by in range(blocks.shape[0]):
            for bx in range(blocks.shape[1]):
                inside = v[by * per_block:(by + 1) * per_block, bx * per_block:(bx + 1) * per_block]
                if inside.size:
                    blocks[by, bx] = min(int(blocks[by, bx]), int(inside.min()))
    for name in ("width", "height", "windows_x", "windows_y", "windows", "sum"):
        out[name] += [0] * (3 - nc)
    out["min"] += [NO_WINDOW] * (3 - nc)
    out["min_x"] += [NONE] * (3 - nc)
    out["min_y"] += [NONE] * (3 - nc)
    if with_map:
        out["map"] = blocks
    return out


def mean(want):
    """vvr_compare_ssim in doubles: [Y, Cb, Cr, all]; 0 for components without windows"""
    nc = want["num_components"]

    def m(total, windows):
        return float(total) / (float(windows) * 16777216.0) if windows else 0.
    return [m(want["sum"][c], want["windows"][c]) if c < nc else 0. for c in range(3)] + [m(float(sum(float(v) for v in want["sum"][:nc])), float(sum(want["windows"][:nc])))]


def textbook(slot_plane, ref_plane, bit_depth, k1=None, k2=None):
    """SSIM of every window in float64 from means and population variances (Wang et al., uniform 8 x 8 window); k1, k2: the stabilising
    constants, by default ( 0.01 L )^2 and ( 0.03 L )^2"""
    top = float((1 << bit_depth) - 1)
    x = np.minimum(np.asarray(slot_plane).astype(np.float64), top)
    y = np.minimum(np.asarray(ref_plane).astype(np.float64), top)
    ny, nx = (x.shape[0] - 8) // 4 + 1, (x.shape[1] - 8) // 4 + 1
    out = np.zeros((ny, nx))
    k1, k2 = (0.01 * top) ** 2 if k1 is None else k1, (0.03 * top) ** 2 if k2 is None else k2
    for j in range(ny):
        for i in range(nx):
            a, b = x[4 * j:4 * j + 8, 4 * i:4 * i + 8], y[4 * j:4 * j + 8, 4 * i:4 * i + 8]
            ma, mb = a.mean(), b.mean()
            va, vb, cov = ((a - ma) ** 2).mean(), ((b - mb) ** 2).mean(), ((a - ma) * (b - mb)).mean()
            out[j, i] = (2 * ma * mb + k1) * (2 * cov + k2) / ((ma * ma + mb * mb + k1) * (va + vb + k2))
    return out
