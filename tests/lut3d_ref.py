"""numpy restatement of the 3-D LUT stage of the output queue (vvr_set_output_lut3d, include/vvr.h), written from the header's text and independent
of the C code: the widening of the matrix' values to 16 bits, the cell and the fractions, the sort, the four-vertex sum of the tetrahedral
interpolation, and the stores - those "under a transform" of tests/colour_transform_ref.py (planar) and tests/interleaved_ref.py (interleaved,
float32).  The arithmetic ahead of the stage is that of tests/rgb_ref.py (chroma to the luma grid, the Q14 matrix at od = bd) and, when a transform
precedes the LUT, the three stages of tests/colour_transform_ref.py.  And the nodes of vvr_output_lut3d_preset in float64, from the standards:
BT.2100 tables 4 and 5 with note 5f (the HLG OOTF and its system gamma), BT.2390 sections 5.4.1 and 6.2."""
import numpy as np

import colour_transform_ref as X
import interleaved_ref as IR
import rgb_ref

SIZES = (17, 33, 65)
PLANAR = ("rgb8", "rgb16", "rgbf16")


def shift(n):
    """s = 16 - log2( n - 1 )"""
    return {17: 12, 33: 11, 65: 10}[n]


def widen(v, bd):
    """0 .. 2^bd - 1 -> 0 .. 65535, correctly rounded"""
    M = (1 << bd) - 1
    return (np.asarray(v, np.int64) * 65535 + (M >> 1)) // M


def interpolate(rgb, n, nodes):
    """three int64 arrays of 16-bit values -> the three Ok; nodes: n^3 x 3 values in .cube order (R fastest)"""
    lut = np.asarray(nodes, np.int64).reshape(n, n, n, 3)      # [jb, jg, jr, k]
    s = shift(n)
    S = 1 << s
    v = np.stack([np.asarray(c, np.int64) for c in rgb], -1)
    shape = v.shape[:-1]
    v = v.reshape(-1, 3)
    i, f = v >> s, v & (S - 1)
    order = np.argsort(-f, axis=1, kind="stable")                # the axes of f1 >= f2 >= f3
    fs = np.take_along_axis(f, order, 1)
    rows = np.arange(len(v))
    vert = [i.copy()]
    for k in range(3):                                           # c1, c2, c3: one step more along the axis of f1, of f2, of f3
        nxt = vert[-1].copy()
        nxt[rows, order[:, k]] += 1
        vert.append(nxt)
    assert (vert[3] == i + 1).all() and int(vert[3].max()) <= n - 1
    w = [S - fs[:, 0], fs[:, 0] - fs[:, 1], fs[:, 1] - fs[:, 2], fs[:, 2]]
    acc = np.full((len(v), 3), S >> 1, np.int64)
    for c, wk in zip(vert, w):
        acc += lut[c[:, 2], c[:, 1], c[:, 0]] * wk[:, None]
    assert int(acc.max()) < 1 << 28
    out = acc >> s
    return [out[:, k].reshape(shape) for k in range(3)]


def base(planes, bd, matrix, full_range, collocated, n, nodes, transform=None):
    """what every format of one frame shares, as interleaved_ref.base gives it, with "e" the three Ok"""
    y, cb, cr = planes
    b = {"y": y, "cb": rgb_ref.upsample(cb, bd, collocated), "cr": rgb_ref.upsample(cr, bd, collocated), "bd": bd, "colour": (matrix, full_range)}
    at_bd, _ = rgb_ref.matrix_int(y, b["cb"], b["cr"], matrix, full_range, bd, bd)
    e = X.stages(at_bd, *transform) if transform is not None else [widen(c, bd) for c in at_bd]
    b["e"] = interpolate(e, n, nodes)
    return b


def frame(planes, bd, fmt, matrix, full_range, collocated, n, nodes, transform=None, norm=None):
    """one 4:2:0 frame -> the planes of `fmt` under the LUT (behind `transform` if there is one)"""
    b = base(planes, bd, matrix, full_range, collocated, n, nodes, transform)
    if fmt in PLANAR:
        return [X.store(e, fmt) for e in b["e"]]
    return IR.pack(*IR.values(b, fmt), fmt, norm)


def random_lut(rng, n):
    return rng.integers(0, 65536, 3 * n ** 3).astype(np.uint16)


def neighbours_differ(n):
    """a LUT whose six neighbours of a node all differ from it and from each other, per channel: steps along R, G, B weigh 1, 3 and 9 units"""
    jb, jg, jr = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    lut = np.stack([(1 * jr + 3 * jg + 9 * jb) * 61 + 7, (3 * jr + 9 * jg + 1 * jb) * 59 + 11, (9 * jr + 1 * jg + 3 * jb) * 53 + 13], -1)
    assert int(lut.max()) <= 65535
    return lut.astype(np.uint16).reshape(-1)


def parity(n):
    """0 / 65535 by the parity of jr + jg + jb"""
    jb, jg, jr = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.repeat((((jr + jg + jb) & 1) * 65535).astype(np.uint16).reshape(-1), 3)


# ---- the preset, float64

def hlg_gamma(lw):
    """BT.2100 note 5f inside 400 .. 2000 cd/m2, BT.2390 section 6.2 outside"""
    return 1.2 + 0.42 * np.log10(lw / 1000) if 400 <= lw <= 2000 else 1.2 * 1.111 ** np.log2(lw / 1000)


def preset(n, transfer, primaries, target, src_peak=1000., dst_peak=100.):
    """the nodes of vvr_output_lut3d_preset as int64, n^3 x 3 in .cube order"""
    S = 65536 // (n - 1)
    e = np.minimum(np.arange(n) * S, 65535) / 65535
    jb, jg, jr = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    w = X.rgb_to_xyz(primaries)[1]
    if transfer == 16:
        lin = X.pq_eotf(e)
        L = np.stack([lin[jr], lin[jg], lin[jb]])
        Y = np.tensordot(w, L, axes=1)
        safe = np.where(Y > 0, Y, 1.)
        L = L * np.where(Y > 0, X.pq_eotf(X.eetf(X.pq_inverse_eotf(safe), src_peak, dst_peak)) / safe, 1.) / dst_peak
    else:
        assert transfer == 18
        lin = X.hlg_inverse_oetf(e)
        L = np.stack([lin[jr], lin[jg], lin[jb]])
        Y = np.tensordot(w, L, axes=1)
        L = L * np.where(Y > 0, np.power(np.where(Y > 0, Y, 1.), hlg_gamma(dst_peak) - 1), 0.)
    t = np.clip(np.tensordot(X.gamut_matrix(primaries), L, axes=1), 0, 1)
    return np.floor(np.moveaxis(X.oetf(t, target), 0, -1) * 65535 + 0.5).astype(np.int64).reshape(-1)
