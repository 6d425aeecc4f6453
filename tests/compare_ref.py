"""The definition of a comparison request (vvr_compare_submit, include/vvr.h) restated in numpy: d = slot sample - reference sample in int64, per
component the number of samples, of differing samples, the sums of d * d and of |d|, the largest |d|, the first differing sample in raster order
(np.argmax of the raveled mask), and the map: differing samples over all components per block of 64 x 64 luma samples, a chroma sample
( i, j ) of a 4:2:0 picture counted in the block of ( 2 i, 2 j ).  Python integers throughout: nothing here can overflow."""
import numpy as np

NONE = 0xffffffff


def window_planes(planes, win):
    """the window of a picture's planes (4:2:0 when there are three)"""
    x, y, w, h = win
    if len(planes) == 1:
        return [planes[0][y:y + h, x:x + w]]
    return [p[y >> s:(y + h) >> s, x >> s:(x + w) >> s] for p, s in zip(planes, (0, 1, 1))]


def compare(slot_planes, ref_planes, with_map=True):
    """slot_planes, ref_planes: the window's planes, of equal shapes per component -> dict of per-component lists and the map"""
    nc = len(slot_planes)
    out = dict(num_components=nc, width=[], height=[], samples=[], differing=[], sse=[], sad=[], max_abs=[], first_x=[], first_y=[])
    h0, w0 = slot_planes[0].shape
    blocks = np.zeros(((h0 + 63) // 64, (w0 + 63) // 64), np.int64)
    for c in range(nc):
        a, b = np.asarray(slot_planes[c]).astype(np.int64), np.asarray(ref_planes[c]).astype(np.int64)
        assert a.shape == b.shape
        d = a - b
        mask = d != 0
        h, w = d.shape
        out["width"].append(w)
        out["height"].append(h)
        out["samples"].append(w * h)
        out["differing"].append(int(mask.sum()))
        out["sse"].append(sum(int(v) for v in (d * d).sum(axis=1)))      # (a row of 8192 samples: below 2^46 - rows added as Python integers)
        out["sad"].append(int(np.abs(d).sum()))
        out["max_abs"].append(int(np.abs(d).max()))
        if mask.any():
            at = int(np.argmax(mask.ravel()))
            out["first_x"].append(at % w)
            out["first_y"].append(at // w)
        else:
            out["first_x"].append(NONE)
            out["first_y"].append(NONE)
        side = 32 if c and nc == 3 else 64
        for by in range(blocks.shape[0]):
            for bx in range(blocks.shape[1]):
                blocks[by, bx] += int(mask[by * side:(by + 1) * side, bx * side:(bx + 1) * side].sum())
    for name in ("width", "height", "samples", "differing", "sse", "sad", "max_abs"):
        out[name] += [0] * (3 - nc)
    out["first_x"] += [NONE] * (3 - nc)
    out["first_y"] += [NONE] * (3 - nc)
    if with_map:
        out["map"] = blocks
    return out


def psnr(want, bit_depth, peak=0.):
    """vvr_compare_psnr in numpy doubles: [Y, Cb, Cr, all]; inf where the sse is 0, 0 for absent components"""
    peak = np.float64(peak if peak > 0 else (1 << bit_depth) - 1)
    nc = want["num_components"]

    def db(samples, sse):
        return np.inf if sse == 0 else float(np.float64(10.0) * np.log10(peak * peak * np.float64(samples) / np.float64(sse)))
    out = [db(want["samples"][c], want["sse"][c]) if c < nc else 0. for c in range(3)]
    # (the sums over the components in double, as the library forms them: exact below 2^53)
    return out + [db(float(sum(np.float64(v) for v in want["samples"][:nc])), float(sum(np.float64(v) for v in want["sse"][:nc])))]
