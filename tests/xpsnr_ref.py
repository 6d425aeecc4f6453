"""The definition of an XPSNR request (vvr_xpsnr_submit, include/vvr.h) restated in numpy, independently of the loops in the library: the
block size and filter a request resolves to, the high-pass value f and the temporal value t of every position as whole arrays built from
shifted slices (filter 2: of the plane of 2 x 2 sums taken at even origins), the positions sorted into blocks by their coordinates, per block
the sums of ( x - o )^2 of every component (a chroma sample ( i, j ) of a 4:2:0 picture counted in the block of ( 2 i, 2 j )), of |f|, of t and
the number of positions - all in int64, which holds every sum for 16-bit words - and vvr_compare_xpsnr in float64."""
import math

import numpy as np

BLOCK_DTYPE = np.dtype([("sse", "<u8", (3,)), ("act_spatial", "<u8"), ("act_temporal", "<u8"), ("count", "<u4"), ("pad", "<u4")])
MAX_BLOCKS = 16384

# filter 2: the weights of o( i - 2 + di, j - 2 + dj ), rows dj
WEIGHTS_2 = np.array([[0, -1, -1, -1, -1, 0],
                      [-1, -2, -3, -3, -2, -1],
                      [-1, -3, 12, 12, -3, -1],
                      [-1, -3, 12, 12, -3, -1],
                      [-1, -2, -3, -3, -2, -1],
                      [0, -1, -1, -1, -1, 0]], np.int64)


def resolve_block(w, h, block=0):
    return block if block else max(4, 4 * int(32.0 * math.sqrt(w * h / 8294400.0) + 0.5))


def resolve_filter(w, h, filter_=0):
    return filter_ if filter_ else (2 if w * h > 2048 * 1152 else 1)


def geometry(w, h, block=0):
    """-> B, blocks_x, blocks_y"""
    b = resolve_block(w, h, block)
    return b, (w + b - 1) // b, (h + b - 1) // b


def activity(ref_luma, prev, filter_):
    """|f| and t of every position -> (columns i, rows j, |f|, t) as flat int64 arrays; prev: the luma planes o1 (, o2)"""
    o = np.asarray(ref_luma).astype(np.int64)
    prev = [np.asarray(q).astype(np.int64) for q in prev]
    h, w = o.shape
    assert all(q.shape == o.shape for q in prev) and len(prev) <= 2
    if filter_ == 1:
        if w < 3 or h < 3:
            z = np.zeros(0, np.int64)
            return z, z, z, z
        c = o[1:-1, 1:-1]
        f = (12 * c - 2 * (o[1:-1, :-2] + o[1:-1, 2:] + o[:-2, 1:-1] + o[2:, 1:-1])
             - (o[:-2, :-2] + o[:-2, 2:] + o[2:, :-2] + o[2:, 2:]))
        if not prev:
            t = np.zeros_like(f)
        elif len(prev) == 1:
            t = np.abs(c - prev[0][1:-1, 1:-1])
        else:
            t = np.abs(c - 2 * prev[0][1:-1, 1:-1] + prev[1][1:-1, 1:-1])
        jj, ii = np.meshgrid(np.arange(1, h - 1), np.arange(1, w - 1), indexing="ij")
    else:
        ii = np.arange(2, w - 3, 2)      # even, 2 <= i <= w - 4
        jj = np.arange(2, h - 3, 2)
        if not len(ii) or not len(jj):
            z = np.zeros(0, np.int64)
            return z, z, z, z
        jj, ii = np.meshgrid(jj, ii, indexing="ij")
        f = np.zeros(ii.shape, np.int64)
        for dj in range(6):
            for di in range(6):
                if WEIGHTS_2[dj, di]:
                    f += WEIGHTS_2[dj, di] * o[jj - 2 + dj, ii - 2 + di]

        def s(a):
            return a[jj, ii] + a[jj, ii + 1] + a[jj + 1, ii] + a[jj + 1, ii + 1]
        if not prev:
            t = np.zeros_like(f)
        elif len(prev) == 1:
            t = np.abs(s(o) - s(prev[0]))
        else:
            t = np.abs(s(o) - 2 * s(prev[0]) + s(prev[1]))
    return ii.ravel(), jj.ravel(), np.abs(f).ravel(), t.ravel()


def xpsnr_integers(slot_planes, ref_planes, prev=(), block=0, filter_=0):
    """slot_planes, ref_planes: the WINDOW of every component (1 or 3 arrays, chroma at half size); prev: 0, 1 or 2 luma planes ->
    dict(block, filter, blocks_x, blocks_y, temporal, blocks (structured array, row-major), width, height, samples, sse, act_spatial,
    act_temporal, count)"""
    h, w = np.asarray(ref_planes[0]).shape
    b, nbx, nby = geometry(w, h, block)
    flt = resolve_filter(w, h, filter_)
    assert nbx * nby <= MAX_BLOCKS and b % 4 == 0
    rec = np.zeros(nbx * nby, BLOCK_DTYPE)
    for c, (x, o) in enumerate(zip(slot_planes, ref_planes)):
        x, o = np.asarray(x).astype(np.int64), np.asarray(o).astype(np.int64)
        assert x.shape == o.shape
        scale = 2 if c else 1
        d2 = (x - o) ** 2
        jj, ii = np.meshgrid(np.arange(d2.shape[0]), np.arange(d2.shape[1]), indexing="ij")
        k = (scale * jj // b) * nbx + scale * ii // b
        sums = np.zeros(nbx * nby, np.int64)
        np.add.at(sums, k.ravel(), d2.ravel())
        rec["sse"][:, c] = sums.astype(np.uint64)
    ii, jj, af, t = activity(ref_planes[0], prev, flt)
    k = (jj // b) * nbx + ii // b
    for name, v in (("act_spatial", af), ("act_temporal", t), ("count", np.ones_like(af))):
        sums = np.zeros(nbx * nby, np.int64)
        np.add.at(sums, k, v)
        rec[name] = sums
    nc = len(ref_planes)
    out = dict(block=b, filter=flt, blocks_x=nbx, blocks_y=nby, temporal=len(prev), blocks=rec, num_components=nc,
               width=[np.asarray(p).shape[1] for p in ref_planes] + [0] * (3 - nc), height=[np.asarray(p).shape[0] for p in ref_planes] + [0] * (3 - nc))
    out["samples"] = [a * b_ for a, b_ in zip(out["width"], out["height"])]
    out["sse"] = [int(rec["sse"][:, c].astype(object).sum()) for c in range(3)]
    for name in ("act_spatial", "act_temporal", "count"):
        out[name] = int(rec[name].astype(object).sum())
    return out


def block_wsse(r, bit_depth, a_pic=0.0):
    """wsse of every component (float64, the blocks added in ascending order) from the dict of xpsnr_integers()"""
    if a_pic <= 0:
        a_pic = 2.0 ** (2 * bit_depth - 9) * math.sqrt(3840.0 * 2160.0 / (r["width"][0] * r["height"][0]))
    wsse = [0.0, 0.0, 0.0]
    for rec in r["blocks"]:
        count = int(rec["count"])
        q = count * (4 if r["filter"] == 2 else 1)
        act = 1.0 + float(rec["act_spatial"]) / q + 2.0 * float(rec["act_temporal"]) / q if count else 0.0
        act = max(act, 2.0 ** (bit_depth - 6))
        wk = math.sqrt(a_pic) / act
        for c in range(3):
            wsse[c] += wk * float(rec["sse"][c])
    return wsse


def xpsnr(r, bit_depth, a_pic=0.0, peak=0.0):
    """vvr_compare_xpsnr -> [Y, Cb, Cr, all components together]"""
    if peak <= 0:
        peak = float((1 << bit_depth) - 1)
    wsse = block_wsse(r, bit_depth, a_pic)
    nc = r["num_components"]

    def db(samples, e):
        return math.inf if e == 0 else 10.0 * math.log10(peak * peak * samples / e)
    out = [db(float(r["samples"][c]), wsse[c]) if c < nc else 0.0 for c in range(3)]
    out.append(db(float(sum(r["samples"][:nc])), sum(wsse[:nc])))
    return out


def anchor_planes():
    """the anchor the definition was checked with: bit depth 10, 4:2:0, window = picture = 208 x 80.  P_k( i, j ) = ( 3 i^2 + 5 j^2 +
    ( k + 1 ) i j + 37 k ) mod 1021 at the plane's own size, i the column; reference Y, Cb, Cr = P_0, P_1, P_2; o1 = P_3, o2 = P_4 at luma
    size; slot = clip( o + ( ( 3 j + i ) mod 7 ) - 3, 0, 1023 ) per plane -> slot planes, reference planes, [o1, o2]"""
    def plane(k, w, h):
        j, i = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
        return (3 * i * i + 5 * j * j + (k + 1) * i * j + 37 * k) % 1021, i, j
    sizes = [(208, 80), (104, 40), (104, 40)]
    ref, slot = [], []
    for k, (w, h) in enumerate(sizes):
        o, i, j = plane(k, w, h)
        ref.append(o.astype(np.uint16))
        slot.append(np.clip(o + ((3 * j + i) % 7) - 3, 0, 1023).astype(np.uint16))
    prev = [plane(3, 208, 80)[0].astype(np.uint16), plane(4, 208, 80)[0].astype(np.uint16)]
    return slot, ref, prev
