"""CPU: the interleaved RGB formats of the output queue (VVR_OUT_RGBA8 / _BGRA8 / _RGB24 / _BGR24 / _RGB10A2 / _RGBA16F), VVR_OUT_RGBF32 and its
normalisation (vvr_set_output_normalisation) on the stand-in runtime of tests/hoststub, where launch_output_rgb is a plain loop (vvr_output.inc,
host only).  The expected bytes come from tests/interleaved_ref.py, a numpy restatement of the definition in include/vvr.h, applied the way
tests/test_output_rgb_host.py builds its expectation: for plain windows to the crop of the picture the test wrote, with grain or a size to the
planes of the planar16 request of the same window, size, grain and seed.  A second set of checks does not use that restatement: the new formats
against the planar rgb8 / rgb16 / rgbf16 requests of the same frame, rearranged.  All comparisons are of bytes.  The helpers take a library and a
context, so tests/interleaved_on_the_device.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import colour_transform_ref as X
import interleaved_ref as IR
import output_support as SUP
import test_host_glue as T
import test_output_queue_host as Q
import test_output_semiplanar_host as S
import test_output_transform_host as XH
from vvdec_amd import abi

pytestmark = T.pytestmark
FILL = SUP.FILL
W, H_ = S.W, S.H_
FORMATS = IR.FORMATS
# one entry per instantiation of the store: bgra8 runs rgba8's code with R and B exchanged, bgr24 rgb24's
CLASSES = [("rgba8", "bgra8"), ("rgb24", "bgr24"), ("rgb10a2",), ("rgba16f",), ("rgbf32",)]
COLOURS = [(1, 0), (6, 1), (9, 0), (1, 1), (6, 0), (9, 1)]      # matrices 1 / 6 / 9, both ranges
# rows of a multiple of 8 pixels (stored whole) and rows that end 2, 4 and 6 pixels into a lane's 8, at an odd origin
STRAIGHT = [(0, 0, 448, 160), (8, 4, 200, 64), (2, 6, 202, 38), (2, 6, 196, 38), (2, 6, 198, 38)]
SIZES = [(300, 96), (134, 26)]                                  # rows that end 4 and 6 pixels into a lane's 8
NORMS = [None, ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((-3.5, 0., 1000.25), (2. ** -20, 2. ** 20, 0.5))]
XFORMS = ("none", "pq", "table")


def _setup(L, bd, seed):
    return S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(seed), bd)


def transforms(bd, seed=400):
    """none, a preset (PQ, BT.2020 -> sRGB) and a caller's table"""
    return {"none": None, "pq": X.preset(16, 9, X.TO_SRGB, 1000., 100., bd), "table": X.random_transform(np.random.default_rng(seed + bd), bd)}


def set_norm(L, ctx, norm):
    if norm is None:
        return L.vvr_set_output_normalisation(ctx, None, None)
    mean, std = [None if a is None else (C.c_float * 3)(*a) for a in norm]
    return L.vvr_set_output_normalisation(ctx, mean, std)


def same_planes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w_) in enumerate(zip(got, want)):
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), "%s, plane %d: %d bytes differ" % (what, k, int((g.view(np.uint8) != w_.view(np.uint8)).sum()))


def straight_cases():
    """(window, collocated, colour, transform, formats): every window at every chroma position with and without a transform (the preset and the
    table alternate); of every class one format - the swapped one every other time; colours rotate"""
    out = []
    for win in STRAIGHT:
        for c in range(4):
            for t in range(2):
                n = len(out)
                out.append((win, (bool(c & 1), bool(c & 2)), COLOURS[n % 6], XFORMS[0] if t == 0 else XFORMS[1 + (n // 2) % 2], [cls[(c + t + n // 8) % len(cls)] for cls in CLASSES]))
    return out


def check_straight(L, ctx, picture, bd, device=S.device_request):
    """straight from the slot, each request into pageable memory (padded rows) and into device memory with rows back to back (the kernel's own
    store where the base is aligned)"""
    tf = transforms(bd)
    for n, (win, col, colour, xf, fmts) in enumerate(straight_cases()):
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        XH.set_transform(L, ctx, tf[xf])
        b = IR.base(S.crop(picture, win), bd, colour[0], bool(colour[1]), col, tf[xf])
        for fmt in fmts:
            norm = NORMS[n % 3]
            assert set_norm(L, ctx, norm) == abi.VVR_OK, L.vvr_last_error(ctx)
            what = "%s at %d bits straight from the slot, window %r collocated %r colour %r transform %s norm %r" % (fmt, bd, win, col, colour, xf, norm)
            rgb, M = IR.values(b, fmt)
            want = IR.pack(rgb, M, fmt, norm)
            same_planes(Q.queued(L, ctx, 0, win, fmt, 3, col=col), want, what + ", pageable")
            device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=None, size=None, grain=False, stride_kind="row", mis=0, col=col)
    XH.set_transform(L, ctx, None)
    assert set_norm(L, ctx, None) == abi.VVR_OK


def matrix_cases(bd):
    """(window, size, grain, format, collocated, colour, transform, norm): every format straight from the slot, grained, rescaled, and grained
    then rescaled (grain: bit depths 8 and 10); windows, sizes, chroma positions, colours, transforms and normalisations rotate"""
    out = []
    for fmt in FORMATS:
        for grain, sized in [(False, False), (True, False), (False, True), (True, True)]:
            if grain and bd == 9:
                continue
            n = len(out)
            out.append((STRAIGHT[n % 5], SIZES[(n // 2) % 2] if sized else None, grain, fmt, (bool(n & 1), bool(n & 2)), COLOURS[n % 6], XFORMS[n % 3], NORMS[(n // 3) % 3]))
    return out


def check_matrix(L, ctx, picture, bd, device=S.device_request, strides=tuple((s, m) for s in S.STRIDES for m in (0, 2))):
    """every case into pageable destinations with padded rows, into memory of vvr_host_alloc and into device memory at every stride and base"""
    tf = transforms(bd)
    for n, (win, size, grain, fmt, col, colour, xf, norm) in enumerate(matrix_cases(bd)):
        what = "%s at %d bits, window %r size %r grain %r collocated %r colour %r transform %s norm %r" % (fmt, bd, win, size, grain, col, colour, xf, norm)
        seed = 7000 + n
        if size is None and not grain:
            planes = S.crop(picture, win)
        else:
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            planes = Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=grain)
        want = IR.frame(planes, bd, fmt, colour[0], bool(colour[1]), col, tf[xf], norm)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        XH.set_transform(L, ctx, tf[xf])
        assert set_norm(L, ctx, norm) == abi.VVR_OK, L.vvr_last_error(ctx)
        for alloc in (None, lambda nb: L.vvr_host_alloc(ctx, nb)):
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            got = Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain, alloc=alloc)      # (checks the padding of every row)
            same_planes(got, want, "%s, %s" % (what, "pinned" if alloc else "pageable"))
        for stride_kind, mis in strides:
            device(L, ctx, 0, win, fmt, 3, want, "%s, device, stride %s, base + %d" % (what, stride_kind, mis), seed=seed, size=size, grain=grain, stride_kind=stride_kind, mis=mis, col=col)
    XH.set_transform(L, ctx, None)
    assert set_norm(L, ctx, None) == abi.VVR_OK


def interleave(planes, order, alpha=None):
    """three planes of one dtype -> (h, w * C) in the given channel order, `alpha` as the fourth element"""
    h, w = planes[0].shape
    px = np.empty((h, w, 3 if alpha is None else 4), planes[0].dtype)
    for k, c in enumerate(order):
        px[:, :, k] = planes[c]
    if alpha is not None:
        px[:, :, 3] = alpha
    return px.reshape(h, -1)


def check_against_the_planar_formats(L, ctx, bd, transform, wins=((8, 4, 200, 64), (2, 6, 198, 38))):
    """the new formats from the planar requests of the same frame: no use of tests/interleaved_ref.py"""
    assert L.vvr_set_output_colour(ctx, 9, 0) == abi.VVR_OK
    XH.set_transform(L, ctx, transform)
    assert set_norm(L, ctx, None) == abi.VVR_OK
    for n, win in enumerate(wins):
        col = (bool(n & 1), not (n & 1))
        what = "%d bits, window %r, %s a transform" % (bd, win, "under" if transform is not None else "without")
        p8, p16, pf16 = [Q.queued(L, ctx, 0, win, fmt, 3, col=col) for fmt in ("rgb8", "rgb16", "rgbf16")]
        got = {fmt: Q.queued(L, ctx, 0, win, fmt, 3, col=col) for fmt in FORMATS}
        same_planes(got["rgba8"], [interleave(p8, (0, 1, 2), 255)], "rgba8 is rgb8 interleaved, " + what)
        same_planes(got["bgra8"], [interleave(p8, (2, 1, 0), 255)], "bgra8 is rgb8 interleaved with R and B exchanged, " + what)
        same_planes(got["rgb24"], [interleave(p8, (0, 1, 2))], "rgb24 is rgb8 interleaved, " + what)
        same_planes(got["bgr24"], [interleave(p8, (2, 1, 0))], "bgr24 is rgb8 interleaved with R and B exchanged, " + what)
        one = np.array(0x3C00, np.uint16).view(np.float16)
        same_planes(got["rgba16f"], [interleave(pf16, (0, 1, 2), one)], "rgba16f is rgbf16 interleaved, " + what)
        M = 65535 if transform is not None else (1 << bd) - 1
        same_planes(got["rgbf32"], [p.astype(np.float32) * np.float32(1.0 / M) for p in p16], "rgbf32 with nothing set is float32( rgb16 ) * float32( 1 / M ), " + what)
        if bd == 10 and transform is None:
            r, g, b = [p.astype(np.uint32) for p in p16]
            same_planes(got["rgb10a2"], [r | g << 10 | b << 20 | np.uint32(3 << 30)], "rgb10a2 at 10 bits is rgb16 packed, " + what)
    XH.set_transform(L, ctx, None)


# ---- the restatement

def test_the_restatement_on_values_worked_by_hand():
    one = [np.array([[v]]) for v in (1, 2, 3)]
    assert IR.pack(one, 255, "rgba8")[0].tolist() == [[1, 2, 3, 255]] and IR.pack(one, 255, "bgra8")[0].tolist() == [[3, 2, 1, 255]]
    assert IR.pack(one, 255, "rgb24")[0].tolist() == [[1, 2, 3]] and IR.pack(one, 255, "bgr24")[0].tolist() == [[3, 2, 1]]
    assert IR.pack([np.array([[1023]]), np.array([[0]]), np.array([[512]])], 1023, "rgb10a2")[0].tolist() == [[1023 | 512 << 20 | 3 << 30]]
    assert IR.pack([np.array([[1023]])] * 3, 1023, "rgba16f")[0].view(np.uint16).tolist() == [[0x3C00] * 4]
    # the 16 -> 10 bit reduction: 65535 -> 1023, 32 -> 0 ( 32 * 1023 + 32767 = 65503 ), 33 -> 1 ( 66526 ), 32767 -> 511, 32768 -> 512
    b = {"bd": 10, "e": [np.array([65535, 32, 33, 32767, 32768])] * 3}
    assert IR.values(b, "rgb10a2")[0][0].tolist() == [1023, 0, 1, 511, 512] and IR.values(b, "rgb10a2")[1] == 65535
    for e in (0, 1, 31, 32, 33, 64, 32767, 32768, 65503, 65535):
        assert (e * 1023 + 32767) // 65535 == int(np.floor(e * 1023 / 65535 + 0.5))
    # float32: scale and bias from float64, rounded once; two roundings in the frame
    scale, bias = IR.scale_bias(1023, ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
    assert scale[0] == np.float32(1.0 / (1023.0 * float(np.float32(0.229)))) and bias[2] == np.float32(-float(np.float32(0.406)) / float(np.float32(0.225)))
    f = IR.pack([np.array([[1023]]), np.array([[0]]), np.array([[700]])], 1023, "rgbf32", ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
    assert all(p.dtype == np.float32 for p in f) and f[1][0, 0] == bias[1] and f[2][0, 0] == np.float32(np.float32(700) * scale[2]) + bias[2]
    plain = IR.pack([np.array([[1023]])] * 3, 1023, "rgbf32")
    assert plain[0][0, 0] == np.float32(1023) * np.float32(1.0 / 1023) and np.signbit(IR.scale_bias(1023, None)[1][0]) == False      # noqa: E712


def test_the_cases_meet_every_instantiation_of_the_store():
    """80 = 5 classes x 4 chroma positions x 2 kinds of store x with / without a transform; both formats of a class that has two; and in the
    matrix every format plain, grained, rescaled and grained then rescaled"""
    met, fmts = set(), set()
    for win, col, _, xf, formats in straight_cases():
        for fmt in formats:
            cls = [n for n, c in enumerate(CLASSES) if fmt in c][0]
            met.add((cls, col, win[2] % 8 == 0, xf != "none"))
            fmts.add((fmt, win[2] % 8 == 0, xf != "none"))
    assert len(met) == 80
    assert fmts == set((fmt, whole, xf) for fmt in FORMATS for whole in (False, True) for xf in (False, True))
    assert set(win[2] % 8 for win in STRAIGHT) == {0, 2, 4, 6}
    for bd in (8, 9, 10):
        assert set((fmt, size is not None, grain) for _, size, grain, fmt, _, _, _, _ in matrix_cases(bd)) == set((fmt, s, g) for fmt in FORMATS for s in (False, True) for g in ((False, True) if bd != 9 else (False,)))
        assert set(c for _, _, _, _, c, _, _, _ in matrix_cases(bd)) == set((a, b) for a in (False, True) for b in (False, True))
        assert set(c for _, _, _, _, _, c, _, _ in matrix_cases(bd)) == set(COLOURS) and set(x for _, _, _, _, _, _, x, _ in matrix_cases(bd)) == set(XFORMS)


# ---- the queue

@pytest.mark.parametrize("bd", [10, 8, 9])
def test_every_instantiation_straight_from_the_slot(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 410 + bd)
    check_straight(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_interleaved_matrix(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 420 + bd)
    check_matrix(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_against_the_planar_formats(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 430 + bd)
    check_against_the_planar_formats(L, ctx, bd, None)
    check_against_the_planar_formats(L, ctx, bd, transforms(bd)["pq"])
    check_against_the_planar_formats(L, ctx, bd, transforms(bd)["table"])
    L.vvr_destroy(ctx)


def check_normalisation_state(L, ctx, picture, bd):
    """set between two submits it changes only the second; each refusal leaves the earlier value in force; NULL, NULL clears it; the half formats
    never see it"""
    win, col, colour = (2, 6, 202, 38), (True, False), (1, 0)
    assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
    XH.set_transform(L, ctx, None)
    b = IR.base(S.crop(picture, win), bd, colour[0], bool(colour[1]), col)
    want = [IR.pack(*IR.values(b, "rgbf32"), "rgbf32", norm) for norm in NORMS]
    assert not all(np.array_equal(a, b_) for a, b_ in zip(want[0], want[1]))
    assert set_norm(L, ctx, None) == abi.VVR_OK
    halves = {fmt: Q.queued(L, ctx, 0, win, fmt, 3, col=col) for fmt in ("rgbf16", "rgba16f")}
    t0, o0 = Q.submit(L, ctx, 0, win, "rgbf32", 3, col=col)
    assert set_norm(L, ctx, NORMS[1]) == abi.VVR_OK
    t1, o1 = Q.submit(L, ctx, 0, win, "rgbf32", 3, col=col)
    assert set_norm(L, ctx, NORMS[2]) == abi.VVR_OK
    t2, o2 = Q.submit(L, ctx, 0, win, "rgbf32", 3, col=col)
    assert min(t0, t1, t2) >= 0, L.vvr_last_error(ctx)
    same_planes(Q.collect(L, ctx, t2, o2), want[2], "third")
    same_planes(Q.collect(L, ctx, t0, o0), want[0], "first")
    same_planes(Q.collect(L, ctx, t1, o1), want[1], "second")
    for fmt, planes in halves.items():
        same_planes(Q.queued(L, ctx, 0, win, fmt, 3, col=col), planes, fmt + " under a normalisation")
    # refusals: the value set before stays
    mean, std = NORMS[1]
    assert set_norm(L, ctx, NORMS[1]) == abi.VVR_OK
    inf, nan = float("inf"), float("nan")
    for text, norm in [(b"given together", (mean, None)), (b"given together", (None, std)),
                       (b"not finite", ((nan, 0, 0), std)), (b"not finite", (mean, (1, inf, 1))), (b"not finite", ((0, -inf, 0), std)), (b"not finite", (mean, (1, 1, nan))),
                       (b"std outside", (mean, (0, 1, 1))), (b"std outside", (mean, (1, -1, 1))), (b"std outside", (mean, (1, 1, 2. ** -21))), (b"std outside", (mean, (2. ** 20 + 1, 1, 1))),
                       (b"mean | above", ((2. ** 20 + 1, 0, 0), std)), (b"mean | above", ((0, 0, -2. ** 21), std))]:
        assert set_norm(L, ctx, norm) == abi.VVR_ERR_PARAMETER and b"vvr_set_output_normalisation" in L.vvr_last_error(ctx) and text in L.vvr_last_error(ctx), (text, norm, L.vvr_last_error(ctx))
        same_planes(Q.queued(L, ctx, 0, win, "rgbf32", 3, col=col), want[1], "after a refused call (%s, %r)" % (text.decode(), norm))
    assert L.vvr_set_output_normalisation(None, None, None) == abi.VVR_ERR_PARAMETER
    assert set_norm(L, ctx, None) == abi.VVR_OK
    same_planes(Q.queued(L, ctx, 0, win, "rgbf32", 3, col=col), want[0], "after NULL, NULL")


@pytest.mark.parametrize("bd", [10, 8])
def test_normalisation_is_taken_when_the_request_is_submitted(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 440 + bd)
    check_normalisation_state(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_and_the_seed_chain_alone():
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 10, 450)
    win = (8, 4, 200, 64)

    def refused(text, c=ctx, fmt="rgba8", mutate=None, size=None, grain=False, w_=win):
        shapes, dt = abi.output_plane_shapes(w_, fmt, size, 3)
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, w_, fmt, size, (True, False), grain, True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c), (fmt, text, rc, L.vvr_last_error(c))

    # the refusals of the three planar RGB formats, with their texts
    for fmt in FORMATS:
        refused(b"RGB output with no colour description set (vvr_set_output_colour)", fmt=fmt)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    assert L.vvr_set_output_colour(ctx400, 1, 0) == abi.VVR_OK
    for fmt in FORMATS:
        refused(b"RGB output of a 4:0:0 context: there is no chroma to convert", c=ctx400, fmt=fmt)
    L.vvr_destroy(ctx400)
    # (a bit depth outside 8..10: no context of one exists - vvr_create refuses it - so that text cannot be met)
    for fmt in FORMATS:
        for size in [(301, 96), (300, 97)]:
            refused(b"RGB output needs an even out_w and out_h", fmt=fmt, size=size, grain=True)
    # the planes a format uses: dst[0] alone for the interleaved ones, at the row of the format
    for fmt, row in [("rgba8", 800), ("bgra8", 800), ("rgb24", 600), ("bgr24", 600), ("rgb10a2", 800), ("rgba16f", 1600), ("rgbf32", 800)]:
        refused(b"missing plane", fmt=fmt, mutate=lambda r: r.dst.__setitem__(0, None), grain=True)
        refused(b"stride below the output's row", fmt=fmt, mutate=lambda r, row=row: r.dst_stride_bytes.__setitem__(0, row - 1), grain=True)
    for k in (1, 2):
        refused(b"missing plane", fmt="rgbf32", mutate=lambda r, k=k: r.dst.__setitem__(k, None), grain=True)
        refused(b"stride below the output's row", fmt="rgbf32", mutate=lambda r, k=k: r.dst_stride_bytes.__setitem__(k, 798), grain=True)
    for f in (3, 4, 15, 18, 31, 35, 37, 47, 54, 255):
        refused(b"unknown format", mutate=lambda r, f=f: setattr(r, "format", f))
    # dst[1], dst[2] and their strides are ignored by the interleaved formats: NULL / 0 (what output_request leaves), or anything
    b = IR.base(S.crop(picture, win), 10, 1, False, (True, False))
    for fmt in FORMATS[1:]:
        shapes, dt = abi.output_plane_shapes(win, fmt, None, 3)
        assert len(shapes) == 1
        for junk in (False, True):
            outs = [np.zeros(shapes[0], dt)]
            req = abi.output_request(0, None, win, fmt, None, (True, False), False, True, outs)
            assert not req.dst[1] and not req.dst[2] and req.dst_stride_bytes[1] == 0
            if junk:
                req.dst[1], req.dst[2], req.dst_stride_bytes[1], req.dst_stride_bytes[2] = 8, 24, 1, 3
            t = L.vvr_output_submit(ctx, C.byref(req))
            assert t >= 0 and L.vvr_output_wait(ctx, t) == abi.VVR_OK, (fmt, L.vvr_last_error(ctx))
            same_planes(outs, IR.pack(*IR.values(b, fmt), fmt), "%s with dst[1], dst[2] %s" % (fmt, "set to junk" if junk else "NULL"))
    # device ranges: a plane partly inside a range (one plane of pixels; a plane of three), device planes mixed with host planes
    for fmt in ("bgr24", "rgbf32"):
        half = S.DevicePlanes(L, ctx, win, fmt, None, 3, register=False)
        nplanes = len(half.views)
        bases = [half.raw[k].ctypes.data + half.off[k] for k in range(nplanes)]
        ext = [half.geo[k][3] for k in range(nplanes)]
        req = abi.output_request(0, None, win, fmt, None, (True, False), True, True, half.views)
        for k in range(nplanes - 1):
            assert L.vvr_device_register(ctx, bases[k], ext[k]) == abi.VVR_OK
        if nplanes > 1:
            assert L.vvr_output_submit(ctx, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"mixed with planes in host memory" in L.vvr_last_error(ctx)
        assert L.vvr_device_register(ctx, bases[-1], ext[-1] // 2) == abi.VVR_OK
        assert L.vvr_output_submit(ctx, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"partly inside a device range" in L.vvr_last_error(ctx)
        for p in bases:
            assert L.vvr_device_unregister(ctx, p) == abi.VVR_OK      # (no request holds a range: none was accepted)
        assert all((raw == FILL).all() for raw in half.raw)
    # the ring is untouched: eight requests still fit; the chain too: the first of them is the frame of seed 9
    flight = [Q.submit(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(8)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    got = [Q.collect(L, ctx, t, outs) for t, outs in flight]
    assert all(np.array_equal(a, b_) for a, b_ in zip(got[0], first))
    L.vvr_destroy(ctx)


def test_python_mirror_of_the_formats_and_the_symbol():
    import vvdec_amd
    assert {name: abi.OUT_FORMATS[name] for name in FORMATS} == IR.CODES == {"rgbf32": 36, "rgba8": 48, "bgra8": 49, "rgb24": 50, "bgr24": 51, "rgb10a2": 52, "rgba16f": 53}
    assert "vvr_set_output_normalisation" in vvdec_amd.EXPORTED_SYMBOLS and hasattr(SUP.stub_lib(), "vvr_set_output_normalisation")
    win = (2, 6, 202, 38)
    assert abi.output_plane_shapes(win, "rgba8", None, 3) == ([(38, 808)], np.uint8) and abi.output_plane_shapes(win, "bgra8", (134, 26), 3) == ([(26, 536)], np.uint8)
    assert abi.output_plane_shapes(win, "rgb24", None, 3) == ([(38, 606)], np.uint8) and abi.output_plane_shapes(win, "bgr24", None, 3) == ([(38, 606)], np.uint8)
    assert abi.output_plane_shapes(win, "rgb10a2", None, 3) == ([(38, 202)], np.uint32)
    assert abi.output_plane_shapes(win, "rgba16f", None, 3) == ([(38, 808)], np.float16)
    assert abi.output_plane_shapes(win, "rgbf32", (134, 26), 3) == ([(26, 134)] * 3, np.float32)
