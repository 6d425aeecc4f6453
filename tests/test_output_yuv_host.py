"""CPU: the Y'CbCr formats at 4:4:4 and 4:2:2 of the output queue (VVR_OUT_YUV444P8 ... VVR_OUT_Y410) on the stand-in runtime of tests/hoststub,
where launch_output_yuv is a plain loop (vvr_output.inc, host only).  The expected bytes come from tests/yuv_ref.py, a numpy restatement of the
definition in include/vvr.h: for plain windows applied to the crop of the picture the test wrote, with grain or a size applied to the planes of
the planar16 request of the same window, size, grain and seed (which their own tests pin to vvdec::FilmGrain and vvdec::rescalePlane).  Two
cross-checks do not go through the restatement: the matrix of the RGB formats applied to the planes of a yuv444p16 request gives the rgb16
request, and with a collocated vertical position every second chroma row of a yuv422p16 request is the source row.  The helpers take a library
and a context, so tests/yuv_on_the_device.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import rgb_ref
import yuv_ref
import test_host_glue as T
import test_output_queue_host as Q
import test_output_rgb_host as RGB
import test_output_semiplanar_host as S
from vvdec_amd import abi

pytestmark = T.pytestmark
FILL = SUP.FILL
W, H_ = S.W, S.H_
PER_CASE = 3
ALL_STRIDES = tuple((s, m) for s in S.STRIDES for m in (0, 2))


def cases(bd):
    """(window, size, grain, format, collocated): the windows, sizes and grain of the semi-planar matrix, three formats to a case.  The formats
    the bit depth accepts (nine at 8 bits, five above) rotate three to a case and move on by three more every six cases, the positions come
    round every four cases: every format meets every size, and no size, and every position, and v210 rows that end in a full group, in a
    group of four and in a group of two pixels (test_the_cases_meet_every_instantiation_of_the_kernel)."""
    F = yuv_ref.formats(bd)
    out = []
    for n, (win, size, grain) in enumerate(S.cases(bd)):
        for j in range(PER_CASE):
            out.append((win, size, grain, F[(PER_CASE * n + j + 3 * (n // 6)) % len(F)], (bool(n & 1), bool(n & 2))))
    return out


def instantiations(bd):
    """(window, format, collocated): every format at every chroma position it has - four at 4:4:4, the two vertical ones at 4:2:2 - straight
    from the slot, on two windows whose rows are stored whole and one whose rows are stored pixel pair by pixel pair"""
    return [(win, fmt, (bool(c & 1), bool(c & 2))) for win in RGB.STRAIGHT for fmt in yuv_ref.formats(bd) for c in range(4) if fmt in yuv_ref.FULL or not c & 1]


def same_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in range(len(want)):
        g, w_ = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), "%s, plane %d: %d elements differ" % (what, k, int((g != w_).sum()))


def expected_planes(L, ctx, picture, win, size, grain, seed, col):
    """the 4:2:0 frame that is converted: the crop of what was written, or the planar16 request of the same window, size, grain and seed"""
    if size is None and not grain:
        return S.crop(picture, win)
    assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    return Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=grain)


def check_instantiations(L, ctx, picture, bd, device=S.device_request):
    """each into pageable memory and into device memory with rows back to back (the kernel's own store where the base is aligned)"""
    for win, fmt, col in instantiations(bd):
        what = "%s at %d bits straight from the slot, window %r collocated %r" % (fmt, bd, win, col)
        want = yuv_ref.yuv(S.crop(picture, win), bd, fmt, col)
        same_bytes(Q.queued(L, ctx, 0, win, fmt, 3, col=col), want, what + ", pageable")
        device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=None, size=None, grain=False, stride_kind="row", mis=0, col=col)


def check_matrix(L, ctx, picture, bd, device=S.device_request, strides=ALL_STRIDES, per_request=2):
    """every case into pageable destinations with padded rows, into memory of vvr_host_alloc and into device memory; the strides and bases
    rotate over the requests, `per_request` of them each"""
    planes, turn = None, 0
    for n, (win, size, grain, fmt, col) in enumerate(cases(bd)):
        what = "%s at %d bits, window %r size %r grain %r collocated %r" % (fmt, bd, win, size, grain, col)
        seed = 7000 + n // PER_CASE
        if n % PER_CASE == 0:
            planes = expected_planes(L, ctx, picture, win, size, grain, seed, col)
        want = yuv_ref.yuv(planes, bd, fmt, col)
        for alloc in (None, lambda nb: L.vvr_host_alloc(ctx, nb)):
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            got = Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain, alloc=alloc)      # (checks the padding of every row)
            same_bytes(got, want, "%s, %s" % (what, "pinned" if alloc else "pageable"))
        for _ in range(per_request):
            stride_kind, mis = strides[turn % len(strides)]
            turn += 1
            device(L, ctx, 0, win, fmt, 3, want, "%s, device, stride %s, base + %d" % (what, stride_kind, mis), seed=seed, size=size, grain=grain, stride_kind=stride_kind, mis=mis, col=col)


def check_the_planes_are_the_ones_rgb_converts(L, ctx, bd, wins=RGB.STRAIGHT):
    """rgb_ref.matrix_int of the three planes of a yuv444p16 request is the rgb16 request of the same window, for all eight colour descriptions"""
    for n, colour in enumerate(RGB.COLOURS):
        win, col = wins[n % len(wins)], (bool(n & 1), bool(n & 2))
        y, u, v = Q.queued(L, ctx, 0, win, "yuv444p16", 3, col=col)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        rgb16 = Q.queued(L, ctx, 0, win, "rgb16", 3, col=col)
        want, _ = rgb_ref.matrix_int(y, u, v, colour[0], bool(colour[1]), bd, bd)
        same_bytes(rgb16, [w_.astype(np.uint16) for w_ in want], "rgb16 from the planes of yuv444p16, %r %r %r" % (win, col, colour))


def check_phase_0_is_the_identity(L, ctx, picture, wins=RGB.STRAIGHT):
    """yuv422p16 with a collocated vertical position: every second chroma row is the source row, the luma is planar16's"""
    for win in wins:
        for hor in (False, True):
            y, u, v = Q.queued(L, ctx, 0, win, "yuv422p16", 3, col=(hor, True))
            src = S.crop(picture, win)
            assert np.array_equal(u[0::2], src[1]) and np.array_equal(v[0::2], src[2]), (win, hor)
            assert np.array_equal(y, Q.queued(L, ctx, 0, win, "planar16", 3)[0]), (win, hor)


def _setup(L, bd, seed):
    return S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(seed), bd)


# ---- the restatement itself

def test_the_vertical_pass_alone_is_the_two_passes_with_phase_0():
    """( sum + 32 ) >> 6 over the rows equals the two passes of the RGB formats at the even columns of a horizontally collocated upsample (phase 0:
    64 times the sample, then ( 64 sum + 2048 ) >> 12), and a collocated vertical position copies every source row"""
    rng = np.random.default_rng(120)
    for bd in (8, 9, 10):
        p = rng.integers(0, 1 << bd, (19, 23), dtype=np.uint16)
        p[:3], p[-2:] = (1 << bd) - 1, 0
        for ver in (False, True):
            rows = yuv_ref.upsample_rows(p, bd, ver)
            assert np.array_equal(rows, rgb_ref.upsample(p, bd, (True, ver))[:, 0::2]), (bd, ver)
        assert np.array_equal(yuv_ref.upsample_rows(p, bd, True)[0::2], p)


def test_the_packing_of_a_known_group():
    """v210, y410, uyvy, yuy2 and y210 of samples whose place shows in their value"""
    y = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11, 12, 13, 14, 15, 16]])
    cb, cr = np.array([[101, 102, 103, 104]]), np.array([[201, 202, 203, 204]])
    col = (True, True)
    v, = yuv_ref.yuv((y, cb, cr), 10, "v210", col)
    assert v.shape == (2, 8) and v.dtype == np.uint32
    assert list(v[0]) == [101 | 1 << 10 | 201 << 20, 2 | 102 << 10 | 3 << 20, 202 | 4 << 10 | 103 << 20, 5 | 203 << 10 | 6 << 20, 104 | 7 << 10 | 204 << 20, 8, 0, 0]
    assert list(yuv_ref.yuv((y, cb, cr), 8, "v210", col)[0][0][:2]) == [404 | 4 << 10 | 804 << 20, 8 | 408 << 10 | 12 << 20]
    assert list(yuv_ref.yuv((y, cb, cr), 8, "uyvy", col)[0][0][:8]) == [101, 1, 201, 2, 102, 3, 202, 4]
    assert list(yuv_ref.yuv((y, cb, cr), 8, "yuy2", col)[0][1][:8]) == [9, 101, 10, 201, 11, 102, 12, 202]
    assert list(yuv_ref.yuv((y, cb, cr), 9, "y210", col)[0][0][:4]) == [1 << 7, 101 << 7, 2 << 7, 201 << 7]
    assert yuv_ref.yuv((y, cb, cr), 9, "y410", (True, True))[0][0][0] == (101 << 1) | (1 << 1) << 10 | (201 << 1) << 20 | 3 << 30


# ---- the queue

def test_the_cases_meet_every_instantiation_of_the_kernel():
    """46 = 3 formats x 4 positions x 2 kinds of store at 4:4:4, 5 x 2 x 2 at 4:2:2 and v210 at its two positions, straight from the slot; in
    the matrix every format with every size and none and with every position, and v210 with every kind of last group"""
    met = set((fmt, col if fmt in yuv_ref.FULL else col[1], fmt == "v210" or win[2] % 8 == 0) for win, fmt, col in instantiations(8))
    assert len(met) == 46
    assert set(f for _, f, _ in instantiations(10)) == set(yuv_ref.formats(10)) == set(f for _, f, _ in instantiations(9)) and len(yuv_ref.formats(10)) == 5
    for bd in (8, 9, 10):
        F = yuv_ref.formats(bd)
        assert set((fmt, size) for _, size, _, fmt, _ in cases(bd)) == set((fmt, size) for fmt in F for size in S.SIZES)
        assert set((fmt, col) for _, _, _, fmt, col in cases(bd)) == set((fmt, (a, b)) for fmt in F for a in (False, True) for b in (False, True))
        assert set((size or win[2:])[0] % 6 for win, size, _, fmt, _ in cases(bd) if fmt == "v210") == {0, 2, 4}
    # ... which the widths of the matrix give: rows that end in a full group, in four pixels and in two
    assert [w_ % 6 for w_ in (144, 300, 448, 202, 200, 134)] == [0, 0, 4, 4, 2, 2]


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_every_instantiation_straight_from_the_slot(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 125 + bd)
    check_instantiations(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_yuv_matrix(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 130 + bd)
    check_matrix(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_the_444_planes_are_the_ones_the_rgb_formats_convert(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 140 + bd)
    check_the_planes_are_the_ones_rgb_converts(L, ctx, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_phase_0_of_422_is_the_identity(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 150 + bd)
    check_phase_0_is_the_identity(L, ctx, picture)
    L.vvr_destroy(ctx)


def test_one_plane_formats_ignore_the_other_planes():
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 8, 160)
    win = (8, 4, 200, 64)
    for fmt in yuv_ref.ONE_PLANE:
        shapes, dt = abi.output_plane_shapes(win, fmt, None, 3)
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, win, fmt, None, (False, True), False, True, outs)
        req.dst[1], req.dst[2], req.dst_stride_bytes[1], req.dst_stride_bytes[2] = None, None, 0, 0
        t = L.vvr_output_submit(ctx, C.byref(req))
        assert t >= 0 and L.vvr_output_wait(ctx, t) == abi.VVR_OK, (fmt, L.vvr_last_error(ctx))
        same_bytes(outs, yuv_ref.yuv(S.crop(picture, win), 8, fmt, (False, True)), fmt)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_and_the_seed_chain_alone():
    L = SUP.stub_lib()
    rng = np.random.default_rng(161)
    ctx, picture, bank = S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, 10, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, 10)
    win = (8, 4, 200, 64)

    def refused(text, c=ctx, fmt="yuv444p16", mutate=None, size=None, grain=False, w_=win):
        shapes, dt = abi.output_plane_shapes(w_, fmt, size, 3)
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, w_, fmt, size, (True, False), grain, True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c), (text, rc, L.vvr_last_error(c))

    # the seed chain: what a grained planar16 request gives from seed 9 - before and after all the refusals below
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    # a 4:0:0 context: no chroma to upsample
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    for fmt in yuv_ref.FORMATS:
        refused(b"no chroma to upsample", c=ctx400, fmt=fmt)
    L.vvr_destroy(ctx400)
    # the 8-bit formats in a context of more than 8 bits: VVR_OUT_PLANAR8's wording
    for fmt in yuv_ref.BYTES:
        refused(b"8-bit output of a stream with more than 8 bits per sample", fmt=fmt, grain=True)
    ctx9 = SUP.make_ctx(L, W, H_, 9, 1)
    for fmt in yuv_ref.BYTES:
        refused(b"8-bit output of a stream with more than 8 bits per sample", c=ctx9, fmt=fmt)
    L.vvr_destroy(ctx9)
    # (a bit depth outside 8 .. 10 has its refusal too, but vvr_create makes no such context: the text cannot be reached from here)
    # an odd out_w or out_h
    for fmt in ("yuv444p16", "yuv422p16", "y210", "v210", "y410"):
        for size in [(301, 96), (300, 97), (301, 97)]:
            refused(b"even out_w and out_h", fmt=fmt, size=size, grain=True)
    # a missing plane or a stride below the row, among the planes the format uses
    for fmt, rows in (("yuv444p16", (400, 400, 400)), ("yuv422p16", (400, 200, 200)), ("y210", (800,)), ("v210", (34 * 16,)), ("y410", (800,))):
        for k, row in enumerate(rows):
            refused(b"missing plane", fmt=fmt, mutate=lambda r, k=k: r.dst.__setitem__(k, None), grain=True)
            refused(b"stride below the output's row", fmt=fmt, mutate=lambda r, k=k, row=row: r.dst_stride_bytes.__setitem__(k, row - 2), grain=True)
    refused(b"stride below the output's row", fmt="v210", size=(134, 26), mutate=lambda r: r.dst_stride_bytes.__setitem__(0, 23 * 16 - 16))      # (134 pixels: 23 groups, the last of two pixels)
    # the codes next to the new ones, and the codes that have always been refused
    for f in (63, 73, 3, 4, 15, 18, 31, 35, 37, 47, 54, 255):
        refused(b"unknown format", mutate=lambda r, f=f: setattr(r, "format", f))
    # inherited
    for w_ in [(300, 0, 200, 64), (1, 0, 200, 64), (0, 0, 201, 64), (0, 0, 200, 63)]:
        refused(b"outside the picture, or odd", fmt="v210", w_=w_)
    refused(b"wider than 128", fmt="y210", grain=True, w_=(0, 0, 128, 64))
    refused(b"1/8", fmt="yuv422p16", size=(8, 64))
    # device ranges: a plane partly inside a range, device planes mixed with host planes
    half = S.DevicePlanes(L, ctx, win, "yuv422p16", None, 3, register=False)
    b = [half.raw[k].ctypes.data + half.off[k] for k in range(3)]
    e = [half.geo[k][3] for k in range(3)]
    assert L.vvr_device_register(ctx, b[0], e[0]) == abi.VVR_OK and L.vvr_device_register(ctx, b[1], e[1]) == abi.VVR_OK
    req = abi.output_request(0, None, win, "yuv422p16", None, (True, False), True, True, half.views)
    assert L.vvr_output_submit(ctx, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"mixed with planes in host memory" in L.vvr_last_error(ctx)
    assert L.vvr_device_register(ctx, b[2], e[2] // 2) == abi.VVR_OK
    assert L.vvr_output_submit(ctx, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"partly inside a device range" in L.vvr_last_error(ctx)
    for k in range(3):
        assert L.vvr_device_unregister(ctx, b[k]) == abi.VVR_OK      # (no request holds a range: none was accepted)
    assert all((raw == FILL).all() for raw in half.raw)
    # the ring is untouched: eight requests still fit; the chain too: the first of them is the frame of seed 9
    flight = [Q.submit(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(8)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    got = [Q.collect(L, ctx, t, outs) for t, outs in flight]
    assert all(np.array_equal(a, b_) for a, b_ in zip(got[0], first))
    L.vvr_destroy(ctx)


def test_an_accepted_grained_request_advances_the_chain_once():
    """a grained y210 request takes one frame of the seed chain, as a grained planar16 request does: the request after it gets the next frame"""
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 10, 162)
    win = (8, 4, 200, 64)
    assert L.vvr_set_film_grain_seed(ctx, 33) == abi.VVR_OK
    a = [Q.queued(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(2)]
    assert L.vvr_set_film_grain_seed(ctx, 33) == abi.VVR_OK
    got = Q.queued(L, ctx, 0, win, "y210", 3, grain=True)
    same_bytes(got, yuv_ref.yuv(a[0], 10, "y210", (True, False)), "first frame of the chain")
    same_bytes(Q.queued(L, ctx, 0, win, "planar16", 3, grain=True), a[1], "second frame of the chain")
    L.vvr_destroy(ctx)


def test_python_mirror_of_the_formats():
    assert [abi.OUT_FORMATS[f] for f in yuv_ref.FORMATS] == list(range(64, 73))
    win = (2, 6, 202, 38)
    assert abi.output_plane_shapes(win, "yuv444p8", None, 3) == ([(38, 202)] * 3, np.uint8)
    assert abi.output_plane_shapes(win, "yuv444p16", (134, 26), 3) == ([(26, 134)] * 3, np.uint16)
    assert abi.output_plane_shapes(win, "yuv422p8", None, 3) == ([(38, 202), (38, 101), (38, 101)], np.uint8)
    assert abi.output_plane_shapes(win, "yuv422p16", (134, 26), 3) == ([(26, 134), (26, 67), (26, 67)], np.uint16)
    assert abi.output_plane_shapes(win, "uyvy", None, 3) == ([(38, 404)], np.uint8) and abi.output_plane_shapes(win, "yuy2", (300, 96), 3) == ([(96, 600)], np.uint8)
    assert abi.output_plane_shapes(win, "y210", None, 3) == ([(38, 404)], np.uint16)
    assert abi.output_plane_shapes(win, "v210", None, 3) == ([(38, 34 * 4)], np.uint32) and abi.output_plane_shapes(win, "v210", (300, 96), 3) == ([(96, 200)], np.uint32)
    assert abi.output_plane_shapes(win, "v210", (134, 26), 3) == ([(26, 23 * 4)], np.uint32) and abi.output_plane_shapes((0, 0, 2, 2), "v210", None, 3) == ([(2, 4)], np.uint32)
    assert abi.output_plane_shapes(win, "y410", None, 3) == ([(38, 202)], np.uint32)
    # the planes of yuv_ref have these shapes and types
    rng = np.random.default_rng(163)
    planes = [rng.integers(0, 256, (38 >> s, 202 >> s), dtype=np.uint16) for s in (0, 1, 1)]
    for fmt in yuv_ref.FORMATS:
        shapes, dt = abi.output_plane_shapes(win, fmt, None, 3)
        got = yuv_ref.yuv(planes, 8, fmt, (False, False))
        assert [g.shape for g in got] == shapes and all(g.dtype == dt for g in got), fmt


def test_into_is_checked_before_anything_is_submitted():
    """Reconstructor.output_submit(into=...): what the shape of the argument alone decides, on an object that has no context"""
    torch = pytest.importorskip("torch")
    import vvdec_amd
    rec = object.__new__(vvdec_amd.Reconstructor)
    rec.width, rec.height, rec.chroma_format = 64, 32, 1
    with pytest.raises(ValueError, match="one 2-D tensor"):
        rec.output_submit(0, fmt="v210", into=torch.zeros((3, 32, 44), dtype=torch.int32))
    with pytest.raises(ValueError, match="4:4:4"):
        rec.output_submit(0, fmt="yuv422p16", into=torch.zeros((3, 32, 64), dtype=torch.int16))
    with pytest.raises(ValueError, match="needs 3 planes"):
        rec.output_submit(0, fmt="yuv422p8", into=[torch.zeros((32, 64), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="needs 1 planes"):
        rec.output_submit(0, fmt="y410", into=[torch.zeros((32, 64), dtype=torch.int32)] * 3)
