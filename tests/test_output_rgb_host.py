"""CPU: the RGB formats of the output queue (VVR_OUT_RGB8 / _RGB16 / _RGBF16, vvr_set_output_colour) on the stand-in runtime of tests/hoststub,
where launch_output_rgb is a plain loop (vvr_output.inc, host only).  The expected bytes come from tests/rgb_ref.py, a numpy restatement of the
definition in include/vvr.h: for plain windows applied to the crop of the picture the test wrote, with grain or a size applied to the planes of
the planar16 request of the same window, size, grain and seed (which their own tests pin to vvdec::FilmGrain and vvdec::rescalePlane).  The
restatement itself is checked against the real-valued H.273 equations, on ramps, and against vvdec::rescalePlane.  The helpers take a library and
a context, so tests/rgb_on_the_device.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import rescale_ref
import rgb_ref
import test_film_grain_host as H
import test_host_glue as T
import test_output_queue_host as Q
import test_output_semiplanar_host as S
from vvdec_amd import abi

pytestmark = T.pytestmark
FILL = SUP.FILL
W, H_ = S.W, S.H_
FORMATS = ["rgb8", "rgb16", "rgbf16"]
COLOURS = [(1, 0), (5, 1), (9, 0), (6, 0), (1, 1), (9, 1), (5, 0), (6, 1)]      # (matrix_coefficients, full_range): every accepted pair
DEPTHS = [(8, 8), (9, 8), (9, 9), (10, 8), (10, 10)]                           # (bd, od)
BOUND = 0.5 + (1023 + 512 + 512) / 2 ** 15                                     # rounding of the result + of the coefficients, at most 10 bits


def cases(bd):
    """(window, size, grain, format, collocated, colour): the windows, sizes and grain of the semi-planar matrix; formats (3), chroma positions
    (4) and colour descriptions (8) rotate over them.  The sizes are the inner loop of that matrix, three of them, and the positions come
    round every four cases, so the format moves on by one more every four cases: in 12 cases every format meets every size, and no size, and
    every position (test_the_cases_meet_every_instantiation_of_the_kernel)."""
    out = []
    for n, (win, size, grain) in enumerate(S.cases(bd)):
        out.append((win, size, grain, FORMATS[(n + n // 4) % 3], (bool(n & 1), bool(n & 2)), COLOURS[(n + n // 8) % 8]))
    return out


# k_output_rgb is compiled once per (chroma position, format, kind of store): rows of a multiple of 8 samples are stored whole, others pair by pair
STRAIGHT = [(0, 0, 448, 160), (8, 4, 200, 64), (2, 6, 202, 38)]


def instantiations():
    """(window, format, collocated, colour): every format at every chroma position straight from the slot, on two windows whose rows are stored
    whole and one whose rows are stored pair by pair - all 24 instantiations of the kernel with values compared"""
    out = []
    for win in STRAIGHT:
        for fmt in FORMATS:
            for c in range(4):
                out.append((win, fmt, (bool(c & 1), bool(c & 2)), COLOURS[len(out) % 8]))
    return out


def check_instantiations(L, ctx, picture, bd, device=S.device_request):
    """each into pageable memory and into device memory with rows back to back (the kernel's own store where the base is aligned)"""
    for win, fmt, col, colour in instantiations():
        what = "%s at %d bits straight from the slot, window %r collocated %r colour %r" % (fmt, bd, win, col, colour)
        want = rgb_ref.rgb(S.crop(picture, win), bd, fmt, colour[0], bool(colour[1]), col)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        same_bytes(Q.queued(L, ctx, 0, win, fmt, 3, col=col), want, what + ", pageable")
        device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=None, size=None, grain=False, stride_kind="row", mis=0, col=col)


def expected(L, ctx, picture, win, size, grain, seed, fmt, col, colour, bd):
    if size is None and not grain:
        planes = S.crop(picture, win)
    else:
        assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
        planes = Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=grain)
    return rgb_ref.rgb(planes, bd, fmt, colour[0], bool(colour[1]), col)


def same_bytes(got, want, what):
    assert len(got) == 3
    for k in range(3):
        g, w_ = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), "%s, plane %d: %d samples differ" % (what, k, int((g.view(np.uint8) != w_.view(np.uint8)).reshape(g.shape[0], g.shape[1], -1).any(axis=2).sum()))


def check_matrix(L, ctx, picture, bd, device=S.device_request, strides=tuple((s, m) for s in S.STRIDES for m in (0, 2))):
    """every case into pageable destinations with padded rows, into memory of vvr_host_alloc and into device memory at every stride and base"""
    for n, (win, size, grain, fmt, col, colour) in enumerate(cases(bd)):
        what = "%s at %d bits, window %r size %r grain %r collocated %r colour %r" % (fmt, bd, win, size, grain, col, colour)
        seed = 5000 + n
        want = expected(L, ctx, picture, win, size, grain, seed, fmt, col, colour, bd)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        for alloc in (None, lambda nb: L.vvr_host_alloc(ctx, nb)):
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            got = Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain, alloc=alloc)      # (checks the padding of every row)
            same_bytes(got, want, "%s, %s" % (what, "pinned" if alloc else "pageable"))
        for stride_kind, mis in strides:
            device(L, ctx, 0, win, fmt, 3, want, "%s, device, stride %s, base + %d" % (what, stride_kind, mis), seed=seed, size=size, grain=grain, stride_kind=stride_kind, mis=mis, col=col)


# ---- the restatement itself

def test_coefficient_checkpoints():
    assert rgb_ref.coefficients(1, False, 8, 8) == (19077, 29372, -3494, -8731, 34610)
    assert rgb_ref.coefficients(1, False, 10, 10) == (19133, 29459, -3504, -8757, 34711)
    assert rgb_ref.coefficients(5, True, 8, 8) == (16384, 22970, -5638, -11700, 29032)
    assert rgb_ref.coefficients(9, False, 10, 8) == (4769, 6876, -767, -2664, 8773)
    assert rgb_ref.coefficients(6, True, 8, 8) == rgb_ref.coefficients(5, True, 8, 8)


@pytest.mark.parametrize("matrix", [1, 5, 9])
def test_integer_matrix_is_within_the_bound_of_the_real_valued_equations(matrix):
    """all 2^24 triples at 8 bits; at 9 and 10 bits a seeded sample with the eight corners; both ranges, every (bd, od).  int32 is enough."""
    rng = np.random.default_rng(70 + matrix)
    worst = 0.
    for full in (False, True):
        for bd, od in DEPTHS:
            top = (1 << bd) - 1
            if bd == 8:
                cb, cr = [a.ravel() for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
                blocks = [(np.full(cb.shape, y), cb, cr) for y in range(256)]
            else:
                t = rng.integers(0, top + 1, (3, 1 << 18))
                t[:, :8] = np.array([[top * ((k >> b) & 1) for k in range(8)] for b in range(3)])
                blocks = [tuple(t)]
            for y, cb, cr in blocks:
                got, acc = rgb_ref.matrix_int(y, cb, cr, matrix, full, bd, od)
                assert acc < 3.7e7
                err = max(float(np.abs(g - f).max()) for g, f in zip(got, rgb_ref.float_rgb(y, cb, cr, matrix, full, bd, od)))
                worst = max(worst, err)
                assert err <= BOUND, (matrix, full, bd, od, err)
    print("matrix %d: largest distance from the real-valued equations %.4f (bound %.4f)" % (matrix, worst, BOUND))


def test_phases_on_a_ramp():
    """chroma 8 * i: the collocated direction gives 4 X, the other 4 X - 2, exactly, away from the edges (the DCTIF reproduces linear ramps)"""
    n = 24
    ramp = 8 * np.arange(n)
    X = np.arange(2 * n)
    inner = slice(4, 2 * n - 4)
    for col in (True, False):
        hor = rgb_ref.upsample(np.tile(ramp, (6, 1)), 10, (col, True))
        ver = rgb_ref.upsample(np.tile(ramp.reshape(-1, 1), (1, 6)), 10, (True, col))
        want = 4 * X - (0 if col else 2)
        assert (hor[:, inner] == want[inner]).all() and (ver[inner, :] == want[inner].reshape(-1, 1)).all(), col


@Q.need_ref
def test_upsampler_is_rescale_plane_at_twice_the_size(tmp_path):
    """both directions collocated: vvdec::rescalePlane of the plane as a chroma plane of a 4:4:4 frame at twice the size reads at 16 * i too"""
    rng = np.random.default_rng(71)
    planes = [(rng.integers(0, 1 << bd, (h, w), dtype=np.uint16), bd) for bd in (8, 10) for w, h in ((101, 19), (2, 2))]
    got = rescale_ref.rescale([(p, 2 * p.shape[1], 2 * p.shape[0], 1, 3, bd, True, True) for p, bd in planes], T.build_stub(), False, str(tmp_path))
    for (p, bd), g in zip(planes, got):
        assert np.array_equal(g, rgb_ref.upsample(p, bd, (True, True))), (p.shape, bd)


# ---- the queue

def test_the_cases_meet_every_instantiation_of_the_kernel():
    """24 = 4 chroma positions x 3 formats x 2 kinds of store, straight from the slot; and in the matrix every format with every size and none"""
    met = set((fmt, col, win[2] % 8 == 0) for win, fmt, col, _ in instantiations())
    assert len(met) == 24
    for bd in (8, 9, 10):
        assert set((fmt, size) for _, size, _, fmt, _, _ in cases(bd)) == set((fmt, size) for fmt in FORMATS for size in S.SIZES)
        assert set((fmt, col) for _, _, _, fmt, col, _ in cases(bd)) == set((fmt, (a, b)) for fmt in FORMATS for a in (False, True) for b in (False, True))
        assert set(colour for _, _, _, _, _, colour in cases(bd)) == set(COLOURS)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_every_instantiation_straight_from_the_slot(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(85 + bd), bd)
    check_instantiations(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_rgb_matrix(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(80 + bd), bd)
    check_matrix(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_and_the_seed_chain_alone():
    L = SUP.stub_lib()
    rng = np.random.default_rng(81)
    ctx, picture, bank = S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, 10, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, 10)
    win = (8, 4, 200, 64)

    def refused(text, c=ctx, fmt="rgb16", mutate=None, size=None, grain=False, w_=win):
        shapes, dt = abi.output_plane_shapes(w_, fmt, size, 3)
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, w_, fmt, size, (True, False), grain, True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c), (text, rc, L.vvr_last_error(c))

    # the colour description: none in a new context; what is not accepted is refused with a text
    for fmt in FORMATS:
        refused(b"no colour description set", fmt=fmt)
    for m, full in [(0, 0), (2, 0), (14, 0), (3, 1), (-1, 0), (1, 2), (1, -1)]:
        assert L.vvr_set_output_colour(ctx, m, full) == abi.VVR_ERR_PARAMETER and b"vvr_set_output_colour" in L.vvr_last_error(ctx), (m, full)
    refused(b"no colour description set")
    assert L.vvr_set_output_colour(None, 1, 0) == abi.VVR_ERR_PARAMETER
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    # the seed chain: what a grained planar16 request gives from seed 9 - before and after all the refusals below
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    assert L.vvr_set_output_colour(ctx400, 1, 0) == abi.VVR_OK
    for fmt in FORMATS:
        refused(b"no chroma", c=ctx400, fmt=fmt)
    L.vvr_destroy(ctx400)
    for size in [(301, 96), (300, 97), (301, 97)]:
        refused(b"even out_w and out_h", size=size, grain=True)
    refused(b"stride below the output's row", mutate=lambda r: r.dst_stride_bytes.__setitem__(1, 2 * 200 - 2), grain=True)      # (a chroma row would fit: RGB planes are at the luma size)
    refused(b"stride below the output's row", fmt="rgb8", mutate=lambda r: r.dst_stride_bytes.__setitem__(2, 199), grain=True)
    for k in range(3):
        refused(b"missing plane", mutate=lambda r, k=k: r.dst.__setitem__(k, None), grain=True)
    # inherited
    for w_ in [(300, 0, 200, 64), (1, 0, 200, 64), (0, 0, 201, 64), (0, 0, 200, 63)]:
        refused(b"outside the picture, or odd", w_=w_)
    refused(b"wider than 128", grain=True, w_=(0, 0, 128, 64))
    refused(b"1/8", size=(8, 64))
    refused(b"no such slot", mutate=lambda r: setattr(r, "slot", 7))
    for f in (3, 4, 15, 18, 31, 35, 255):
        refused(b"unknown format", mutate=lambda r, f=f: setattr(r, "format", f))
    ctx9 = SUP.make_ctx(L, W, H_, 9, 1)
    assert L.vvr_set_output_colour(ctx9, 1, 0) == abi.VVR_OK
    bank9 = abi.film_grain_bank(**H._bank(rng))
    assert L.vvr_set_film_grain(ctx9, C.addressof(bank9)) == abi.VVR_OK
    refused(b"bit depth of 8 or 10", c=ctx9, grain=True)
    L.vvr_destroy(ctx9)
    # device ranges: a plane partly inside a range, device planes mixed with host planes
    half = S.DevicePlanes(L, ctx, win, "rgb16", None, 3, register=False)
    b = [half.raw[k].ctypes.data + half.off[k] for k in range(3)]
    e = [half.geo[k][3] for k in range(3)]
    assert L.vvr_device_register(ctx, b[0], e[0]) == abi.VVR_OK and L.vvr_device_register(ctx, b[1], e[1]) == abi.VVR_OK
    req = abi.output_request(0, None, win, "rgb16", None, (True, False), True, True, half.views)
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


def test_a_request_takes_the_colour_description_set_when_it_is_submitted():
    """vvr_set_output_colour between two submits changes only the second; a refused call leaves the first value in force"""
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    picture = film_grain_ref.grain_picture(np.random.default_rng(82), W, H_, 10, 1)
    SUP.write_picture(L, ctx, 0, picture)
    win, col = (2, 6, 202, 38), (True, False)
    want = {colour: rgb_ref.rgb(S.crop(picture, win), 10, "rgb16", colour[0], bool(colour[1]), col) for colour in [(1, 0), (9, 1)]}
    assert not all(np.array_equal(a, b) for a, b in zip(want[(1, 0)], want[(9, 1)]))
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    t0, o0 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    assert L.vvr_set_output_colour(ctx, 9, 1) == abi.VVR_OK
    t1, o1 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    assert L.vvr_set_output_colour(ctx, 2, 0) == abi.VVR_ERR_PARAMETER and L.vvr_set_output_colour(ctx, 1, 7) == abi.VVR_ERR_PARAMETER
    t2, o2 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    assert min(t0, t1, t2) >= 0, L.vvr_last_error(ctx)
    same_bytes(Q.collect(L, ctx, t2, o2), want[(9, 1)], "after a refused call")
    same_bytes(Q.collect(L, ctx, t0, o0), want[(1, 0)], "first")
    same_bytes(Q.collect(L, ctx, t1, o1), want[(9, 1)], "second")
    L.vvr_destroy(ctx)


def test_python_mirror_of_the_formats():
    assert (abi.OUT_FORMATS["rgb8"], abi.OUT_FORMATS["rgb16"], abi.OUT_FORMATS["rgbf16"]) == (32, 33, 34)
    assert abi.output_plane_shapes((2, 6, 202, 38), "rgb8", None, 3) == ([(38, 202)] * 3, np.uint8)
    assert abi.output_plane_shapes((2, 6, 202, 38), "rgb16", (134, 26), 3) == ([(26, 134)] * 3, np.uint16)
    assert abi.output_plane_shapes((0, 0, 448, 160), "rgbf16", None, 3) == ([(160, 448)] * 3, np.float16)
