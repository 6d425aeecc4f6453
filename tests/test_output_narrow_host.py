"""CPU: 8-bit Y'CbCr frames from 9- and 10-bit pictures (vvr_set_output_narrowing; VVR_OUT_PLANAR8, _NV12, _YUV444P8, _YUV422P8, _UYVY, _YUY2) on the
stand-in runtime of tests/hoststub, where launch_output_narrow and the narrowing of launch_output_yuv are plain loops (vvr_output.inc, host
only).  The expected bytes come from tests/narrow_ref.py, a numpy restatement of the definition in include/vvr.h, applied to the planes of the
16-bit sibling request (planar16, yuv444p16, yuv422p16) of the same window, size, grain and seed - which their own tests pin to the picture, to
vvdec::FilmGrain, to vvdec::rescalePlane and to tests/yuv_ref.py.  Four checks do not go through the restatement: the bytes of a constant plane
under DITHER add up to the 10-bit value over every aligned 2 x 2 cell, a picture of multiples of 4 stores v / 4 in every mode, TRUNCATE is
planar16 >> s, and the luma of every format is planar8's.  The helpers take a library and a context, so tests/narrow_on_the_device.py runs the
same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import narrow_ref
import output_support as SUP
import yuv_ref
import test_host_glue as T
import test_output_queue_host as Q
import test_output_rgb_host as RGB
import test_output_semiplanar_host as S
from vvdec_amd import abi

pytestmark = T.pytestmark
FILL = SUP.FILL
W, H_ = S.W, S.H_
# luma rows of 18 and chroma rows of 9 samples: shorter than two of a lane's pieces of 16 and of odd length, so one piece spans three rows and
# the column parity of its samples flips inside it
TINY = (4, 2, 18, 6)
WINDOWS = S.WINDOWS + [TINY]
SIZES = S.SIZES
FORMATS = narrow_ref.FORMATS
MODES = narrow_ref.MODES
REFUSAL = b"8-bit output of a stream with more than 8 bits per sample (only narrowing of 8-bit content, vvdecimpl.cpp:853)"
ALL_STRIDES = tuple((s, m) for s in S.STRIDES for m in (0, 2))


def set_mode(L, ctx, mode, phase=0):
    assert L.vvr_set_output_narrowing(ctx, mode, phase) == abi.VVR_OK, L.vvr_last_error(ctx)


def feasible(win, size):
    """the rule of every rescaled request: output sides within 1/8 .. 8 times the window's, plane by plane"""
    return size is None or all(a <= 8 * b and b <= 8 * a for s in (0, 1) for a, b in ((win[2] >> s, size[0] >> s), (win[3] >> s, size[1] >> s)))


def base_cases(bd):
    """(window, size, grain): every window plain and at both sizes - but the one pair the rescaler refuses, 18 samples to 300 - and, at 10 bits,
    with grain on the windows wider than 128, alone and with each size"""
    out = [(win, size, False) for win in WINDOWS for size in SIZES if feasible(win, size)]
    if bd == 10:
        out += [(win, size, True) for win in WINDOWS if win[2] > 128 for size in SIZES]
    return out


def cases(bd):
    """(window, size, grain, format, mode, phase, collocated): the six formats on every base case; the modes - DITHER at its four phases - move on
    by one from format to format and from case to case, the chroma positions come round every four cases"""
    out = []
    for n, (win, size, grain) in enumerate(base_cases(bd)):
        for j, fmt in enumerate(FORMATS):
            mode, phase = MODES[(n + j) % len(MODES)]
            out.append((win, size, grain, fmt, mode, phase, (bool(n & 1), bool(n & 2))))
    return out


def instantiations():
    """(window, format, mode, phase, collocated) straight from the slot: every format at every chroma position it has (four for yuv444p8, the two
    vertical ones at 4:2:2, one for planar8 / nv12) on two windows whose rows are stored whole, one whose rows are stored pixel pair by pixel
    pair, the modes taking turns - and on the window of 18 x 6 in every mode and phase"""
    out, n = [], 0
    for win in RGB.STRAIGHT + [TINY]:
        for fmt in FORMATS:
            for c in range(4):
                if (c and fmt in ("planar8", "nv12")) or (c & 1 and fmt != "yuv444p8"):
                    continue
                for mode, phase in (MODES if win == TINY else [MODES[n % len(MODES)]]):
                    out.append((win, fmt, mode, phase, (bool(c & 1), bool(c & 2))))
                n += 1
    return out


SPECIAL_AT = ((6, 8), (1, 4))      # first row and column of the planted block: luma, chroma - inside every window


def specials(bd):
    return [0, 1, 2, 3] + [(1 << bd) - k for k in (4, 3, 2, 1)]


def plant(picture, bd):
    """4 x 16 samples of every plane take the values 0 .. 3 and 2^bd - 4 .. 2^bd - 1 in turn, at both parities of column and row: without the top
    ones a missing min( 255, . ) passes"""
    sp = specials(bd)
    for c, p in enumerate(picture):
        r0, c0 = SPECIAL_AT[1 if c else 0]
        for j in range(4):
            for i in range(16):
                p[r0 + j, c0 + i] = sp[(i + 3 * j) % 8]
    return picture


def assert_planted(picture, bd):
    """every special value is in every plane of the picture, in its crop to every window (the chroma of the 18 x 6 window has room for seven of the
    eight), and a top value lies at an odd column of an odd row and at an even column of an even row"""
    for c, p in enumerate(picture):
        assert set(specials(bd)) <= set(np.unique(p).tolist()), c
    for win in WINDOWS:
        for c, p in enumerate(S.crop(picture, win)):
            found = set(specials(bd)) & set(np.unique(p).tolist())
            assert len(found) >= (7 if win == TINY and c else 8), (win, c, found)
            top = np.argwhere(np.asarray(p) >= (1 << bd) - 3)
            assert {(int(j) & 1, int(i) & 1) for j, i in top} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (win, c)


def same_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in range(len(want)):
        g, w_ = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), "%s, plane %d: %d bytes differ" % (what, k, int((g != w_).sum()))


def sibling(L, ctx, fmt, win, size, grain, seed, col, ncomp=3):
    """the planes of the 16-bit sibling request of the same window, size, grain and seed (the mode does not touch them: checked in the state tests)"""
    if seed is not None:
        assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    return Q.queued(L, ctx, 0, win, narrow_ref.SIBLING[fmt], ncomp, size=size, col=col, grain=grain)


def check_instantiations(L, ctx, picture, bd, device=S.device_request):
    """each into pageable memory and into device memory with rows back to back (the kernel's own store where the base is aligned; the last piece
    of a plane of 18 x 6, 9 x 3 or 202 x 38 bytes is a partial store there).  Straight from the slot the sibling's planes are also the crop of
    the picture that was written (planar8, nv12: checked)"""
    sib = {}
    for win, fmt, mode, phase, col in instantiations():
        what = "%s at %d bits straight from the slot, window %r mode %d phase %d collocated %r" % (fmt, bd, win, mode, phase, col)
        key = (win, narrow_ref.SIBLING[fmt], col)
        if key not in sib:
            sib[key] = sibling(L, ctx, fmt, win, None, False, None, col)
            if key[1] == "planar16":
                same_bytes(sib[key], S.crop(picture, win), "planar16 is the crop, " + what)
        want = narrow_ref.narrow(sib[key], bd, fmt, mode, phase)
        set_mode(L, ctx, mode, phase)
        same_bytes(Q.queued(L, ctx, 0, win, fmt, 3, col=col), want, what + ", pageable")
        device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=None, size=None, grain=False, stride_kind="row", mis=0, col=col)


def check_matrix(L, ctx, picture, bd, device=S.device_request, strides=ALL_STRIDES):
    """every case into pageable destinations with padded rows, into memory of vvr_host_alloc and into device memory; the strides and bases
    rotate over the requests"""
    sib, turn = {}, 0
    for n, (win, size, grain, fmt, mode, phase, col) in enumerate(cases(bd)):
        what = "%s at %d bits, window %r size %r grain %r mode %d phase %d collocated %r" % (fmt, bd, win, size, grain, mode, phase, col)
        seed = 8000 + n // len(FORMATS)
        if n % len(FORMATS) == 0:
            sib = {}
        s16 = narrow_ref.SIBLING[fmt]
        if s16 not in sib:
            sib[s16] = sibling(L, ctx, fmt, win, size, grain, seed, col)
        want = narrow_ref.narrow(sib[s16], bd, fmt, mode, phase)
        set_mode(L, ctx, mode, phase)
        for alloc in (None, lambda nb: L.vvr_host_alloc(ctx, nb)):
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            got = Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain, alloc=alloc)      # (checks the padding of every row)
            same_bytes(got, want, "%s, %s" % (what, "pinned" if alloc else "pageable"))
        stride_kind, mis = strides[turn % len(strides)]
        turn += 1
        device(L, ctx, 0, win, fmt, 3, want, "%s, device, stride %s, base + %d" % (what, stride_kind, mis), seed=seed, size=size, grain=grain, stride_kind=stride_kind, mis=mis, col=col)


def planes_of(fmt, got):
    """Y, Cb, Cr of the planes a request of `fmt` stored"""
    if fmt == "nv12":
        return [got[0], got[1][:, 0::2], got[1][:, 1::2]]
    if fmt in ("uyvy", "yuy2"):
        p, = got
        return [np.stack([p[:, 1::4], p[:, 3::4]], 2).reshape(p.shape[0], -1), p[:, 0::4], p[:, 2::4]] if fmt == "uyvy" else \
               [np.stack([p[:, 0::4], p[:, 2::4]], 2).reshape(p.shape[0], -1), p[:, 1::4], p[:, 3::4]]
    return list(got)


def check_cells_add_up(L, ctx, write, values=(0, 1, 2, 3, 517, 1018, 1019, 1020)):
    """10 bits, DITHER: a plane of constant v <= 1020 stores bytes whose sum over every aligned 2 x 2 cell of the plane is exactly v, at every
    phase - in every plane of every format (the upsampled chroma of a constant plane is the constant).  Leaves its last picture in slot 0."""
    win = (8, 4, 200, 64)
    for v in values:
        write(ctx, 0, [np.full((H_ >> s, W >> s), v, np.uint16) for s in (0, 1, 1)])
        for phase in range(4):
            set_mode(L, ctx, narrow_ref.DITHER, phase)
            for fmt in FORMATS:
                for k, p in enumerate(planes_of(fmt, Q.queued(L, ctx, 0, win, fmt, 3))):
                    p = p.astype(np.int64)
                    cells = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
                    assert (cells == v).all(), (v, phase, fmt, k, np.unique(cells))


def check_multiples_of_4(L, ctx, write, rng):
    """10 bits: a picture of multiples of 4 stores v / 4 in all three modes and at every phase (luma of every format; chroma where it is not
    interpolated).  Leaves its picture in slot 0."""
    picture = [(rng.integers(0, 256, (H_ >> s, W >> s)) * 4).astype(np.uint16) for s in (0, 1, 1)]
    write(ctx, 0, picture)
    for win in ((2, 6, 202, 38), TINY):
        want = [(p >> 2).astype(np.uint8) for p in S.crop(picture, win)]
        for mode, phase in MODES:
            set_mode(L, ctx, mode, phase)
            for fmt in FORMATS:
                got = planes_of(fmt, Q.queued(L, ctx, 0, win, fmt, 3))
                same_bytes(got[:1] if fmt not in ("planar8", "nv12") else got, want[:1] if fmt not in ("planar8", "nv12") else want, "multiples of 4, %s mode %d phase %d %r" % (fmt, mode, phase, win))


def check_truncate_and_luma(L, ctx, bd, grain_ok):
    """TRUNCATE is planar16 >> s (plain, rescaled, grained); the luma of nv12, yuv444p8 and yuv422p8 is planar8's in every mode"""
    s = bd - 8
    for n, (win, size, grain) in enumerate([((2, 6, 202, 38), None, False), (TINY, (134, 26), False), ((8, 4, 200, 64), (300, 96), True), ((6, 2, 144, 34), None, True)]):
        if grain and not grain_ok:
            continue
        p16 = sibling(L, ctx, "planar8", win, size, grain, 8500 + n, (True, False))
        set_mode(L, ctx, narrow_ref.TRUNCATE, 0)
        assert L.vvr_set_film_grain_seed(ctx, 8500 + n) == abi.VVR_OK
        same_bytes(Q.queued(L, ctx, 0, win, "planar8", 3, size=size, grain=grain), [(p >> s).astype(np.uint8) for p in p16], "truncate %r %r %r" % (win, size, grain))
        for mode, phase in MODES:
            set_mode(L, ctx, mode, phase)
            luma = []
            for fmt in ("planar8", "nv12", "yuv444p8", "yuv422p8"):
                assert L.vvr_set_film_grain_seed(ctx, 8500 + n) == abi.VVR_OK
                luma.append(Q.queued(L, ctx, 0, win, fmt, 3, size=size, grain=grain)[0])
            assert all(np.array_equal(luma[0], l_) for l_ in luma[1:]), (win, size, grain, mode, phase)


def check_out_of_range_words(L, ctx, write, rng):
    """words beyond the bit depth (vvr_write_plane stores anything) leave as 255 in every mode: the luma of every format, and the chroma where
    it is not interpolated.  Leaves its picture in slot 0."""
    picture = [rng.choice(np.array([1024, 4095, 65535], np.uint16), (H_ >> s, W >> s)) for s in (0, 1, 1)]
    write(ctx, 0, picture)
    for win in ((8, 4, 200, 64), TINY):
        for mode, phase in MODES:
            set_mode(L, ctx, mode, phase)
            for fmt in FORMATS:
                got = planes_of(fmt, Q.queued(L, ctx, 0, win, fmt, 3))
                for p in (got if fmt in ("planar8", "nv12") else got[:1]):
                    assert (p == 255).all(), (fmt, mode, phase, win)


def _setup(L, bd, seed):
    return S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, plant(p, bd)), np.random.default_rng(seed), bd)


# ---- the restatement and the cases

def test_the_restatement_on_known_samples():
    """the formula by hand: 10 bits, the cell { { 0, 2 }, { 3, 1 } } at phase 0, moved by a column (1), a row (2), both (3); 9 bits: >> 1"""
    v = np.array([[1023, 1023, 5, 6], [1021, 1022, 7, 4]])
    assert narrow_ref.reduce(v, 10, narrow_ref.TRUNCATE, 0).tolist() == [[255, 255, 1, 1], [255, 255, 1, 1]]
    assert narrow_ref.reduce(v, 10, narrow_ref.ROUND, 0).tolist() == [[255, 255, 1, 2], [255, 255, 2, 1]]
    assert narrow_ref.reduce(v, 10, narrow_ref.DITHER, 0).tolist() == [[255, 255, 1, 2], [255, 255, 2, 1]]      # a: 0 2 0 2 / 3 1 3 1
    assert narrow_ref.reduce(v, 10, narrow_ref.DITHER, 1).tolist() == [[255, 255, 1, 1], [255, 255, 2, 1]]      # a: 2 0 2 0 / 1 3 1 3
    assert narrow_ref.reduce(v, 10, narrow_ref.DITHER, 2).tolist() == [[255, 255, 2, 1], [255, 255, 1, 1]]      # a: 3 1 3 1 / 0 2 0 2
    assert narrow_ref.thresholds((2, 2), 10, narrow_ref.DITHER, 3).tolist() == [[1, 3], [2, 0]]
    assert narrow_ref.thresholds((2, 3), 9, narrow_ref.DITHER, 0).tolist() == [[0, 1, 0], [1, 0, 1]] and narrow_ref.thresholds((1, 2), 9, narrow_ref.ROUND, 0).tolist() == [[1, 1]]
    assert narrow_ref.reduce(np.array([[511, 510, 3]]), 9, narrow_ref.DITHER, 1).tolist() == [[255, 255, 2]]
    # nv12: the Cb and the Cr of a pair share the pair's column; uyvy / yuy2: the byte order of yuv_ref at 8 bits
    y, cb, cr = np.zeros((2, 4), np.int64), np.array([[2, 2]]), np.array([[2, 2]])
    assert narrow_ref.narrow([y, cb, cr], 10, "nv12", narrow_ref.DITHER, 0)[1].tolist() == [[0, 0, 1, 1]]
    rng = np.random.default_rng(180)
    p = [rng.integers(0, 256, (4, 8)), rng.integers(0, 256, (4, 4)), rng.integers(0, 256, (4, 4))]
    for fmt in ("uyvy", "yuy2"):
        want, = yuv_ref.yuv([p[0], p[1][0::2], p[2][0::2]], 8, fmt, (True, True))
        got, = narrow_ref.pack422(*[a.astype(np.uint8) for a in p], fmt)
        assert np.array_equal(got[0::2], want[0::2]), fmt      # (the rows yuv_ref does not interpolate)


def test_the_cases_meet_what_they_should():
    for bd in (10, 9):
        cs = cases(bd)
        assert set((c[3], c[4], c[5]) for c in cs) == set((f, m, p) for f in FORMATS for m, p in MODES)
        assert set((c[3], c[1]) for c in cs) == set((f, s) for f in FORMATS for s in SIZES)
        assert set((c[3], c[0]) for c in cs) == set((f, w_) for f in FORMATS for w_ in WINDOWS)
        assert set(c[6] for c in cs if c[3] == "yuv444p8") == set((a, b) for a in (False, True) for b in (False, True))
        assert any(c[2] for c in cs) == (bd == 10) and all(c[0][2] > 128 for c in cs if c[2])
    # the one pair of the matrix that cannot be: 18 samples to 300 is beyond the rescaler's 8 times (refused: test_state_and_refusals); chroma width 67 is odd
    assert [(w_, s) for w_ in WINDOWS for s in SIZES if not feasible(w_, s)] == [(TINY, (300, 96))] and (134 >> 1) & 1
    inst = instantiations()
    assert set((f, c if f == "yuv444p8" else c[1], w_[2] % 8 == 0) for w_, f, _, _, c in inst if f not in ("planar8", "nv12")) == \
        set((f, c, whole) for f in ("yuv444p8",) for c in [(a, b) for a in (False, True) for b in (False, True)] for whole in (False, True)) | \
        set((f, c, whole) for f in ("yuv422p8", "uyvy", "yuv422p8", "yuy2") for c in (False, True) for whole in (False, True))      # 20 new instantiations of k_output_yuv
    assert set((f, m, p) for w_, f, m, p, _ in inst if w_ == TINY) == set((f, m, p) for f in FORMATS for m, p in MODES)


@pytest.mark.parametrize("bd", [10, 9])
def test_the_picture_holds_the_ends_of_the_range(bd):
    picture = plant(film_grain_ref.grain_picture(np.random.default_rng(181), W, H_, bd, 1), bd)
    assert_planted(picture, bd)


# ---- the queue

@pytest.mark.parametrize("bd", [10, 9])
def test_every_instantiation_straight_from_the_slot(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 182 + bd)
    assert_planted(picture, bd)
    check_instantiations(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 9])
def test_narrow_matrix(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 184 + bd)
    assert_planted(picture, bd)
    check_matrix(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_the_bytes_of_a_dithered_cell_add_up_to_the_sample():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    check_cells_add_up(L, ctx, SUP.writer(L))
    L.vvr_destroy(ctx)


def test_multiples_of_4_leave_as_their_quarter():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    check_multiples_of_4(L, ctx, SUP.writer(L), np.random.default_rng(186))
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 9])
def test_truncate_is_a_shift_and_the_luma_is_planar8s(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 187 + bd)
    check_truncate_and_luma(L, ctx, bd, bd == 10)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 9])
def test_out_of_range_words_leave_as_255(bd):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    check_out_of_range_words(L, ctx, SUP.writer(L), np.random.default_rng(189))
    L.vvr_destroy(ctx)


# ---- state

def check_state(L, ctx, picture, bd):
    """the mode is context state: refused when none is set - today's text - , accepted under one, refused again; a bad mode or phase changes
    nothing; the formats it is not looked at for store what they store without it"""
    win = (8, 4, 200, 64)

    def refused(fmt):
        t, _ = Q.submit(L, ctx, 0, win, fmt, 3)
        assert t == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx) == b"vvr_output_submit: " + REFUSAL, (fmt, t, L.vvr_last_error(ctx))

    set_mode(L, ctx, narrow_ref.REFUSE)
    p16 = Q.queued(L, ctx, 0, win, "planar16", 3)
    others = {fmt: Q.queued(L, ctx, 0, win, fmt, 3) for fmt in ("planar16", "p010", "yuv444p16", "y210") + (("v210", "packed10") if bd == 10 else ())}
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    others["rgb8"] = Q.queued(L, ctx, 0, win, "rgb8", 3)
    for fmt in FORMATS:
        refused(fmt)
    set_mode(L, ctx, narrow_ref.DITHER, 0)
    for fmt in FORMATS:
        same_bytes(planes_of(fmt, Q.queued(L, ctx, 0, win, fmt, 3))[:1], [narrow_ref.reduce(p16[0], bd, narrow_ref.DITHER, 0)], fmt)
    set_mode(L, ctx, narrow_ref.REFUSE, 0)
    for fmt in FORMATS:
        refused(fmt)
    # a mode or a phase outside 0 .. 3: VVR_ERR_PARAMETER with a text, and the value set before stays
    set_mode(L, ctx, narrow_ref.DITHER, 2)
    for mode, phase in ((4, 0), (-1, 0), (1, 4), (3, -1), (255, 255)):
        assert L.vvr_set_output_narrowing(ctx, mode, phase) == abi.VVR_ERR_PARAMETER and b"vvr_set_output_narrowing: " in L.vvr_last_error(ctx), (mode, phase)
        same_bytes(Q.queued(L, ctx, 0, win, "planar8", 3), narrow_ref.narrow(p16, bd, "planar8", narrow_ref.DITHER, 2), "after the refused ( %d, %d )" % (mode, phase))
    # every other format: the same bytes under every mode
    for mode, phase in MODES:
        set_mode(L, ctx, mode, phase)
        for fmt, want in others.items():
            same_bytes(Q.queued(L, ctx, 0, win, fmt, 3), want, "%s under mode %d phase %d" % (fmt, mode, phase))
    # a request submitted before a change keeps its mode
    set_mode(L, ctx, narrow_ref.TRUNCATE)
    t1, o1 = Q.submit(L, ctx, 0, win, "nv12", 3)
    set_mode(L, ctx, narrow_ref.DITHER, 3)
    t2, o2 = Q.submit(L, ctx, 0, win, "nv12", 3)
    set_mode(L, ctx, narrow_ref.ROUND)
    assert t1 >= 0 and t2 >= 0
    same_bytes(Q.collect(L, ctx, t2, o2), narrow_ref.narrow(p16, bd, "nv12", narrow_ref.DITHER, 3), "the second request")
    same_bytes(Q.collect(L, ctx, t1, o1), narrow_ref.narrow(p16, bd, "nv12", narrow_ref.TRUNCATE, 0), "the first request")


@pytest.mark.parametrize("bd", [10, 9])
def test_the_mode_is_context_state(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 190 + bd)
    check_state(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_a_context_of_8_bits_ignores_the_mode():
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 8, 192)
    win = (2, 6, 202, 38)
    before = {fmt: Q.queued(L, ctx, 0, win, fmt, 3) for fmt in FORMATS}
    same_bytes(before["nv12"], S.semi(S.crop(picture, win), "nv12", 8), "nv12 at 8 bits")
    for mode, phase in MODES:
        set_mode(L, ctx, mode, phase)
        for fmt in FORMATS:
            same_bytes(Q.queued(L, ctx, 0, win, fmt, 3), before[fmt], "%s at 8 bits under mode %d phase %d" % (fmt, mode, phase))
    L.vvr_destroy(ctx)


def test_400_contexts():
    """planar8 of a 4:0:0 context at 10 bits is accepted, luma alone; the formats that need chroma stay refused under a mode"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(193)
    ctx = SUP.make_ctx(L, W, H_, 10, 0)
    luma = plant([rng.integers(0, 1024, (H_, W)).astype(np.uint16)], 10)
    SUP.write_picture(L, ctx, 0, luma)
    t, _ = Q.submit(L, ctx, 0, TINY, "planar8", 1)
    assert t == abi.VVR_ERR_PARAMETER and REFUSAL in L.vvr_last_error(ctx)
    for win in (TINY, (2, 6, 202, 38)):
        for mode, phase in MODES:
            set_mode(L, ctx, mode, phase)
            same_bytes(Q.queued(L, ctx, 0, win, "planar8", 1), [narrow_ref.reduce(S.crop(luma, win)[0], 10, mode, phase)], "4:0:0 %r mode %d phase %d" % (win, mode, phase))
            S.device_request(L, ctx, 0, win, "planar8", 1, [narrow_ref.reduce(S.crop(luma, win)[0], 10, mode, phase)], "4:0:0, device", stride_kind="row", mis=0)
    for fmt, text in [("nv12", b"no chroma to interleave")] + [(f, b"no chroma to upsample") for f in ("yuv444p8", "yuv422p8", "uyvy", "yuy2")]:
        t, _ = Q.submit(L, ctx, 0, (8, 4, 200, 64), fmt, 3)
        assert t == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(ctx), (fmt, L.vvr_last_error(ctx))
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_and_the_seed_chain_alone():
    """what vvr_output_submit refuses stays refused under a mode - with its own text - and a refused request takes neither a ring entry nor a
    frame of the seed chain"""
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 10, 194)
    win = (8, 4, 200, 64)

    def refused(text, c=ctx, fmt="nv12", mutate=None, size=None, grain=False, w_=win):
        shapes, dt = abi.output_plane_shapes(w_, fmt, size, 3)
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, w_, fmt, size, (True, False), grain, True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c), (text, rc, L.vvr_last_error(c))

    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    for fmt in FORMATS:
        refused(REFUSAL, fmt=fmt, grain=True)      # (no mode set)
    set_mode(L, ctx, narrow_ref.DITHER, 1)
    # grain at 9 bits
    ctx9 = SUP.make_ctx(L, W, H_, 9, 1)
    set_mode(L, ctx9, narrow_ref.ROUND)
    assert L.vvr_set_film_grain(ctx9, C.addressof(bank)) == abi.VVR_OK
    for fmt in FORMATS:
        refused(b"film grain needs a bit depth of 8 or 10", c=ctx9, fmt=fmt, grain=True)
    L.vvr_destroy(ctx9)
    for fmt in FORMATS:
        refused(b"wider than 128", fmt=fmt, grain=True, w_=(0, 0, 128, 64))
        refused(b"outside the picture, or odd", fmt=fmt, grain=True, w_=(0, 0, 201, 64))
        refused(b"1/8", fmt=fmt, grain=True, size=(8, 64))
        refused(b"1/8", fmt=fmt, w_=TINY, size=(300, 96))      # (the pair the matrix leaves out)
        refused(b"missing plane", fmt=fmt, grain=True, mutate=lambda r: r.dst.__setitem__(0, None))
        refused(b"stride below the output's row", fmt=fmt, grain=True, mutate=lambda r: r.dst_stride_bytes.__setitem__(0, 198))
    for fmt in ("yuv444p8", "yuv422p8", "uyvy", "yuy2"):
        refused(b"even out_w and out_h", fmt=fmt, size=(301, 96), grain=True)
    # the ring is untouched: eight requests still fit; the chain too: the first of them is the frame of seed 9
    flight = [Q.submit(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(8)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    got = [Q.collect(L, ctx, t, outs) for t, outs in flight]
    assert all(np.array_equal(a, b_) for a, b_ in zip(got[0], first))
    # an accepted grained request takes one frame of the chain, as its sibling does
    assert L.vvr_set_film_grain_seed(ctx, 33) == abi.VVR_OK
    a = [Q.queued(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(2)]
    assert L.vvr_set_film_grain_seed(ctx, 33) == abi.VVR_OK
    same_bytes(Q.queued(L, ctx, 0, win, "planar8", 3, grain=True), narrow_ref.narrow(a[0], 10, "planar8", narrow_ref.DITHER, 1), "first frame of the chain")
    same_bytes(Q.queued(L, ctx, 0, win, "planar16", 3, grain=True), a[1], "second frame of the chain")
    L.vvr_destroy(ctx)


def test_python_mirror():
    import vvdec_amd
    assert (abi.NARROW_REFUSE, abi.NARROW_TRUNCATE, abi.NARROW_ROUND, abi.NARROW_DITHER) == (0, 1, 2, 3)
    assert abi.NARROW_MODES == {"refuse": 0, "truncate": 1, "round": 2, "dither": 3} and list(abi.OUT_NARROWED) == FORMATS
    assert "vvr_set_output_narrowing" in vvdec_amd.EXPORTED_SYMBOLS and hasattr(SUP.stub_lib(), "vvr_set_output_narrowing")
    assert hasattr(vvdec_amd.Reconstructor, "set_output_narrowing")
    # the shapes and dtypes of the six formats do not depend on the bit depth: bytes
    win = (2, 6, 202, 38)
    assert abi.output_plane_shapes(win, "planar8", None, 3) == ([(38, 202), (19, 101), (19, 101)], np.uint8) and abi.output_plane_shapes(win, "planar8", None, 1) == ([(38, 202)], np.uint8)
    assert abi.output_plane_shapes(win, "nv12", (134, 26), 3) == ([(26, 134), (13, 134)], np.uint8)
    assert abi.output_plane_shapes(TINY, "yuv422p8", None, 3) == ([(6, 18), (6, 9), (6, 9)], np.uint8) and abi.output_plane_shapes(TINY, "uyvy", None, 3) == ([(6, 36)], np.uint8)
