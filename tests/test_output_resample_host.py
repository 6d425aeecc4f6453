"""CPU: antialiased resampling at the output (vvr_set_output_resampling: area, triangle, Keys cubic; vvr_resample_taps) on the stand-in runtime of
tests/hoststub, where launch_output_resample is a plain loop over the tap tables the host builds (vvr_output.inc, host only).  The expected
samples come from tests/resample_ref.py, a numpy / Python-integer restatement of the definition in include/vvr.h, and every comparison of
samples with it is exact.  The formats behind the resampler are the restatement fed to the existing rgb_ref / yuv_ref / narrow_ref /
interleaved_ref; a grained request is the restatement of the planes the grained planar16 request of the same seed stores at the window's own
size (which its own tests pin to vvdec::FilmGrain).  torch's antialiased interpolate in float64 on the CPU is the outside definition the
triangle and the cubic filter are held against.  The case functions take a library and a context, so tests/test_gpu_output_resample.py and
tests/resample_on_the_device.py run them on the device."""
import ctypes as C

import numpy as np
import pytest

import interleaved_ref
import narrow_ref
import output_support as SUP
import resample_ref as R
import rgb_ref
import yuv_ref
import test_film_grain_host as H
import test_host_glue as T
import test_output_interleaved_host as I
import test_output_queue_host as Q
import test_output_semiplanar_host as S
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = 208, 80
W400, H400 = 136, 8
FILTERS = (R.AREA, R.TRIANGLE, R.CUBIC)
CONTENTS = ("noise", "checker", "flat")
# (window, output): non-integer ratios, chroma 104 x 40 -> 28 x 12; one axis at ratio 1, odd chroma sizes 35 x 17 -> 25 x 17; the 8x limit, two
# output tiles across; a last tile of 18 columns; about 200 cubic taps, more taps than lanes, chroma -> 2 x 1; the 64x limit on both axes for
# luma and chroma, 256 taps
GEOMETRIES = [((0, 0, 208, 80), (56, 24)), ((2, 2, 70, 34), (50, 34)), ((0, 0, 16, 16), (128, 128)), ((0, 0, 208, 80), (210, 82)), ((0, 0, 208, 80), (4, 2)), ((0, 0, 128, 64), (2, 2))]
GEOMETRIES_400 = [((0, 0, 136, 8), (17, 1)), ((3, 0, 131, 8), (262, 16))]
COLLOCATED = [(False, False), (True, False), (False, True), (True, True)]      # the request's `collocated` 0 .. 3
REFUSAL = b"under vvr_set_output_resampling window and output sides must be 1..8192, the output's within 1/64 .. 8 times the window's in every plane"
REFUSAL_REFERENCE = b"output sides must be 1..8192 and within 1/8 .. 8 times the window's"
SWEEP = [(8191, 128), (8192, 128), (1, 8), (2, 16), (17, 9), (1023, 8184), (208, 56), (104, 28), (70, 50), (35, 25), (16, 128), (208, 210), (208, 4), (128, 2), (64, 1), (136, 17), (131, 262), (3840, 224), (2160, 224), (3840, 1920)]


def set_filter(L, ctx, filt):
    assert L.vvr_set_output_resampling(ctx, filt) == abi.VVR_OK, L.vvr_last_error(ctx)


def content(kind, w, h, bd, ncomp, seed=0):
    """fixed-seed noise; a 0 / top checkerboard (cubic overshoot clips at both ends, H goes negative); flat at top"""
    top = (1 << bd) - 1
    shapes = [(h >> s, w >> s) for s in (0, 1, 1)[:ncomp]]
    if kind == "noise":
        rng = np.random.default_rng(500 + seed)
        return [rng.integers(0, top + 1, s).astype(np.uint16) for s in shapes]
    if kind == "checker":
        return [((np.add.outer(np.arange(s[0]), np.arange(s[1])) & 1) * top).astype(np.uint16) for s in shapes]
    return [np.full(s, top, np.uint16) for s in shapes]


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w_) in enumerate(zip(got, want)):
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), "%s, plane %d: %d bytes differ" % (what, k, int((g.view(np.uint8) != w_.view(np.uint8)).sum()))


def check_geometries(L, ctx, write, bd, ncomp):
    """each filter x each geometry x each content, planar samples against the restatement: every geometry with `collocated` 1, the first one at
    every `collocated`.  Flat at top must stay top everywhere.  Leaves the flat picture in slot 0."""
    fmt = "planar16" if bd > 8 else "planar8"
    w, h = (W, H_) if ncomp == 3 else (W400, H400)
    runs = [(g, COLLOCATED[1]) for g in (GEOMETRIES if ncomp == 3 else GEOMETRIES_400)] + ([(GEOMETRIES[0], c) for c in COLLOCATED if c != COLLOCATED[1]] if ncomp == 3 else [])
    for kind in CONTENTS:
        picture = content(kind, w, h, bd, ncomp, bd)
        write(ctx, 0, picture)
        for filt in FILTERS:
            set_filter(L, ctx, filt)
            for (win, size), col in runs:
                what = "%s, filter %d, %d bits, %r -> %r collocated %r" % (kind, filt, bd, win, size, col)
                got = Q.queued(L, ctx, 0, win, fmt, ncomp, size=size, col=col)
                same(got, R.resample(S.crop(picture, win)[:ncomp], filt, size, bd, col), what)
                if kind == "flat":
                    assert all((g == (1 << bd) - 1).all() for g in got), what


def check_formats(L, ctx, write, bd, grain_bank=None, device=S.device_request):
    """the formats behind the resampler on the first geometry, the filters taking turns: the restatement fed to the existing restatements of
    the formats; grain then resample; a destination in vvr_host_alloc memory at a padded stride; a destination in device memory"""
    win, size = GEOMETRIES[0]
    col = (True, False)
    picture = content("noise", W, H_, bd, 3, 40 + bd)
    write(ctx, 0, picture)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert I.set_norm(L, ctx, norm) == abi.VVR_OK
    if bd > 8:
        assert L.vvr_set_output_narrowing(ctx, narrow_ref.DITHER, 1) == abi.VVR_OK
    formats = ["planar16", "p010", "rgb8", "rgbf32", "yuv444p16"] + (["nv12", "v210"] if bd == 10 else []) + (["planar8"] if bd == 8 else [])
    for n, fmt in enumerate(formats):
        filt = FILTERS[n % 3]
        set_filter(L, ctx, filt)
        frame = R.resample(S.crop(picture, win), filt, size, bd, col)
        if fmt in ("planar16", "planar8"):
            want = [p.astype(np.uint16 if fmt == "planar16" else np.uint8) for p in frame]
        elif fmt == "p010":
            want = S.semi(frame, "p010", bd)
        elif fmt == "nv12":
            want = narrow_ref.narrow(frame, bd, "nv12", narrow_ref.DITHER, 1)
        elif fmt == "rgb8":
            want = rgb_ref.rgb(frame, bd, "rgb8", 1, False, col)
        elif fmt == "rgbf32":
            want = interleaved_ref.frame(frame, bd, "rgbf32", 1, False, col, None, norm)
        else:
            want = yuv_ref.yuv(frame, bd, fmt, col)
        what = "%s behind filter %d at %d bits" % (fmt, filt, bd)
        same(Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col), want, what + ", pageable")
        same(Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, alloc=lambda nb: L.vvr_host_alloc(ctx, nb)), want, what + ", vvr_host_alloc at a padded stride")
        device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=None, size=size, grain=False, stride_kind=("row", "row+6")[n & 1], mis=0, col=col)
    if grain_bank is not None:
        assert L.vvr_set_film_grain(ctx, C.addressof(grain_bank)) == abi.VVR_OK
        for n, filt in enumerate(FILTERS):
            set_filter(L, ctx, filt)
            assert L.vvr_set_film_grain_seed(ctx, 77 + n) == abi.VVR_OK
            grained = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
            assert any(not np.array_equal(g, p) for g, p in zip(grained, S.crop(picture, win)))
            assert L.vvr_set_film_grain_seed(ctx, 77 + n) == abi.VVR_OK
            same(Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=True), [p.astype(np.uint16) for p in R.resample(grained, filt, size, bd, col)], "grain, then filter %d" % filt)
            assert L.vvr_set_film_grain_seed(ctx, 77 + n) == abi.VVR_OK
            same(Q.queued(L, ctx, 0, win, "rgb8", 3, size=size, col=col, grain=True), rgb_ref.rgb(R.resample(grained, filt, size, bd, col), bd, "rgb8", 1, False, col), "grain, filter %d, rgb8" % filt)
    assert I.set_norm(L, ctx, None) == abi.VVR_OK


def check_state(L, ctx, write, bd):
    """the filter is context state: a new context has 0; a value outside 0 .. 3 is refused with a text and the value before stays; a request
    keeps the filter it was submitted under"""
    win, size = GEOMETRIES[0]
    fmt = "planar16" if bd > 8 else "planar8"
    picture = content("noise", W, H_, bd, 3, 60 + bd)
    write(ctx, 0, picture)
    want = {f: R.resample(S.crop(picture, win), f, size, bd) for f in FILTERS}
    set_filter(L, ctx, R.CUBIC)
    for bad in (4, -1, 255):
        assert L.vvr_set_output_resampling(ctx, bad) == abi.VVR_ERR_PARAMETER and b"vvr_set_output_resampling: " in L.vvr_last_error(ctx), bad
        same(Q.queued(L, ctx, 0, win, fmt, 3, size=size), want[R.CUBIC], "after the refused %d" % bad)
    set_filter(L, ctx, R.AREA)
    t1, o1 = Q.submit(L, ctx, 0, win, fmt, 3, size=size)
    set_filter(L, ctx, R.TRIANGLE)
    t2, o2 = Q.submit(L, ctx, 0, win, fmt, 3, size=size)
    set_filter(L, ctx, R.CUBIC)
    assert t1 >= 0 and t2 >= 0
    same(Q.collect(L, ctx, t2, o2), want[R.TRIANGLE], "the second request")
    same(Q.collect(L, ctx, t1, o1), want[R.AREA], "the first request")
    # a request at the window's own size does not look at the filter
    same(Q.queued(L, ctx, 0, win, fmt, 3), [p.astype(np.uint16 if bd > 8 else np.uint8) for p in S.crop(picture, win)], "no size")


def check_in_flight(L, ctx, write, bd=10):
    """eight requests of different filters and formats in flight, collected out of order"""
    win, size = GEOMETRIES[0]
    picture = content("noise", W, H_, bd, 3, 70)
    write(ctx, 0, picture)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    flight = []
    for n in range(8):
        filt, fmt = FILTERS[n % 3], ("planar16", "p010", "rgb8", "yuv444p16")[n % 4]
        set_filter(L, ctx, filt)
        t, outs = Q.submit(L, ctx, 0, win, fmt, 3, size=size)
        assert t >= 0, L.vvr_last_error(ctx)
        frame = R.resample(S.crop(picture, win), filt, size, bd)
        want = {"planar16": lambda: [p.astype(np.uint16) for p in frame], "p010": lambda: S.semi(frame, "p010", bd), "rgb8": lambda: rgb_ref.rgb(frame, bd, "rgb8", 1, False, (True, False)),
                "yuv444p16": lambda: yuv_ref.yuv(frame, bd, "yuv444p16", (True, False))}[fmt]()
        flight.append((t, outs, want, "request %d: %s under filter %d" % (n, fmt, filt)))
    assert len(set(f[0] for f in flight)) == 8
    t, _ = Q.submit(L, ctx, 0, win, "planar16", 3, size=size)
    assert t == abi.VVR_ERR_BUSY
    for n in (5, 0, 7, 2, 3, 6, 1, 4):
        t, outs, want, what = flight[n]
        same(Q.collect(L, ctx, t, outs), want, what)


# ---- the restatement and the helper

def test_the_restatement_on_values_worked_by_hand():
    # 2 -> 1, phi 2: n' = 2, m' = 1, S = 8, Q = 4, P = 2, 6: N = 2, 2
    assert R.numerators(R.TRIANGLE, 2, 1, 2, 0) == (0, [6, 6]) and R.taps(R.TRIANGLE, 2, 1, 2, 0) == (0, (8192, 8192))
    assert R.numerators(R.AREA, 2, 1, 2, 0) == (0, [4, 4])
    assert R.numerators(R.CUBIC, 2, 1, 2, 0) == (0, [3 * 8 - 5 * 4 * 8 + 2 * 512] * 2)
    # ratio 1: the identity in all three (cubic: the neighbours' numerators are 0 and stay taps)
    for n in (1, 2, 5):
        for i in range(n):
            assert R.taps(R.TRIANGLE, n, n, 2, i) == (i, (16384,)) and R.taps(R.AREA, n, n, 1, i) == (i, (16384,))
            first, w = R.taps(R.CUBIC, n, n, 2, i)
            assert [first + k for k, v in enumerate(w) if v] == [i] and sum(w) == 16384
    # 4 -> 2 collocated chroma (phi 1): Q = 2, 10; P = 1, 5, 9, 13; S = 8: sample 0 takes 0 (N = 1), 1 (N = 3), and nothing at N = 7 but 1/8
    assert R.numerators(R.TRIANGLE, 4, 2, 1, 0) == (0, [7, 5, 1])
    # the footprints [ -2, 6 ) and [ 6, 14 ) over the boxes ( -inf, 3 ), [ 3, 7 ), [ 7, 11 ), [ 11, inf )
    assert R.numerators(R.AREA, 4, 2, 1, 0) == (0, [5, 3]) and R.numerators(R.AREA, 4, 2, 1, 1) == (1, [1, 4, 3])
    # upwards the cubic has negative lobes; floor towards minus infinity
    first, w = R.taps(R.CUBIC, 16, 128, 2, 61)
    assert len(w) == 4 and w[0] < 0 and w[3] < 0 and sum(w) == 16384
    assert (-3) // 2 == -2


def sweep_samples(m):
    return range(m) if m <= 300 else list(range(40)) + list(range(40, m - 40, 61)) + list(range(m - 40, m))


def test_taps_against_python_integers():
    """vvr_resample_taps over a sweep (8191 -> 128 is the coprime 64-bit worst case), both phi: count <= 256, the weights sum to 16384, the taps
    lie inside the plane and | H | < 32768 at 10 bits - the sum of the positive weights times 1023, rounded, is the largest H there is"""
    L = SUP.stub_lib()
    most = 0
    for n, m in SWEEP:
        assert R.accepted(n, m)
        for filt in FILTERS:
            for phi in (1, 2):
                for i in sweep_samples(m):
                    got = abi.resample_taps(L, filt, n, m, phi, i)
                    assert got is not None, (filt, n, m, phi, i)
                    first, w = got
                    assert (first, tuple(w)) == R.taps(filt, n, m, phi, i), (filt, n, m, phi, i)
                    assert 1 <= len(w) <= 256 and sum(w) == 16384 and first >= 0 and first + len(w) <= n
                    pos, neg = sum(v for v in w if v > 0), -sum(v for v in w if v < 0)
                    assert (pos * 1023 + 512) >> 10 < 32768 and (neg * 1023 + 512) >> 10 < 32768
                    most = max(most, len(w))
    assert most == 256


def test_taps_refusals():
    L = SUP.stub_lib()
    ok = (R.CUBIC, 208, 56, 2, 0)
    assert abi.resample_taps(L, *ok) is not None
    for bad in [(0, 208, 56, 2, 0), (4, 208, 56, 2, 0), (-1, 208, 56, 2, 0), (R.CUBIC, 0, 56, 2, 0), (R.CUBIC, 208, 0, 2, 0), (R.CUBIC, 8193, 8192, 2, 0), (R.CUBIC, 8192, 8193, 2, 0),
                (R.AREA, 129, 2, 2, 0), (R.AREA, 2, 17, 2, 0), (R.CUBIC, 208, 56, 0, 0), (R.CUBIC, 208, 56, 3, 0), (R.CUBIC, 208, 56, 2, -1), (R.CUBIC, 208, 56, 2, 56)]:
        assert abi.resample_taps(L, *bad) is None, bad
    assert abi.resample_taps(L, R.AREA, 128, 2, 2, 1) is not None and abi.resample_taps(L, R.AREA, 2, 16, 1, 15) is not None
    first, w = C.c_int32(), (C.c_int16 * 256)()
    assert L.vvr_resample_taps(R.CUBIC, 208, 56, 2, 0, None, w) == abi.VVR_ERR_PARAMETER and L.vvr_resample_taps(R.CUBIC, 208, 56, 2, 0, C.byref(first), None) == abi.VVR_ERR_PARAMETER


# ---- the queue

@pytest.mark.parametrize("bd", [10, 8])
def test_every_filter_geometry_and_content(bd):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    check_geometries(L, ctx, SUP.writer(L), bd, 3)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_400_contexts(bd):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W400, H400, bd, 0)
    check_geometries(L, ctx, SUP.writer(L), bd, 1)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_formats_behind_the_resampler(bd):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    bank = abi.film_grain_bank(**H._bank(np.random.default_rng(510 + bd)))
    check_formats(L, ctx, SUP.writer(L), bd, bank)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_the_filter_is_context_state(bd):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    check_state(L, ctx, SUP.writer(L), bd)
    L.vvr_destroy(ctx)


def test_eight_requests_in_flight():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    check_in_flight(L, ctx, SUP.writer(L))
    L.vvr_destroy(ctx)


def test_a_context_at_filter_0_is_todays():
    """a new context, and one set back to 0: the bytes of the synchronous rescaler (vvdec::rescalePlane's) and the refusal below 1/8 with
    today's text; under a filter the same request is accepted"""
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    picture = content("noise", W, H_, 10, 3, 80)
    SUP.write_picture(L, ctx, 0, picture)
    win, size = GEOMETRIES[0]
    for turn in range(2):
        same(Q.queued(L, ctx, 0, win, "planar16", 3, size=size), Q.sync_read(L, ctx, 0, win, 2, 3, size=size), "filter 0")
        t, _ = Q.submit(L, ctx, 0, win, "planar16", 3, size=(4, 2))
        assert t == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx) == b"vvr_output_submit: " + REFUSAL_REFERENCE, L.vvr_last_error(ctx)
        set_filter(L, ctx, R.TRIANGLE)
        assert not np.array_equal(Q.queued(L, ctx, 0, win, "planar16", 3, size=size)[0], Q.sync_read(L, ctx, 0, win, 2, 3, size=size)[0])
        assert len(Q.queued(L, ctx, 0, win, "planar16", 3, size=(4, 2))) == 3
        set_filter(L, ctx, R.REFERENCE)
    L.vvr_destroy(ctx)


def test_refusals_per_plane_leave_the_ring_and_the_seed_chain_alone():
    """the limits hold per plane and axis: 130 -> 3 passes the luma test ( 130 <= 64 * 3 ) and fails the chroma one ( 65 > 64 * 1 ); 130 -> 2
    fails both; 128 -> 2 and 128 -> 3 pass.  Upwards 16 -> 128 passes, 16 -> 130 does not.  A refused request takes neither a ring entry nor a
    frame of the seed chain."""
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    picture = content("noise", W, H_, 10, 3, 81)
    SUP.write_picture(L, ctx, 0, picture)
    bank = abi.film_grain_bank(**H._bank(np.random.default_rng(82)))
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    set_filter(L, ctx, R.AREA)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, (0, 0, 208, 80), "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK

    def refused(win, size, grain=False):
        t, _ = Q.submit(L, ctx, 0, win, "planar16", 3, size=size, grain=grain)
        assert t == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx) == b"vvr_output_submit: " + REFUSAL, (win, size, t, L.vvr_last_error(ctx))

    refused((0, 0, 130, 80), (3, 80))
    refused((0, 0, 130, 80), (2, 80))
    refused((0, 0, 208, 80), (3, 80), grain=True)
    refused((0, 0, 208, 80), (208, 1), grain=True)      # (chroma rows: 40 -> 0)
    refused((0, 0, 16, 16), (130, 16))
    refused((0, 0, 16, 16), (16, 8194))
    refused((0, 0, 208, 80), (0, 24))
    for win, size in (((0, 0, 128, 80), (2, 80)), ((0, 0, 128, 80), (3, 80)), ((0, 0, 16, 16), (128, 128))):
        assert len(Q.queued(L, ctx, 0, win, "planar16", 3, size=size)) == 3
    # the ring is untouched: eight requests still fit; the chain too: the first of them is the frame of seed 9
    flight = [Q.submit(L, ctx, 0, (0, 0, 208, 80), "planar16", 3, grain=True) for _ in range(8)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    got = [Q.collect(L, ctx, t, outs) for t, outs in flight]
    assert all(np.array_equal(a, b_) for a, b_ in zip(got[0], first))
    L.vvr_destroy(ctx)


def test_the_synchronous_call_and_a_scaled_comparison_do_not_look_at_the_filter():
    import test_output_scaled_compare_host as SC
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    picture = content("noise", W, H_, 10, 3, 83)
    SUP.write_picture(L, ctx, 0, picture)
    win, size = GEOMETRIES[0]
    before = Q.sync_read(L, ctx, 0, win, 2, 3, size=size)
    cmp_before = scaled_comparison(L, ctx, win, size)
    for filt in FILTERS:
        set_filter(L, ctx, filt)
        same(Q.sync_read(L, ctx, 0, win, 2, 3, size=size), before, "vvr_read_output_scaled under filter %d" % filt)
        assert scaled_comparison(L, ctx, win, size) == cmp_before, filt
    L.vvr_destroy(ctx)


def scaled_comparison(L, ctx, win, size):
    """one comparison under vvr_set_compare_scaling against a fixed reference of the size -> the SSE words of the three components"""
    import test_output_scaled_compare_host as SC
    SC.scaling(L, ctx, size)
    raw, blocks = SC.queued(L, ctx, SC.submit_compare(L, ctx, 0, win, size, SC.words16(content("noise", size[0], size[1], 10, 3, 84))))
    SC.off(L, ctx)
    return C.string_at(C.addressof(raw), C.sizeof(raw)), blocks.tobytes()


# ---- agreement with the outside definition

def _torch_reference(plane, mode, size, bd):
    import torch
    t = torch.from_numpy(np.asarray(plane).astype(np.float64))[None, None]
    out = torch.nn.functional.interpolate(t, size=(size[1], size[0]), mode=mode, antialias=True, align_corners=False)
    return np.clip(out[0, 0].numpy(), 0, (1 << bd) - 1)


@pytest.mark.parametrize("bd", [10, 8])
def test_triangle_and_cubic_are_torchs_antialiased_interpolate(bd):
    """luma of the six geometries, all three contents: max | out - clip( interpolate( ..., antialias = True, align_corners = False ) ) | < 1.0 in
    float64 on the CPU - the integer result never differs from torch's rounded one by more than one code value - and the float64 evaluation of
    the definition's own numerators equals torch's to 1e-9 of the range.  Measured maximum of the first: 0.5663 at 10 bits, 0.5348 at 8 bits."""
    pytest.importorskip("torch")
    worst = 0.0
    for kind in CONTENTS:
        picture = content(kind, W, H_, bd, 1, bd)
        for filt, mode in ((R.TRIANGLE, "bilinear"), (R.CUBIC, "bicubic")):
            for win, size in GEOMETRIES:
                src = S.crop(picture, win)[0]
                want = _torch_reference(src, mode, size, bd)
                exact = np.clip(R.resample_exact(src, filt, size[0], size[1]), 0, (1 << bd) - 1)
                assert np.abs(exact - want).max() < 1e-9 * (1 << bd), (kind, filt, win, size, np.abs(exact - want).max())
                got = R.resample_plane(src, filt, size[0], size[1], bd).astype(np.float64)
                err = np.abs(got - want).max()
                worst = max(worst, err)
                print("%s filter %d %r -> %r at %d bits: %.4f" % (kind, filt, win, size, bd, err))
                assert err < 1.0, (kind, filt, win, size, err)
    print("worst at %d bits: %.4f" % (bd, worst))


@pytest.mark.parametrize("bd", [10, 8])
def test_area_is_its_own_numerators_and_the_block_mean(bd):
    """AREA against the float64 evaluation of its own numerators (the integer pipeline within one code value: measured 0.5385 at 10 bits, 0.5288 at 8), and at integer
    ratios against the plain block mean"""
    worst = 0.0
    for kind in CONTENTS:
        picture = content(kind, W, H_, bd, 1, bd)
        for win, size in GEOMETRIES + [((0, 0, 208, 80), (52, 20)), ((0, 0, 128, 64), (16, 16))]:
            src = S.crop(picture, win)[0]
            exact = R.resample_exact(src, R.AREA, size[0], size[1])
            got = R.resample_plane(src, R.AREA, size[0], size[1], bd).astype(np.float64)
            err = np.abs(got - exact).max()
            worst = max(worst, err)
            assert err < 1.0, (kind, win, size, err)
            if src.shape[1] % size[0] == 0 and src.shape[0] % size[1] == 0:
                fy, fx = src.shape[0] // size[1], src.shape[1] // size[0]
                mean = src.astype(np.float64).reshape(size[1], fy, size[0], fx).mean(axis=(1, 3))
                assert np.abs(exact - mean).max() < 1e-9 * (1 << bd), (kind, win, size)
    print("worst at %d bits: %.4f" % (bd, worst))


def test_python_mirror():
    import vvdec_amd
    assert (abi.RESAMPLE_REFERENCE, abi.RESAMPLE_AREA, abi.RESAMPLE_TRIANGLE, abi.RESAMPLE_CUBIC) == (0, 1, 2, 3) and abi.RESAMPLE_MAX_TAPS == 256
    assert abi.RESAMPLE_FILTERS == {None: 0, "reference": 0, "area": 1, "triangle": 2, "cubic": 3}
    assert all(s in vvdec_amd.EXPORTED_SYMBOLS and hasattr(SUP.stub_lib(), s) for s in ("vvr_set_output_resampling", "vvr_resample_taps"))
    assert hasattr(vvdec_amd.Reconstructor, "set_output_resampling") and hasattr(vvdec_amd, "resample_taps")
