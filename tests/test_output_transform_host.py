"""CPU: the colour transform of the RGB formats of the output queue (vvr_set_output_transform, vvr_output_transform_preset) on the stand-in runtime
of tests/hoststub, where launch_output_rgb is a plain loop (vvr_output.inc, host only).  The expected bytes come from tests/colour_transform_ref.py,
a numpy restatement of the three stages and the stores as include/vvr.h defines them, applied the way tests/test_output_rgb_host.py builds its
expectation: for plain windows to the crop of the picture the test wrote, with grain or a size to the planes of the planar16 request of the same
window, size, grain and seed.  The preset's tables are compared with float64 formulas written from the standards, and the whole integer pipeline
under them with the real-valued one.  The helpers take a library and a context, so tests/output_transform_on_the_device.py runs the same cases on
the device."""
import ctypes as C

import numpy as np
import pytest

import colour_transform_ref as X
import film_grain_ref
import output_support as SUP
import rgb_ref
import test_host_glue as T
import test_output_queue_host as Q
import test_output_rgb_host as R
import test_output_semiplanar_host as S
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = S.W, S.H_
FORMATS, STRAIGHT = R.FORMATS, R.STRAIGHT
COLOUR = (9, 0)       # BT.2020 non-constant luminance, limited range: what HDR video is


def _setup(L, bd, seed):
    return S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(seed), bd)


def set_transform(L, ctx, transform):
    t = None if transform is None else abi.output_transform(*transform)
    assert L.vvr_set_output_transform(ctx, None if t is None else C.addressof(t)) == abi.VVR_OK, L.vvr_last_error(ctx)      # (copied: t may go)


def both_ways(L, ctx, win, fmt, col, want, what, device, size=None, grain=False, seed=None):
    """the request into pageable memory (padded rows) and into device memory with rows back to back, compared with `want`"""
    if seed is not None:
        assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    R.same_bytes(Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain), want, what + ", pageable")
    device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=seed, size=size, grain=grain, stride_kind="row", mis=0, col=col)


# ---- the cases; tests/output_transform_on_the_device.py runs them on the device

def check_identity(L, ctx, picture, bd, device=S.device_request):
    """lin[v] = v, the unit matrix, enc[i] = min( 64 i, 65535 ): stage 3 is exact for this table below 65472, so rgb16 under it is plain rgb16"""
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    for n, win in enumerate(STRAIGHT):
        col = (bool(n & 1), bool(n & 2))
        set_transform(L, ctx, None)
        plain = Q.queued(L, ctx, 0, win, "rgb16", 3, col=col)
        R.same_bytes(plain, rgb_ref.rgb(S.crop(picture, win), bd, "rgb16", COLOUR[0], bool(COLOUR[1]), col), "plain rgb16 %r" % (win,))
        set_transform(L, ctx, X.identity(bd))
        both_ways(L, ctx, win, "rgb16", col, plain, "rgb16 at %d bits under the identity, window %r" % (bd, win), device)
    set_transform(L, ctx, None)


def random_cases(bd):
    """(window, size, grain, format, collocated, colour): every format at every chroma position on the three windows straight from the slot (rows
    stored whole and pair by pair); once behind a rescale and once - bit depths with grain - behind grain and a rescale"""
    out = []
    for win in STRAIGHT:
        for fmt in FORMATS:
            for c in range(4):
                out.append((win, None, False, fmt, (bool(c & 1), bool(c & 2)), R.COLOURS[len(out) % 8]))
    out.append(((8, 4, 200, 64), (300, 96), False, "rgb8", (True, False), COLOUR))
    if bd != 9:
        out.append(((0, 0, 448, 160), (134, 26), True, "rgbf16", (False, True), COLOUR))
    return out


def check_random_tables(L, ctx, picture, bd, device=S.device_request, seed=200):
    rng = np.random.default_rng(seed + bd)
    for n, (win, size, grain, fmt, col, colour) in enumerate(random_cases(bd)):
        what = "%s at %d bits under random tables, window %r size %r grain %r collocated %r colour %r" % (fmt, bd, win, size, grain, col, colour)
        transform = X.random_transform(rng, bd)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        if size is None and not grain:
            planes = S.crop(picture, win)
        else:
            assert L.vvr_set_film_grain_seed(ctx, 6000 + n) == abi.VVR_OK
            planes = Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=grain)
        want = X.rgb(planes, bd, fmt, colour[0], bool(colour[1]), col, transform)
        set_transform(L, ctx, transform)
        both_ways(L, ctx, win, fmt, col, want, what, device, size=size, grain=grain, seed=6000 + n if grain else None)
    set_transform(L, ctx, None)


def check_extremes(L, ctx, picture, bd, device=S.device_request):
    """lin all 65535 with all nine coefficients + 65536, then - 65536: sums of +- 3 * 65536 * 65535, beyond 32 bits; the clip gives 65535 and 0"""
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    _, _, enc = X.identity(bd)
    for sign, top in ((1, 65535), (-1, 0)):
        transform = (np.full(1024, 65535, np.uint16), np.full((3, 3), sign * 65536, np.int64), enc)
        e = X.stages([np.zeros(1, np.int64)] * 3, *transform)
        assert all(int(c[0]) == int(X.stages([np.full(1, top, np.int64)] * 3, np.arange(65536), 16384 * np.eye(3, dtype=np.int64), enc)[0][0]) for c in e)
        set_transform(L, ctx, transform)
        for win, fmt in zip(STRAIGHT, FORMATS):
            want = X.rgb(S.crop(picture, win), bd, fmt, COLOUR[0], bool(COLOUR[1]), (True, False), transform)
            assert all(len(np.unique(p)) == 1 for p in want)
            both_ways(L, ctx, win, fmt, (True, False), want, "%s at %d bits, all coefficients %d" % (fmt, bd, sign * 65536), device)
    set_transform(L, ctx, None)


def check_snapshot_and_scope(L, ctx, picture, bd, p010=True):
    """a request takes the transform that is set when it is submitted; the other formats never see it; NULL restores the plain bytes"""
    rng = np.random.default_rng(300 + bd)
    win, col = (2, 6, 202, 38), (True, False)
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    set_transform(L, ctx, None)
    plain = {fmt: Q.queued(L, ctx, 0, win, fmt, 3, col=col) for fmt in ["rgb16", "planar16"] + (["p010"] if p010 else [])}
    ta, tb = X.random_transform(rng, bd), X.random_transform(rng, bd)
    want = [X.rgb(S.crop(picture, win), bd, "rgb16", COLOUR[0], bool(COLOUR[1]), col, t) for t in (ta, tb)]
    assert not all(np.array_equal(a, b) for a, b in zip(*want))
    set_transform(L, ctx, ta)
    t0, o0 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    set_transform(L, ctx, tb)
    t1, o1 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    others = [(fmt, Q.submit(L, ctx, 0, win, fmt, 3, col=col)) for fmt in plain if fmt != "rgb16"]
    set_transform(L, ctx, None)
    t2, o2 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    assert min(t0, t1, t2) >= 0, L.vvr_last_error(ctx)
    R.same_bytes(Q.collect(L, ctx, t2, o2), plain["rgb16"], "after vvr_set_output_transform( NULL )")
    R.same_bytes(Q.collect(L, ctx, t0, o0), want[0], "the first of two requests in flight")
    R.same_bytes(Q.collect(L, ctx, t1, o1), want[1], "the second of two requests in flight")
    for fmt, (t, o) in others:
        assert t >= 0, L.vvr_last_error(ctx)
        got = Q.collect(L, ctx, t, o)
        assert len(got) == len(plain[fmt]) and all(np.array_equal(a, b) for a, b in zip(got, plain[fmt])), "%s changed under a transform" % fmt


# ---- the restatement

def test_the_restatement_on_values_worked_by_hand():
    lin, m, enc = X.identity()
    e = X.stages([np.array([0, 1, 1023])] * 3, lin, m, enc)
    assert [list(c) for c in e] == [[0, 1, 1023]] * 3
    enc2 = enc.copy()
    enc2[1], enc2[2] = 1000, 3000
    # t = 100: i = 1, f = 36: ( 1000 * 28 + 3000 * 36 + 32 ) >> 6 = 2125
    assert int(X.stages([np.array([100])] * 3, lin, m, enc2)[0][0]) == 2125
    # the stores: 65535 -> 255 and 1.0; 128 -> 0, 129 -> 1 ( ( 129 + 128 ) / 257 ); 1 -> the half subnormal nearest to 1 / 65535
    v = np.array([65535, 128, 129, 1, 0], np.int64)
    assert list(X.store(v, "rgb8")) == [255, 0, 1, 0, 0] and list(X.store(v, "rgb16")) == [65535, 128, 129, 1, 0]
    h = X.store(v, "rgbf16")
    assert h.dtype == np.float16 and h[0] == 1 and h[4] == 0 and h[3].view(np.uint16) == 0x0100
    # 65536 x 65535 x 3 needs more than 32 bits
    assert int(X.stages([np.zeros(1, np.int64)] * 3, np.full(1024, 65535), np.full((3, 3), 65536), enc)[0][0]) == 65534


def test_python_mirror_of_the_struct():
    assert C.sizeof(abi.OutputTransform) == 4 + 4 + 2048 + 36 + 2050 + 6
    assert abi.OutputTransform.lin.offset == 8 and abi.OutputTransform.m.offset == 2056 and abi.OutputTransform.enc.offset == 2092
    lin, m, enc = X.random_transform(np.random.default_rng(1))
    back = abi.output_transform_arrays(abi.output_transform(lin, m, enc))
    assert all(np.array_equal(a, b) for a, b in zip(back, (lin, m, enc)))


# ---- the queue

@pytest.mark.parametrize("bd", [10, 8, 9])
def test_identity_is_plain_rgb16(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 110 + bd)
    check_identity(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8, 9])
def test_random_tables(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 120 + bd)
    check_random_tables(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_the_random_cases_meet_every_instantiation_of_the_kernel():
    met = set((fmt, col, win[2] % 8 == 0) for win, size, grain, fmt, col, _ in random_cases(10) if size is None and not grain)
    assert len(met) == 24
    assert any(size and not grain for _, size, grain, _, _, _ in random_cases(10)) and any(size and grain for _, size, grain, _, _, _ in random_cases(10))


@pytest.mark.parametrize("bd", [10, 8])
def test_extremes_need_64_bits(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 130 + bd)
    check_extremes(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_snapshot_and_scope(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 140 + bd)
    check_snapshot_and_scope(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_transform_in_force():
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 10, 150)
    win, col = (8, 4, 200, 64), (True, False)
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    first = X.random_transform(np.random.default_rng(151))
    want = X.rgb(S.crop(picture, win), 10, "rgb16", COLOUR[0], bool(COLOUR[1]), col, first)
    set_transform(L, ctx, first)
    other = X.random_transform(np.random.default_rng(152))

    def refused(text, mutate):
        t = abi.output_transform(*other)
        mutate(t)
        assert L.vvr_set_output_transform(ctx, C.addressof(t)) == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(ctx), (text, L.vvr_last_error(ctx))
        R.same_bytes(Q.queued(L, ctx, 0, win, "rgb16", 3, col=col), want, "after a refused call (%s)" % text.decode())

    for size in (0, C.sizeof(abi.OutputTransform) - 2, C.sizeof(abi.OutputTransform) + 4):
        refused(b"struct_size", lambda t, size=size: setattr(t, "struct_size", size))
    for k, j, v in [(0, 0, 65537), (2, 1, -65537), (1, 2, 1 << 30), (2, 2, -(1 << 31))]:
        refused(b"matrix entry beyond", lambda t, k=k, j=j, v=v: t.m[k].__setitem__(j, v))
    assert L.vvr_set_output_transform(None, None) == abi.VVR_ERR_PARAMETER
    # the limits themselves are accepted
    edge = (other[0], np.array([[65536, -65536, 0]] * 3), other[2])
    set_transform(L, ctx, edge)
    R.same_bytes(Q.queued(L, ctx, 0, win, "rgb16", 3, col=col), X.rgb(S.crop(picture, win), 10, "rgb16", COLOUR[0], bool(COLOUR[1]), col, edge), "+-65536")
    # a transform in a 4:0:0 context: set, and never met - RGB is refused there as ever
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    set_transform(L, ctx400, first)
    assert L.vvr_set_output_colour(ctx400, 1, 0) == abi.VVR_OK
    shapes, dt = abi.output_plane_shapes(win, "rgb16", None, 3)
    req = abi.output_request(0, None, win, "rgb16", None, col, False, True, [np.zeros(s, dt) for s in shapes])
    assert L.vvr_output_submit(ctx400, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"no chroma" in L.vvr_last_error(ctx400)
    L.vvr_destroy(ctx400)
    L.vvr_destroy(ctx)


# ---- the preset

PRESETS = [(tc, cp, target, peaks, bd) for tc in (16, 18) for cp in (9, 1) for target in (X.TO_SRGB, X.TO_BT709, X.TO_LINEAR)
           for peaks, bd in (((1000., 100.), 10), ((4000., 300.), 8), ((600., 1000.), 9))]


def c_preset(L, tc, cp, target, peaks, bd):
    t = abi.OutputTransform()
    rc = L.vvr_output_transform_preset(C.byref(t), tc, cp, target, peaks[0], peaks[1], bd)
    return rc, t


def test_preset_tables_are_the_standards_formulas():
    """every entry of lin and enc within 1 of the float64 restatement (one pow that differs in its last bit can only move a rounding); the matrix equal"""
    L = SUP.stub_lib()
    for tc, cp, target, peaks, bd in PRESETS:
        rc, t = c_preset(L, tc, cp, target, peaks, bd)
        assert rc == abi.VVR_OK and t.struct_size == C.sizeof(abi.OutputTransform), (tc, cp, target, peaks, bd)
        lin, m, enc = abi.output_transform_arrays(t)
        rl, rm, re = X.preset(tc, cp, target, peaks[0], peaks[1], bd)
        assert np.abs(lin.astype(np.int64) - rl).max() <= 1 and np.abs(enc.astype(np.int64) - re).max() <= 1, (tc, cp, target, peaks, bd)
        assert np.array_equal(m, rm), (cp, m, rm)
        assert (lin[1 << bd:] == 0).all() and lin[0] == 0 and enc[0] == 0 and enc[1024] == 65535 and (np.diff(enc.astype(np.int64)) >= 0).all()
        assert (np.diff(lin[:1 << bd].astype(np.int64)) >= 0).all() and (lin[(1 << bd) - 1] == 65535 or (tc == 16 and peaks[0] < peaks[1]))      # (a source peak below the target's never reaches full scale)
    # the matrix BT.2407 section 2.2 prints to four decimals (the inverse of BT.2087's M2)
    assert np.abs(X.gamut_matrix(9) - np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])).max() <= 0.5e-4
    assert [list(r) for r in X.preset(16, 9, 0)[1]] == [[27205, -9628, -1194], [-2041, 18561, -137], [-297, -1648, 18329]]
    assert np.array_equal(X.preset(16, 1, 0)[1], 16384 * np.eye(3, dtype=np.int64))


def test_preset_refuses_what_it_does_not_know():
    L = SUP.stub_lib()
    for args in [(1, 9, 0, 1000., 100., 10), (14, 9, 0, 1000., 100., 10), (16, 5, 0, 1000., 100., 10), (18, 12, 0, 1000., 100., 10), (16, 9, 3, 1000., 100., 10),
                 (16, 9, -1, 1000., 100., 10), (16, 9, 0, 1000., 100., 11), (18, 9, 0, 1000., 100., 7), (16, 9, 0, 0., 100., 10), (16, 9, 0, 1000., -1., 10),
                 (16, 9, 0, 10001., 100., 10), (16, 9, 0, float("nan"), 100., 10)]:
        t = abi.OutputTransform()
        C.memset(C.addressof(t), 0x5a, C.sizeof(t))
        assert L.vvr_output_transform_preset(C.byref(t), *args) == abi.VVR_ERR_PARAMETER, args
        assert bytes(t) == b"\x5a" * C.sizeof(t), args
    assert L.vvr_output_transform_preset(None, 16, 9, 0, 1000., 100., 10) == abi.VVR_ERR_PARAMETER
    assert c_preset(L, 18, 9, 1, (0., 0.), 10)[0] == abi.VVR_OK      # (HLG ignores the peaks)


def accuracy_inputs():
    """per-channel ramps, the grey ramp and the corners of the cube, at 10 bits"""
    v, z = np.arange(1024), np.zeros(1024, np.int64)
    corners = np.array([[1023 * ((k >> b) & 1) for k in range(8)] for b in range(3)])
    return [np.concatenate(c) for c in zip((v, z, z), (z, v, z), (z, z, v), (v, v, v), corners)]


# the largest distance of the integer pipeline (tables of the float64 restatement) from the real-valued one, in output codes: measured by this
# test, which is deterministic, and rounded up to the next quarter code (DESIGN.md section 5 records the figures)
ACCURACY = {(16, 9, X.TO_SRGB): (0.75, 21.25), (18, 9, X.TO_BT709): (0.75, 11.0)}      # measured: 0.5373 and 21.2019; 0.5071 and 10.9390


@pytest.mark.parametrize("tc,cp,target", sorted(ACCURACY))
def test_preset_accuracy_end_to_end(tc, cp, target):
    rgb = accuracy_inputs()
    e = X.stages(rgb, *X.preset(tc, cp, target, 1000., 100., 10))
    real = X.float_pipeline(rgb, 10, tc, cp, target, 1000., 100.)
    d16 = max(float(np.abs(a - r * 65535).max()) for a, r in zip(e, real))
    d8 = max(float(np.abs(X.store(a, "rgb8").astype(np.float64) - r * 255).max()) for a, r in zip(e, real))
    print("transfer %d primaries %d target %d: largest deviation %.4f 8-bit codes, %.4f 16-bit codes" % (tc, cp, target, d8, d16))
    assert d8 <= ACCURACY[(tc, cp, target)][0] and d16 <= ACCURACY[(tc, cp, target)][1], (d8, d16)
