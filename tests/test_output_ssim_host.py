"""CPU: SSIM of a picture against a reference frame as a request of the output queue (vvr_ssim_submit, collected with vvr_output_test /
vvr_output_wait) and the host helper vvr_compare_ssim, on the stand-in runtime of tests/hoststub, where launch_output_ssim is a plain loop
(vvr_output.inc, host only).  Planes are uploaded with vvr_write_plane.  Expected values: tests/ssim_ref.py, the numpy restatement of the
definition in include/vvr.h.  Every comparison of integers is exact.  The helpers take a library and a context, so
tests/test_gpu_output_ssim.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import compare_ref
import output_support as SUP
import ssim_ref
import test_host_glue as T
import test_output_compare_host as XC
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = 208, 80           # four blocks across with a 16-wide last one, two down with a 16-high last one
WINDOWS = [(0, 0, 208, 80),       # the whole picture
           (8, 4, 200, 64),       # an offset window
           (2, 2, 70, 34),        # odd chroma sizes (35 x 17), an uncovered tail in every component
           (0, 0, 132, 76),       # a last block 4 wide: no window origin falls into it
           (6, 2, 8, 8),          # one luma window, no chroma window
           (0, 0, 16, 16)]        # exactly one window per component
W400, H400 = 136, 8
WINDOWS_400 = [(0, 0, 136, 8), (3, 0, 131, 8)]
CONTENTS = ["identical", "noise", "inverse", "random", "flat", "seam", "last_window", "tail", "two_minima"]
ONE = 1 << 24


def picture_size(cf):
    return (W, H_) if cf else (W400, H400)


def windows(nc):
    return WINDOWS if nc == 3 else WINDOWS_400


def submit(L, ctx, slot, win, ref, with_map=True, job=None, blocking=True, bps=2):
    """one vvr_ssim_submit -> (ticket or error, (the vvr_frame_ssim, the map) vvr_output_wait writes, both filled with 0xaa)"""
    raw = abi.FrameSsim()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    blocks = np.full(abi.ssim_map_shape(win), -0x55555556, np.int32) if with_map else None
    req = abi.ssim_request(slot, job, win, ref, raw, blocks, blocking, bps)
    return L.vvr_ssim_submit(ctx, C.byref(req)), (raw, blocks)


collect = XC.collect


def queued(L, ctx, slot, win, ref, **kw):
    t, keep = submit(L, ctx, slot, win, ref, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, keep)


FIELDS = ("width", "height", "windows_x", "windows_y", "windows", "sum", "min", "min_x", "min_y")


def same(got, want, win, bd, what):
    """every field of the vvr_frame_ssim and every word of the map, exactly"""
    raw, blocks = got
    nc = want["num_components"]
    assert (raw.struct_size, raw.bit_depth, raw.num_components, raw.pad, raw.pad2) == (C.sizeof(abi.FrameSsim), bd, nc, 0, 0), what
    for name in FIELDS:
        assert [int(v) for v in getattr(raw, name)] == want[name], "%s: %s is %r, expected %r" % (what, name, [int(v) for v in getattr(raw, name)], want[name])
    assert want["width"][0] == win[2] and want["height"][0] == win[3]
    if blocks is not None:
        assert np.array_equal(blocks.astype(np.int64), want["map"]), "%s: the map is\n%r, expected\n%r" % (what, blocks, want["map"])
        assert int(blocks.min()) == min(want["min"])


def c_mean(L, raw):
    out = (C.c_double * 4)(-1., -1., -1., -1.)
    return L.vvr_compare_ssim(C.byref(raw) if raw is not None else None, out), list(out)


def reference(kind, rng, part, bd):
    """the reference planes of a window whose slot planes are `part`, as int64 arrays; what each content is there for is asserted in
    check_contents"""
    top = (1 << bd) - 1
    ref = [np.minimum(p.astype(np.int64), top) for p in part]
    nc = len(part)
    if kind in ("identical", "flat"):      # (flat: the slot holds the other level)
        return ref
    if kind == "noise":
        return [np.clip(p + rng.integers(-8, 9, p.shape), 0, top) for p in ref]
    if kind == "inverse":
        return [top - p for p in ref]
    if kind == "random":                   # anything 16 bits hold: values above L are clamped
        return [rng.integers(0, 1 << 16, p.shape, dtype=np.int64) for p in ref]
    if kind == "seam":                     # differences only in luma columns and rows 60 .. 71 (chroma: 30 .. 35): the windows that straddle a block border
        for c in range(nc):
            lo, hi = (30, 36) if c and nc == 3 else (60, 72)
            jj, ii = np.mgrid[0:ref[c].shape[0], 0:ref[c].shape[1]]
            mask = ((ii >= lo) & (ii < hi)) | ((jj >= lo) & (jj < hi))
            ref[c] = np.where(mask, ref[c] ^ 21, ref[c])
        return ref
    if kind == "last_window":              # one sample differs, the last one the last window covers
        for c in range(nc):
            h, w = ref[c].shape
            if w >= 8 and h >= 8:
                ref[c][(h - 8) // 4 * 4 + 7, (w - 8) // 4 * 4 + 7] ^= 32
        return ref
    if kind == "tail":                     # one sample differs in every uncovered column and row there is
        for c in range(nc):
            h, w = ref[c].shape
            cw, ch = ((w - 8) // 4 * 4 + 8 if w >= 8 else 0), ((h - 8) // 4 * 4 + 8 if h >= 8 else 0)
            if cw < w:
                ref[c][0, cw] ^= 32
            if ch < h:
                ref[c][ch, 0] ^= 32
        return ref
    assert kind == "two_minima"            # the slot holds a picture of period 16 in both directions (periodic()); one sample is changed at the same place of
    for c in range(nc):                    # two periods: the windows around ( 8, 24 ) in block ( 0, 0 ) tie with those around ( 88, 8 ) - chroma ( 56, 8 ) - in block
        if two_fit(ref[c].shape, c and nc == 3):      # ( 1, 0 ), which the block order has second and the raster order first
            ref[c][8, (48 if c and nc == 3 else 80) + 8] ^= 16
            ref[c][24, 8] ^= 16
    return ref


def two_fit(shape, chroma):
    return shape[0] >= 32 and shape[1] >= (64 if chroma else 96)


def periodic(planes, win, rng, bd):
    """the picture with the window filled, from its origin on, with copies of a random tile of 16 x 16 samples per component"""
    out = [p.copy() for p in planes]
    for c, p in enumerate(out):
        s = 1 if c and len(planes) == 3 else 0
        x, y, w, h = (v >> s for v in win)
        tile = rng.integers(0, 1 << bd, (16, 16)).astype(np.uint16)
        p[y:y + h, x:x + w] = np.tile(tile, ((h + 15) // 16, (w + 15) // 16))[:h, :w]
    return out


def forms(ref):
    """the forms a reference is given in: 2-byte samples at padded strides; 1-byte samples, when its values fit, at an odd byte stride"""
    return SUP.forms(ref)


def check_contents(L, ctx, write, planes, bd):
    """every content at every window in every form, for the picture `planes` (which this leaves in slot 0)"""
    nc = len(planes)
    top = (1 << bd) - 1
    rng = np.random.default_rng(1400 + bd + nc)
    met = dict(two_minima=0, tail=0, seam=0, negative=0, clamped=0, no_window_word=0, eight_bit=0)
    for win in windows(nc):
        part = compare_ref.window_planes(planes, win)
        same_want = ssim_ref.ssim(part, part, bd)
        for kind in CONTENTS:
            held = part
            if kind == "flat":             # both flat, at different levels: no variance on either side, c = 2^24 and l alone decides
                held = [np.full(p.shape, top // 3 + c, np.uint16) for c, p in enumerate(part)]
                full = [np.full(p.shape, top // 3 + c, np.uint16) for c, p in enumerate(planes)]
                write(ctx, 0, full)
            if kind == "two_minima":
                full = periodic(planes, win, rng, bd)
                write(ctx, 0, full)
                held = compare_ref.window_planes(full, win)
            ref = reference(kind, rng, held, bd)
            if kind == "flat":
                ref = [np.full(p.shape, top // 2 - c, np.int64) for c, p in enumerate(part)]
            want = ssim_ref.ssim(held, ref, bd)
            what = "%s at %d bits, window %r" % (kind, bd, win)
            if kind == "identical":
                assert all(want["sum"][c] == want["windows"][c] * ONE for c in range(3)) and ssim_ref.mean(want)[3] == 1.0 and want["windows"][0] >= 1, what
                assert want["min"][:nc] == [ONE if n else ssim_ref.NO_WINDOW for n in want["windows"][:nc]] and want["min_x"][0] == 0, what
            if kind == "inverse":
                assert all(int(ssim_ref.window_values(a, b, bd).max()) < 0 for a, b in zip(held, ref) if min(a.shape) >= 8), what
                met["negative"] += 1
            if kind == "random":
                assert all(int(p.max()) > top for p in ref), what
                met["clamped"] += 1
            if kind == "flat":
                assert all(want["sum"][c] == want["windows"][c] * want["min"][c] and 0 < want["min"][c] < ONE for c in range(nc) if want["windows"][c]), what
            if kind == "seam":             # (luma windows 14 .. 17 of a row or column of windows hold samples 60 .. 71; the others hold none of them)
                v = ssim_ref.window_values(held[0], ref[0], bd)
                jj, ii = np.mgrid[0:v.shape[0], 0:v.shape[1]]
                touched = ((ii >= 14) & (ii <= 17)) | ((jj >= 14) & (jj <= 17))
                assert (v[~touched] == ONE).all() and (v[touched] < ONE).all(), what
                met["seam"] += int(touched.any() and not touched.all())
            if kind == "last_window":
                assert all((want["min_x"][c], want["min_y"][c]) == (4 * (want["windows_x"][c] - 1), 4 * (want["windows_y"][c] - 1)) and
                           want["sum"][c] == (want["windows"][c] - 1) * ONE + want["min"][c] for c in range(nc) if want["windows"][c]), what
            if kind == "tail":
                assert {k: v for k, v in want.items() if k != "map"} == {k: v for k, v in same_want.items() if k != "map"} and np.array_equal(want["map"], same_want["map"]), what
                met["tail"] += any(not np.array_equal(a, b) for a, b in zip(held, ref))
            if kind == "two_minima" and all(two_fit(p.shape, c and nc == 3) for c, p in enumerate(held)):
                for c in range(nc):
                    v = ssim_ref.window_values(held[c], ref[c], bd)
                    mx, my, off = want["min_x"][c], want["min_y"][c], 48 if c and nc == 3 else 80
                    assert mx >= off and my < 16 and want["min"][c] < ONE and v[(my + 16) // 4, (mx - off) // 4] == want["min"][c] and int((v < ONE).sum()) == 8, (what, c, mx, my)
                assert want["map"][0, 0] == want["map"][0, 1] == min(want["min"]), what
                met["two_minima"] += 1
            met["no_window_word"] += int((want["map"] == ssim_ref.NO_WINDOW).any())
            for name, given in forms(ref):
                met["eight_bit"] += name == "8-bit"
                same(queued(L, ctx, 0, win, given), want, win, bd, what + ", %s reference" % name)
            if kind in ("flat", "two_minima"):
                write(ctx, 0, planes)
        # (without a map nothing but the result is written; and the mean of identical pictures is exactly 1)
        got = queued(L, ctx, 0, win, [np.ascontiguousarray(p, np.uint16) for p in part], with_map=False)
        same(got, same_want, win, bd, "no map, window %r" % (win,))
        rc, mean = c_mean(L, got[0])
        assert rc == abi.VVR_OK and mean == ssim_ref.mean(same_want) and mean[0] == mean[3] == 1.0
    assert met["negative"] and met["clamped"] and met["tail"] and met["no_window_word"] and (bd > 8 or met["eight_bit"]), met
    assert nc == 1 or (met["two_minima"] >= 2 and met["seam"] >= 2), met


def check_words_above_the_bit_depth(L, ctx, write, planes, bd):
    """a slot holding 0xffff words (and other values above L): x is clamped as y is"""
    nc = len(planes)
    top = (1 << bd) - 1
    rng = np.random.default_rng(1410 + bd)
    high = [np.where(rng.random(p.shape) < 0.5, 0xffff, rng.integers(0, 1 << 16, p.shape)).astype(np.uint16) for p in planes]
    write(ctx, 0, high)
    for win in windows(nc):
        held = compare_ref.window_planes(high, win)
        for ref in ([np.full(p.shape, top, np.int64) for p in held], [rng.integers(0, 1 << 16, p.shape, dtype=np.int64) for p in held]):
            want = ssim_ref.ssim(held, ref, bd)
            assert want == {**ssim_ref.ssim([np.minimum(p, top) for p in held], [np.minimum(p, top) for p in ref], bd), "map": want["map"]}
            same(queued(L, ctx, 0, win, SUP.forms(ref)[0][1]), want, win, bd, "words above the bit depth in the slot, window %r" % (win,))
    write(ctx, 0, planes)


def ref_slot_case(L, ctx, slot, ref_slot, win, ps, pr, bd, what):
    same(queued(L, ctx, slot, win, ref_slot), ssim_ref.ssim(ps, pr, bd), win, bd, what)


def stats_case(L, ctx, planes, bd):
    """vvr_get_stats: one k_output_ssim and one k_output_ssim_sum per request; none with statistics off"""
    win = SUP.RING_WIN
    part = compare_ref.window_planes(planes, win)
    ref = SUP.noisy(part, bd, 5)

    def request():
        same(queued(L, ctx, 0, win, SUP.forms(ref)[0][1]), ssim_ref.ssim(part, ref, bd), win, bd, "with statistics on")

    def verify(got):
        assert got == {"k_output_ssim": 3, "k_output_ssim_sum": 3}, got
    return [request] * 3, verify, request


def ring_request(L, ctx, planes, win, part, ref, bd):
    given, want = SUP.forms(ref)[0][1], ssim_ref.ssim(part, ref, bd)
    return lambda: submit(L, ctx, 0, win, given), lambda t, keep, what: same(collect(L, ctx, t, keep), want, win, bd, what)


# ---- tests

def test_the_structs_mirror_the_header(tmp_path):
    """sizeof / offsetof of the structs as gcc sees include/vvr.h == their ctypes mirrors; explicit pads only: the size is the sum of the fields"""
    names = [("vvr_frame_ssim", abi.FrameSsim), ("vvr_ssim_request", abi.SsimRequest)]
    SUP.assert_mirrors(tmp_path, names)
    for mirror in (abi.FrameSsim, abi.SsimRequest):
        assert C.sizeof(mirror) == sum(C.sizeof(f[1]) for f in mirror._fields_) and C.sizeof(mirror) % 8 == 0
    assert C.sizeof(abi.FrameSsim) == 152 and C.sizeof(abi.SsimRequest) == C.sizeof(abi.CompareRequest)
    L = SUP.stub_lib()
    assert L.vvr_abi_sizeof(18) == 0      # (no new index)
    assert abi.VVR_ABI_VERSION == 5


def test_the_restatement_agrees_with_textbook_ssim():
    """tests/ssim_ref.py alone against SSIM in float64 from means and population variances per window.  v is the product of two quotients that
    are each truncated once (below 2^-24 each, and both factors are at most 1 in magnitude) and truncated once more: | v / 2^24 - SSIM | <
    3 * 2^-24, with the stabilising constants the definition has, C1 / N^2 and C2 / N^2.  Those are ( K L )^2 rounded at N^2: against the
    unrounded ( 0.01 L )^2 and ( 0.03 L )^2 the same bound widens by the rounding's effect, at most 0.5 / ( 4 C1 ) + 0.5 / ( 2 C2 ), because
    d/dC of ( C + a ) / ( C + b ) is ( b - a ) / ( C + b )^2 <= 1 / ( 4 C ) for 0 <= a <= b and <= 1 / ( 2 C ) for |a| <= b."""
    bound = 3 * 2.0 ** -24 + 1e-12
    rng = np.random.default_rng(1420)
    worst = 0.
    for bd in (8, 10):
        top, c1, c2 = ssim_ref.constants(bd)
        assert (c1, c2) == ((26634, 239708) if bd == 8 else (428658, 3857925))
        base = rng.integers(0, top + 1, (40, 52), dtype=np.int64)
        smooth = (np.add.outer(np.arange(40), np.arange(52)) * top // 90).astype(np.int64)
        checker = (np.add.outer(np.arange(40), np.arange(52)) & 1) * top
        pairs = [("identical", base, base), ("random", base, rng.integers(0, top + 1, base.shape, dtype=np.int64)), ("inverse", base, top - base),
                 ("noise", smooth, np.clip(smooth + rng.integers(-8, 9, smooth.shape), 0, top)), ("flat", np.full(base.shape, top // 3), np.full(base.shape, top // 2)),
                 ("dark flat", np.zeros(base.shape, np.int64), np.full(base.shape, 3)), ("saturated", np.full(base.shape, top), base),
                 ("checkerboard", checker, top - checker), ("above L", base + top, smooth)]
        for what, a, b in pairs:
            v = ssim_ref.window_values(a, b, bd).astype(np.float64) / ONE
            assert v.shape == (9, 12)
            exact = ssim_ref.textbook(a, b, bd, c1 / 4096.0, c2 / 4096.0)
            err = float(np.abs(v - exact).max())
            worst = max(worst, err)
            print("%-12s at %2d bits: largest deviation %.3g (bound %.3g)" % (what, bd, err, bound))
            assert err < bound, (what, bd, err)
            err_k = float(np.abs(v - ssim_ref.textbook(a, b, bd)).max())
            print("%-12s at %2d bits, unrounded K: largest deviation %.3g (bound %.3g)" % (what, bd, err_k, bound + 0.5 / (4 * c1) + 0.5 / (2 * c2)))
            assert err_k < bound + 0.5 / (4 * c1) + 0.5 / (2 * c2), (what, bd, err_k)
    assert worst > 0


def test_truncation_is_toward_zero():
    a = np.array([7, -7, 0, -1, 1 << 40, -(1 << 40)], np.int64)
    assert ssim_ref.trunc_div(a, np.int64(2)).tolist() == [3, -3, 0, 0, 1 << 39, -(1 << 39)]
    assert ssim_ref.trunc_div(a, np.int64(3)).tolist() == [2, -2, 0, 0, (1 << 40) // 3, -((1 << 40) // 3)]


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1430 + bd + cf)
    check_contents(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_slot_holding_words_above_the_bit_depth_is_clamped(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1440)
    check_words_above_the_bit_depth(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference(bd, cf):
    L = SUP.stub_lib()
    ctx, a = SUP.ctx_with(L, picture_size(cf), bd, cf, 1450)
    SUP.check_ref_slot("ssim", L, ctx, SUP.writer(L), a, SUP.noisy(a, bd, 1451), bd)
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1460)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    SUP.tickets_and_the_ring("ssim", L, ctx, planes, 10, ext)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernels():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1461)
    SUP.statistics("ssim", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_alone():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1462)
    SUP.write_picture(L, ctx, 1, planes)
    win = (8, 4, 200, 64)
    part = [np.ascontiguousarray(p) for p in compare_ref.window_planes(planes, win)]
    keep = abi.FrameSsim()

    refused = SUP.refuser(L, ctx, "ssim", lambda ref=part, w_=win: abi.ssim_request(0, None, w_, ref, keep))

    # a window below 8 x 8
    for w, h in [(6, 8), (8, 6), (2, 2), (6, 80), (208, 6)]:
        refused(b"below 8 x 8", ref=1, w_=(0, 0, w, h))
    # everything a comparison request is refused for
    refused(b"struct_size", struct_size=C.sizeof(abi.SsimRequest) - 8)
    refused(b"no such slot", slot=7)
    refused(b"no such slot", slot=-1)
    refused(b"no such ref_slot", ref=5)
    refused(b"no such ref_slot", ref_slot=-2)
    refused(b"the slot itself", ref=0)
    refused(b"job must be", job=-2)
    refused(b"result is NULL", result=None)
    for x, y, w, h in [(W - 100, 0, 200, 64), (0, H_ - 2, 8, 4), (-2, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, 8, -2), (1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 9, 8), (0, 0, 8, 9)]:
        refused(b"outside the picture, empty, or odd", ref=1, w_=(x, y, w, h))
    refused(b"ref_bytes_per_sample", ref_bytes_per_sample=0)
    refused(b"ref_bytes_per_sample", ref_bytes_per_sample=4)
    for k in range(3):
        refused(b"missing reference plane or stride", **{"plane%d" % k: None})
        refused(b"missing reference plane or stride", **{"stride%d" % k: part[k].shape[1] * 2 - 1})
    # device planes mixed with host planes; a plane partly inside a device range
    bufs = [np.zeros(p.nbytes + 64, np.uint8) for p in part]
    for b_ in bufs:
        assert L.vvr_device_register(ctx, b_.ctypes.data, b_.nbytes) == abi.VVR_OK
    inside = [np.frombuffer(b_, np.uint16, p.size).reshape(p.shape) for b_, p in zip(bufs, part)]
    refused(b"mixed", ref=[inside[0], part[1], inside[2]])
    assert L.vvr_device_unregister(ctx, bufs[0].ctypes.data) == abi.VVR_OK
    assert L.vvr_device_register(ctx, bufs[0].ctypes.data, 1) == abi.VVR_OK
    refused(b"partly inside", ref=inside)
    for b_ in bufs:
        assert L.vvr_device_unregister(ctx, b_.ctypes.data) == abi.VVR_OK
    # pictures of different sizes in the two slots
    assert L.vvr_slot_picture_size(ctx, 1, W - 8, H_) == abi.VVR_OK
    refused(b"different sizes", ref=1)
    assert L.vvr_slot_picture_size(ctx, 1, W, H_) == abi.VVR_OK
    # a 4:0:0 context: odd windows are fine, planes 1 and 2 are not looked at
    ctx400, p400 = SUP.ctx_with(L, picture_size(0), 8, 0, 1463)
    refused(b"outside the picture", c=ctx400, ref=[p400[0]], w_=(0, 0, W400 + 1, 8))
    refused(b"below 8 x 8", c=ctx400, ref=[p400[0]], w_=(0, 0, W400, 7))
    L.vvr_destroy(ctx400)
    assert L.vvr_ssim_submit(None, None) == abi.VVR_ERR_PARAMETER and L.vvr_ssim_submit(ctx, None) == abi.VVR_ERR_PARAMETER
    # the ring is untouched: eight requests still fit
    want = ssim_ref.ssim(part, part, 10)
    SUP.eight_still_fit(L, ctx, lambda n: submit(L, ctx, 0, win, part if n % 2 else 1), lambda t, got: same(collect(L, ctx, t, got), want, win, 10, "behind the refusals"))
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("ssim", SUP.stub_lib())


def delivered(keep):
    assert keep[0].windows[0] == 63 * 31


SUP.register("ssim", b"vvr_ssim_submit", ring_request, stats=stats_case, ref_slot=ref_slot_case, cases=windows,
             failing=lambda L, ctx, slot, win, job, ref_slot: submit(L, ctx, slot, win, XC.zeros_or_slot(win, ref_slot), job=job),
             untouched=lambda keep: bytes(keep[0]) == bytes([SUP.FILL]) * C.sizeof(abi.FrameSsim) and (keep[1] == -0x55555556).all(), delivered=delivered)


HAND = [("luma only is below one", 10, 3, [100, 25, 25], [100 * ONE - 12345, 25 * ONE, 25 * ONE]),
        ("every component", 8, 3, [516961, 128961, 128961], [516961 * 9000000, 128961 * 16000000, -128961 * 5]),
        ("negative", 10, 3, [64, 16, 16], [-64 * ONE, -16 * ONE + 1, -3]),
        ("chroma without windows", 9, 3, [1, 0, 0], [ONE - 1, 0, 0]),
        ("4:0:0", 8, 1, [33, 0, 0], [33 * ONE // 2, 0, 0])]


@pytest.mark.parametrize("what,bd,nc,count,total", HAND)
def test_mean_ssim_on_sums_built_by_hand(what, bd, nc, count, total):
    L = SUP.stub_lib()
    raw = abi.FrameSsim()
    raw.struct_size, raw.bit_depth, raw.num_components = C.sizeof(abi.FrameSsim), bd, nc
    for c in range(3):
        raw.windows[c], raw.sum[c] = count[c], total[c]
    rc, got = c_mean(L, raw)
    assert rc == abi.VVR_OK and got == ssim_ref.mean(dict(num_components=nc, windows=count, sum=total)), (what, got)
    if what == "luma only is below one":
        assert got[1] == got[2] == 1.0 and got[0] < got[3] < 1.0
    if what == "negative":
        assert got[0] == -1.0 and -1.0 < got[1] < 0 and got[3] < 0
    if what == "chroma without windows":
        assert got[1] == got[2] == 0. and got[0] == got[3] == (ONE - 1) / ONE
    if what == "4:0:0":
        assert got[1] == got[2] == 0. and got[0] == got[3] and abs(got[0] - 0.5) < 1e-7


def test_mean_ssim_of_a_request_and_its_refusals():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1470)
    win = WINDOWS[0]
    part = compare_ref.window_planes(planes, win)
    ref = SUP.noisy(part, 10, 1471)
    want = ssim_ref.ssim(part, ref, 10)
    raw, _ = queued(L, ctx, 0, win, SUP.forms(ref)[0][1])
    rc, got = c_mean(L, raw)
    assert rc == abi.VVR_OK and got == ssim_ref.mean(want) and all(0 < v < 1 for v in got)
    L.vvr_destroy(ctx)
    untouched = [-1.] * 4
    assert c_mean(L, None) == (abi.VVR_ERR_PARAMETER, untouched)
    assert L.vvr_compare_ssim(C.byref(raw), None) == abi.VVR_ERR_PARAMETER
    for field, value in (("struct_size", C.sizeof(abi.FrameSsim) - 8), ("bit_depth", 7), ("bit_depth", 12)):
        bad = abi.FrameSsim.from_buffer_copy(bytes(raw))
        setattr(bad, field, value)
        assert c_mean(L, bad) == (abi.VVR_ERR_PARAMETER, untouched)
    bad = abi.FrameSsim.from_buffer_copy(bytes(raw))
    bad.windows[0] = 0
    assert c_mean(L, bad) == (abi.VVR_ERR_PARAMETER, untouched)


def test_python_mirror_and_symbols():
    import vvdec_amd
    assert "vvr_ssim_submit" in vvdec_amd.EXPORTED_SYMBOLS and "vvr_compare_ssim" in vvdec_amd.EXPORTED_SYMBOLS
    assert hasattr(vvdec_amd.Reconstructor, "ssim")
    assert abi.ssim_map_shape((0, 0, 208, 80)) == (2, 4) and abi.ssim_map_shape((2, 2, 70, 34)) == (1, 2) and abi.ssim_map_shape((0, 0, 132, 76)) == (2, 3)
