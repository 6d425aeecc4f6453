"""CPU: MS-SSIM of a picture against a reference frame as a request of the output queue (vvr_msssim_submit, collected with vvr_output_test /
vvr_output_wait) and the host helper vvr_compare_msssim, on the stand-in runtime of tests/hoststub, where launch_output_msssim is a plain loop
(vvr_output.inc, host only).  Planes are uploaded with vvr_write_plane.  Expected values: tests/msssim_ref.py, the numpy restatement of the
definition in include/vvr.h.  Every comparison of integers is exact.  The helpers take a library and a context, so
tests/test_gpu_output_msssim.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import compare_ref
import msssim_ref
import output_support as SUP
import ssim_ref
import test_host_glue as T
import test_output_compare_host as XC
import test_output_ssim_host as XS
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = 304, 272
CASES = [((0, 0, 304, 272), 5),       # luma 304, 152, 76, 38, 19 by 272, 136, 68, 34, 17; chroma ends at 9 x 8: a dropped odd column, one window in the last level
         ((6, 2, 262, 258), 5),       # luma 262, 131, 65, 32, 16 by 258, 129, 64, 32, 16: partial cells at levels 0 and 1, odd sizes, levels below one block, an offset origin
         ((0, 0, 256, 256), 5),       # the smallest window that takes five scales
         ((2, 2, 70, 34), 2)]         # fewer scales: luma 70 x 34, 35 x 17; chroma 35 x 17, 17 x 8
W400, H400 = 136, 40
CASES_400 = [((0, 0, 136, 40), 3), ((3, 0, 131, 40), 3)]      # the plain case; an odd origin: the sample-by-sample class at level 0, the wide class below
CONTENTS = ["identical", "noise", "inverse", "random", "seam", "dead_tail", "deepest"]
ONE = 1 << 24
FIELDS = ("width", "height", "windows_x", "windows_y", "windows", "sum_cs", "sum_v")


def picture_size(cf):
    return (W, H_) if cf else (W400, H400)


def cases(nc):
    return CASES if nc == 3 else CASES_400


def submit(L, ctx, slot, win, ref, scales, job=None, blocking=True, bps=2):
    """one vvr_msssim_submit -> (ticket or error, the vvr_frame_msssim vvr_output_wait writes, filled with 0xaa)"""
    raw = abi.FrameMsssim()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    req = abi.msssim_request(slot, job, win, ref, raw, scales, blocking, bps)
    return L.vvr_msssim_submit(ctx, C.byref(req)), raw


collect = XC.collect


def queued(L, ctx, slot, win, ref, scales, **kw):
    t, keep = submit(L, ctx, slot, win, ref, scales, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, keep)


def fields(raw):
    return {name: [[int(v) for v in getattr(raw, name)[k]] for k in range(5)] for name in FIELDS}


def same(raw, want, win, bd, what):
    """every field of the vvr_frame_msssim, exactly"""
    assert (raw.struct_size, raw.bit_depth, raw.num_components, raw.scales) == (C.sizeof(abi.FrameMsssim), bd, want["num_components"], want["scales"]), what
    got = fields(raw)
    for name in FIELDS:
        assert got[name] == want[name], "%s: %s is %r, expected %r" % (what, name, got[name], want[name])
    assert want["width"][0][0] == win[2] and want["height"][0][0] == win[3]


def c_value(L, raw, weights=None):
    out = (C.c_double * 4)(-1., -1., -1., -1.)
    wt = None if weights is None else (C.c_double * len(weights))(*weights)
    return L.vvr_compare_msssim(C.byref(raw) if raw is not None else None, wt, out), list(out)


def close(a, b):
    """the helper against the float64 numpy evaluation of the same formula: a handful of correctly rounded operations and a sub-ulp pow"""
    return all(abs(x - y) <= 1e-12 * abs(y) for x, y in zip(a, b))


def reference(kind, rng, part, bd, scales):
    """the reference planes of a window whose slot planes are `part`, as int64 arrays; what each content is there for is asserted in
    check_contents"""
    top = (1 << bd) - 1
    ref = [np.minimum(p.astype(np.int64), top) for p in part]
    nc = len(part)
    if kind == "identical":
        return ref
    if kind == "noise":
        return [np.clip(p + rng.integers(-8, 9, p.shape), 0, top) for p in ref]
    if kind == "inverse":
        return [top - p for p in ref]
    if kind == "random":                   # anything 16 bits hold: values above L are clamped, before they are averaged
        return [rng.integers(0, 1 << 16, p.shape, dtype=np.int64) for p in ref]
    if kind == "seam":                     # differences only in luma columns and rows 120 .. 143 (chroma: 60 .. 71): level-1 columns 60 .. 71, across its block border
        for c in range(nc):
            lo, hi = (60, 72) if c and nc == 3 else (120, 144)
            jj, ii = np.mgrid[0:ref[c].shape[0], 0:ref[c].shape[1]]
            mask = ((ii >= lo) & (ii < hi)) | ((jj >= lo) & (jj < hi))
            ref[c] = np.where(mask, ref[c] ^ 21, ref[c])
        return ref
    if kind == "dead_tail":                # one sample differs in every column and row of level 0 outside its whole 4 x 4 cells: consequence (b)
        for c in range(nc):
            h, w = ref[c].shape
            for i in range(4 * (w // 4), w):
                ref[c][(7 * i) % h, i] ^= 32
            for j in range(4 * (h // 4), h):
                ref[c][j, (5 * j) % w] ^= 32
        return ref
    assert kind == "deepest"               # the 2 x 2 samples of level 0 at the far corner of the last sample the last level's windows cover
    for c in range(nc):
        h, w = ref[c].shape
        k = scales - 1
        cx, cy = ((w >> k) - 8) // 4 * 4 + 7, ((h >> k) - 8) // 4 * 4 + 7
        x, y = ((cx + 1) << k) - 2, ((cy + 1) << k) - 2
        quad = ref[c][y:y + 2, x:x + 2]
        quad[...] = 0 if int(quad.sum()) >= 2 * top else top
    return ref


def check_contents(L, ctx, planes, bd):
    """every content at every window in every form, for the picture `planes` in slot 0"""
    nc = len(planes)
    top = (1 << bd) - 1
    rng = np.random.default_rng(1500 + bd + nc)
    met = dict(seam=0, dead_tail=0, eight_bit=0, odd=0)
    for win, scales in cases(nc):
        part = compare_ref.window_planes(planes, win)
        same_want = msssim_ref.msssim(part, part, bd, scales)
        for kind in CONTENTS:
            ref = reference(kind, rng, part, bd, scales)
            want = msssim_ref.msssim(part, ref, bd, scales)
            what = "%s at %d bits, window %r, %d scales" % (kind, bd, win, scales)
            levels = [(k, c) for k in range(scales) for c in range(nc)]
            if kind == "identical":        # (this pins the window counts)
                assert all(want["windows"][k][c] >= 1 and want["sum_cs"][k][c] == want["sum_v"][k][c] == want["windows"][k][c] << 24 for k, c in levels), what
                assert msssim_ref.value(want) == [1.0 if c < nc else 0. for c in range(3)] + [1.0], what
                met["odd"] += sum(want["width"][k][c] & 1 for k, c in levels)
            if kind == "noise":
                assert all(int(np.abs(a - np.minimum(b.astype(np.int64), top)).max()) <= 8 for a, b in zip(ref, part)), what
                assert all(0 < want["sum_v"][k][c] < want["windows"][k][c] << 24 for k, c in levels) and all(0 < v < 1 for v in msssim_ref.value(want)[:nc]), what
            if kind == "inverse":          # (at level 0 the planes are anticorrelated far beyond C2; further down the averaged noise no longer is)
                assert all(want["sum_cs"][0][c] < 0 for c in range(nc)), what
                assert msssim_ref.value(want) == [0.] * 4, what
            if kind == "random":           # clamp before the average: the other order gives other sums
                assert all(int(p.max()) > top for p in ref), what
                other = msssim_ref.msssim(part, ref, bd, scales, clamp_first=False)
                assert other["sum_v"][0] == want["sum_v"][0] and all(other["sum_v"][k] != want["sum_v"][k] for k in range(1, scales)), what
            if kind == "seam" and win[2] >= 152 and win[3] >= 152:      # level 1, luma: windows 14 .. 17 of a row or column of windows hold samples 60 .. 71; the others hold none of them
                x1, y1 = msssim_ref.pyramid(part[0], bd, 2)[1], msssim_ref.pyramid(ref[0], bd, 2)[1]
                assert (x1 != y1).any() and not (np.delete(np.delete(x1 != y1, np.s_[60:72], 0), np.s_[60:72], 1)).any(), what
                v = msssim_ref.window_terms(x1, y1, bd)[2]
                jj, ii = np.mgrid[0:v.shape[0], 0:v.shape[1]]
                touched = ((ii >= 14) & (ii <= 17)) | ((jj >= 14) & (jj <= 17))
                assert (v[~touched] == ONE).all() and (v[touched] < ONE).all() and touched.any() and not touched.all(), what
                met["seam"] += 1
            if kind == "dead_tail":
                assert want == same_want, what
                met["dead_tail"] += any(not np.array_equal(a, np.minimum(b.astype(np.int64), top)) for a, b in zip(ref, part))
            if kind == "deepest":          # the last level differs in exactly its last covered sample; its sums change
                for c in range(nc):
                    xs, ys = msssim_ref.pyramid(part[c], bd, scales)[-1], msssim_ref.pyramid(ref[c], bd, scales)[-1]
                    at = np.argwhere(xs != ys)
                    assert at.tolist() == [[(xs.shape[0] - 8) // 4 * 4 + 7, (xs.shape[1] - 8) // 4 * 4 + 7]], (what, c, at)
                    assert want["sum_v"][scales - 1][c] != same_want["sum_v"][scales - 1][c] and want["sum_cs"][scales - 1][c] != same_want["sum_cs"][scales - 1][c], what
            for name, given in SUP.forms(ref):
                met["eight_bit"] += name == "8-bit"
                raw = queued(L, ctx, 0, win, given, scales)
                same(raw, want, win, bd, what + ", %s reference" % name)
                rc, got = c_value(L, raw)
                assert rc == abi.VVR_OK and close(got, msssim_ref.value(want)), (what, got, msssim_ref.value(want))
                if kind == "inverse":
                    assert got == [0.] * 4, what
        # consequence (a): one scale is an SSIM request of the same window, through the library
        given = SUP.forms(reference("noise", rng, part, bd, 1))[0][1]
        one = queued(L, ctx, 0, win, given, 1)
        ssim = XS.queued(L, ctx, 0, win, given, with_map=False)[0]
        assert [int(v) for v in one.sum_v[0]] == [int(v) for v in ssim.sum] and [int(v) for v in one.windows[0]] == [int(v) for v in ssim.windows], win
        assert one.scales == 1 and fields(one)["windows"][1:] == [[0] * 3] * 4 and fields(one)["sum_v"][1:] == [[0] * 3] * 4
    assert met["dead_tail"] and (bd > 8 or met["eight_bit"]) and met["odd"], met
    assert nc == 1 or met["seam"] >= 3, met


def check_words_above_the_bit_depth(L, ctx, write, planes, bd):
    """a slot holding 0xffff words (and other values above L): x is clamped as y is, before the first average"""
    nc = len(planes)
    top = (1 << bd) - 1
    rng = np.random.default_rng(1510 + bd)
    high = [np.where(rng.random(p.shape) < 0.5, 0xffff, rng.integers(0, 1 << 16, p.shape)).astype(np.uint16) for p in planes]
    write(ctx, 0, high)
    for win, scales in cases(nc):
        held = compare_ref.window_planes(high, win)
        for ref in ([np.full(p.shape, top, np.int64) for p in held], [rng.integers(0, 1 << 16, p.shape, dtype=np.int64) for p in held]):
            want = msssim_ref.msssim(held, ref, bd, scales)
            assert want == msssim_ref.msssim([np.minimum(p, top) for p in held], [np.minimum(p, top) for p in ref], bd, scales)
            assert want != msssim_ref.msssim(held, ref, bd, scales, clamp_first=False)
            same(queued(L, ctx, 0, win, SUP.forms(ref)[0][1], scales), want, win, bd, "words above the bit depth in the slot, window %r" % (win,))
    write(ctx, 0, planes)


def ref_slot_case(L, ctx, slot, ref_slot, case, ps, pr, bd, what):
    win, scales = case
    same(queued(L, ctx, slot, win, ref_slot, scales), msssim_ref.msssim(ps, pr, bd, scales), win, bd, what)


RING_WIN, RING_SCALES = SUP.RING_WIN, 2


def stats_case(L, ctx, planes, bd):
    """vvr_get_stats: `scales` k_output_msssim and one k_output_msssim_sum per request; none with statistics off"""
    asked = CASES[:2] + CASES[3:]
    assert sum(scales for _, scales in asked) == 12

    def request(win, scales):
        def run():
            part = compare_ref.window_planes(planes, win)
            ref = SUP.noisy(part, bd, 5)
            same(queued(L, ctx, 0, win, SUP.forms(ref)[0][1], scales), msssim_ref.msssim(part, ref, bd, scales), win, bd, "with statistics on")
        return run

    def verify(got):
        assert got == {"k_output_msssim": 12, "k_output_msssim_sum": 3}, got
    return [request(*case) for case in asked], verify, request(*asked[-1])


def ring_request(L, ctx, planes, win, part, ref, bd):
    given, want = SUP.forms(ref)[0][1], msssim_ref.msssim(part, ref, bd, RING_SCALES)
    return lambda: submit(L, ctx, 0, win, given, RING_SCALES), lambda t, keep, what: same(collect(L, ctx, t, keep), want, win, bd, what)


# ---- tests

def test_the_structs_mirror_the_header(tmp_path):
    """sizeof / offsetof of the structs as gcc sees include/vvr.h == their ctypes mirrors; explicit pads only: the size is the sum of the fields"""
    names = [("vvr_frame_msssim", abi.FrameMsssim), ("vvr_msssim_request", abi.MsssimRequest)]
    SUP.assert_mirrors(tmp_path, names, [("VVR_MSSSIM_MAX_SCALES", abi.MSSSIM_MAX_SCALES)])
    for mirror in (abi.FrameMsssim, abi.MsssimRequest):
        assert C.sizeof(mirror) == sum(C.sizeof(f[1]) for f in mirror._fields_) and C.sizeof(mirror) % 8 == 0
    assert C.sizeof(abi.FrameMsssim) == 616 and C.sizeof(abi.MsssimRequest) == 96 == C.sizeof(abi.SsimRequest) - 8
    assert abi.MsssimRequest.scales.offset == abi.SsimRequest.pad.offset


def test_python_mirror_and_symbols():
    import vvdec_amd
    assert "vvr_msssim_submit" in vvdec_amd.EXPORTED_SYMBOLS and "vvr_compare_msssim" in vvdec_amd.EXPORTED_SYMBOLS
    assert hasattr(vvdec_amd.Reconstructor, "msssim")
    L = SUP.stub_lib()
    assert L.vvr_abi_sizeof(18) == 0      # (no new index)
    assert abi.VVR_ABI_VERSION == 5
    assert abi.MSSSIM_WEIGHTS == msssim_ref.WEIGHTS


def test_the_restatement_agrees_with_textbook_terms_per_level():
    """tests/msssim_ref.py alone.  Per level, on the same integer pyramid and with the definition's constants C1 / 4096 and C2 / 4096:
    sum_cs / ( windows 2^24 ) is within 2^-24 of the float64 mean of the contrast-structure term (c is one truncated quotient) and sum_v /
    ( windows 2^24 ) within 3 * 2^-24 of the float64 mean SSIM (two truncated quotients, both at most 1 in magnitude, and a truncated product),
    + 1e-12 for the float side.  Printed, not asserted: the distance of the whole MS-SSIM to float64 MS-SSIM on an unrounded pyramid with
    unrounded ( K L )^2 - the cost of the integer pyramid (DESIGN.md section 8 records it)."""
    rng = np.random.default_rng(1520)
    scales = 4
    worst = [0., 0.]
    for bd in (8, 10):
        top, c1, c2 = ssim_ref.constants(bd)
        shape = (136, 152)
        base = rng.integers(0, top + 1, shape, dtype=np.int64)
        smooth = (np.add.outer(np.arange(shape[0]), np.arange(shape[1])) * top // (shape[0] + shape[1])).astype(np.int64)
        texture = np.clip(smooth + (np.add.outer(np.arange(shape[0]) % 7, np.arange(shape[1]) % 5) - 5) * (top // 40), 0, top)
        pairs = [("identical", base, base), ("random", base, rng.integers(0, top + 1, shape, dtype=np.int64)), ("inverse", base, top - base),
                 ("noise", smooth, np.clip(smooth + rng.integers(-8, 9, shape), 0, top)), ("texture blurred", texture, smooth),
                 ("above L", base + top, texture)]
        for what, a, b in pairs:
            want = msssim_ref.msssim([a], [b], bd, scales)
            xs, ys = msssim_ref.pyramid(a, bd, scales), msssim_ref.pyramid(b, bd, scales)
            for k in range(scales):
                cs, full = msssim_ref.textbook_terms(xs[k], ys[k], bd, c1 / 4096.0, c2 / 4096.0)
                n = want["windows"][k][0]
                assert n == cs.size >= 1
                err_cs, err_v = abs(want["sum_cs"][k][0] / (n * float(ONE)) - float(cs.mean())), abs(want["sum_v"][k][0] / (n * float(ONE)) - float(full.mean()))
                worst = [max(worst[0], err_cs), max(worst[1], err_v)]
                assert err_cs < 2.0 ** -24 + 1e-12 and err_v < 3 * 2.0 ** -24 + 1e-12, (what, bd, k, err_cs, err_v)
            far = abs(msssim_ref.value(want)[0] - msssim_ref.float_msssim(a, b, bd, scales))
            print("%-16s at %2d bits: MS-SSIM %.6f, %.3g from float64 MS-SSIM on an unrounded pyramid" % (what, bd, msssim_ref.value(want)[0], far))
    assert worst[0] > 0 and worst[1] > 0


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1530 + bd + cf)
    check_contents(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_slot_holding_words_above_the_bit_depth_is_clamped(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1540)
    check_words_above_the_bit_depth(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference(bd, cf):
    L = SUP.stub_lib()
    ctx, a = SUP.ctx_with(L, picture_size(cf), bd, cf, 1550)
    SUP.check_ref_slot("msssim", L, ctx, SUP.writer(L), a, SUP.noisy(a, bd, 1551), bd)
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1560)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    SUP.tickets_and_the_ring("msssim", L, ctx, planes, 10, ext)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernels():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1561)
    SUP.statistics("msssim", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_alone():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1562)
    SUP.write_picture(L, ctx, 1, planes)
    win, scales = RING_WIN, RING_SCALES
    part = [np.ascontiguousarray(p) for p in compare_ref.window_planes(planes, win)]
    keep = abi.FrameMsssim()

    refused = SUP.refuser(L, ctx, "msssim", lambda ref=part, w_=win, n=scales: abi.msssim_request(0, None, w_, ref, keep, n))

    # scales outside 1 .. 5
    for n in (0, 6, 255):
        refused(b"scales must be", ref=1, n=n)
    # a component without a window at the last level
    for w_, n in [((0, 0, 254, 256), 5), ((0, 0, 256, 254), 5), ((2, 2, 70, 34), 3), ((0, 0, 256, 256 - 2), 5), ((0, 0, 14, 16), 1), ((0, 0, 16, 14), 1), ((6, 2, 8, 8), 1), ((0, 0, 30, 32), 2)]:
        refused(b"no 8 x 8 window at the last level", ref=1, w_=w_, n=n)
    # everything a comparison request is refused for
    refused(b"struct_size", struct_size=C.sizeof(abi.MsssimRequest) + 8)
    refused(b"struct_size", struct_size=C.sizeof(abi.MsssimRequest) - 8)
    refused(b"no such slot", slot=7)
    refused(b"no such slot", slot=-1)
    refused(b"no such ref_slot", ref=5)
    refused(b"no such ref_slot", ref_slot=-2)
    refused(b"the slot itself", ref=0)
    refused(b"job must be", job=-2)
    refused(b"result is NULL", result=None)
    for x, y, w, h in [(W - 100, 0, 200, 64), (0, H_ - 2, 16, 16), (-2, 0, 16, 16), (0, 0, 0, 16), (0, 0, 16, 0), (0, 0, 16, -2), (1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 17, 16), (0, 0, 16, 17)]:
        refused(b"outside the picture, empty, or odd", ref=1, w_=(x, y, w, h), n=1)
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
    # a 4:0:0 context: odd windows are fine, planes 1 and 2 are not looked at; 128 x 32 takes three scales, not four
    ctx400, p400 = SUP.ctx_with(L, picture_size(0), 8, 0, 1563)
    refused(b"outside the picture", c=ctx400, ref=[p400[0]], w_=(0, 0, W400 + 1, 8), n=1)
    refused(b"no 8 x 8 window at the last level", c=ctx400, ref=[p400[0]], w_=(0, 0, W400, 40), n=4)
    refused(b"no 8 x 8 window at the last level", c=ctx400, ref=[p400[0]], w_=(0, 0, W400, 7), n=1)
    L.vvr_destroy(ctx400)
    assert L.vvr_msssim_submit(None, None) == abi.VVR_ERR_PARAMETER and L.vvr_msssim_submit(ctx, None) == abi.VVR_ERR_PARAMETER
    # the ring is untouched: eight requests still fit
    want = msssim_ref.msssim(part, part, 10, scales)
    SUP.eight_still_fit(L, ctx, lambda n: submit(L, ctx, 0, win, part if n % 2 else 1, scales), lambda t, got: same(collect(L, ctx, t, got), want, win, 10, "behind the refusals"))
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("msssim", SUP.stub_lib())


def delivered(raw):
    assert fields(raw)["windows"][:4] == [[63 * 31, 31 * 15, 31 * 15], [31 * 15, 15 * 7, 15 * 7], [15 * 7, 7 * 3, 7 * 3], [7 * 3, 3, 3]]


SUP.register("msssim", b"vvr_msssim_submit", ring_request, stats=stats_case, ref_slot=ref_slot_case, cases=cases,
             failing=lambda L, ctx, slot, win, job, ref_slot: submit(L, ctx, slot, win, XC.zeros_or_slot(win, ref_slot), 4, job=job),
             untouched=lambda raw: bytes(raw) == bytes([SUP.FILL]) * C.sizeof(abi.FrameMsssim), delivered=delivered)


def _hand(bd, nc, scales, windows, sum_cs, sum_v):
    raw = abi.FrameMsssim()
    raw.struct_size, raw.bit_depth, raw.num_components, raw.scales = C.sizeof(abi.FrameMsssim), bd, nc, scales
    for k in range(scales):
        for c in range(3):
            raw.windows[k][c], raw.sum_cs[k][c], raw.sum_v[k][c] = windows[k][c], sum_cs[k][c], sum_v[k][c]
    pad = [[0] * 3] * (5 - scales)
    return raw, dict(num_components=nc, scales=scales, windows=windows + pad, sum_cs=sum_cs + pad, sum_v=sum_v + pad)


def test_msssim_on_sums_built_by_hand():
    L = SUP.stub_lib()
    # every component, three scales: sum_v of the first levels and sum_cs of the last are not looked at
    windows = [[100, 25, 25], [25, 6, 6], [6, 1, 1]]
    cs = [[90 * ONE, 25 * ONE - 7, 20 * ONE], [20 * ONE, 5 * ONE, 3 * ONE], [-(1 << 40), -(1 << 40), -(1 << 40)]]
    v = [[1 << 50, -(1 << 50), 12345], [-(1 << 50), 1 << 50, 54321], [5 * ONE, ONE // 2, ONE - 1]]
    raw, want = _hand(10, 3, 3, windows, cs, v)
    rc, got = c_value(L, raw)
    assert rc == abi.VVR_OK and close(got, msssim_ref.value(want)) and all(0 < g < 1 for g in got), got
    wt = msssim_ref.weights_for(3)
    assert abs(got[0] - 0.9 ** wt[0] * 0.8 ** wt[1] * (5 / 6) ** wt[2]) < 1e-12 and abs(sum(wt) - 1) < 1e-15
    # a caller's weights, as given (not normalised); a weight of 0 takes the level out, a negative mean included
    mine = [0.5, 2.0, 1.0]
    rc, got = c_value(L, raw, mine)
    assert rc == abi.VVR_OK and close(got, msssim_ref.value(want, mine)) and abs(got[0] - 0.9 ** 0.5 * 0.8 ** 2 * (5 / 6)) < 1e-12
    raw.sum_cs[1][0] = -3
    want["sum_cs"] = [want["sum_cs"][0], [-3, 5 * ONE, 3 * ONE]] + want["sum_cs"][2:]
    rc, got = c_value(L, raw)               # a negative level gives 0: max( m, 0 ) under a positive weight
    assert rc == abi.VVR_OK and got[0] == 0. and got[1] > 0 and got[3] > 0 and close(got, msssim_ref.value(want))
    rc, got = c_value(L, raw, [1.0, 0.0, 1.0])      # ... and pow( 0, 0 ) = 1 under weight 0
    assert rc == abi.VVR_OK and abs(got[0] - 0.9 * (5 / 6)) < 1e-12 and close(got, msssim_ref.value(want, [1.0, 0.0, 1.0]))
    # 4:0:0: the other components are 0, all components together is the luma
    raw, want = _hand(8, 1, 2, [[33, 0, 0], [8, 0, 0]], [[33 * ONE // 2, 0, 0], [0, 0, 0]], [[0, 0, 0], [8 * ONE // 4, 0, 0]])
    rc, got = c_value(L, raw)
    assert rc == abi.VVR_OK and got[1] == got[2] == 0. and got[0] == got[3] and close(got, msssim_ref.value(want))
    wt = msssim_ref.weights_for(2)
    assert abs(got[0] - 0.5 ** wt[0] * 0.25 ** wt[1]) < 1e-7
    # one scale: the mean SSIM
    raw, want = _hand(9, 3, 1, [[10, 2, 2]], [[0, 0, 0]], [[9 * ONE, ONE, 2 * ONE]])
    rc, got = c_value(L, raw)
    assert rc == abi.VVR_OK and got == [0.9, 0.5, 1.0, 12 / 14]


def test_msssim_of_a_request_and_its_refusals():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1570)
    win, scales = CASES[1]
    part = compare_ref.window_planes(planes, win)
    ref = SUP.noisy(part, 10, 1571)
    want = msssim_ref.msssim(part, ref, 10, scales)
    raw = queued(L, ctx, 0, win, SUP.forms(ref)[0][1], scales)
    rc, got = c_value(L, raw)
    assert rc == abi.VVR_OK and close(got, msssim_ref.value(want)) and all(0 < v < 1 for v in got)
    mine = [0.1, 0.2, 0.3, 0.25, 0.15]
    rc, got = c_value(L, raw, mine)
    assert rc == abi.VVR_OK and close(got, msssim_ref.value(want, mine))
    L.vvr_destroy(ctx)
    untouched = [-1.] * 4
    assert c_value(L, None) == (abi.VVR_ERR_PARAMETER, untouched)
    assert L.vvr_compare_msssim(C.byref(raw), None, None) == abi.VVR_ERR_PARAMETER
    for field, value in (("struct_size", C.sizeof(abi.FrameMsssim) - 8), ("bit_depth", 7), ("bit_depth", 12), ("scales", 0), ("scales", 6)):
        bad = abi.FrameMsssim.from_buffer_copy(bytes(raw))
        setattr(bad, field, value)
        assert c_value(L, bad) == (abi.VVR_ERR_PARAMETER, untouched)
    for k in range(scales):
        bad = abi.FrameMsssim.from_buffer_copy(bytes(raw))
        bad.windows[k][0] = 0
        assert c_value(L, bad) == (abi.VVR_ERR_PARAMETER, untouched)
    for k, w in ((0, -0.1), (4, float("nan")), (2, float("inf")), (1, -float("inf"))):
        wt = list(mine)
        wt[k] = w
        assert c_value(L, raw, wt) == (abi.VVR_ERR_PARAMETER, untouched)
