"""CPU: the four measures of the output queue against a reference of another size than the window (vvr_set_compare_scaling ahead of
vvr_compare_submit, vvr_ssim_submit, vvr_msssim_submit, vvr_xpsnr_submit) on the stand-in runtime of tests/hoststub, where launch_rescale and the
measures' launchers are plain loops (vvr_output.inc, host only).  Expected values: the picture side is what vvr_read_output_scaled delivers for
the window, the size and `collocated` - pinned against vvdec::rescalePlane by tests/test_output_rescale_host.py, and once more here where the
drop-in library is built - fed to the numpy restatements of the measures (compare_ref, ssim_ref, msssim_ref, xpsnr_ref).  Every comparison of
integers is exact.  The helpers take a library and a context, so tests/test_gpu_output_scaled_compare.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import compare_ref
import msssim_ref
import output_support as SUP
import rescale_ref
import ssim_ref
import test_host_glue as T
import test_output_compare_host as XC
import test_output_msssim_host as XM
import test_output_ssim_host as XS
import test_output_xpsnr_host as XX
import xpsnr_ref
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = XC.W, XC.H_              # 208 x 80 in 4:2:0
W400, H400 = XC.W400, XC.H400    # 136 x 8 in 4:0:0
# name, window -> scaled size (luma samples)
CASES = [("2x up", (0, 0, 104, 40), (208, 80)),                 # the plain ladder case: four blocks across, the last 16 wide, two down
         ("non-integer up", (2, 2, 70, 34), (200, 72)),         # a last block 8 wide and 8 high; a width that is no multiple of 64
         ("8x up", (8, 4, 16, 8), (128, 64)),                   # the limit: taps clamped to a tiny window, many output rows per source row
         ("8x down", (0, 0, 208, 80), (26, 10)),                # the limit: a 13 x 5 chroma plane, whose rows are odd - the by-sample class
         ("equal size", (0, 0, 208, 80), (208, 80))]            # the phase-0 luma filter and the chroma phase of `collocated`
CASES_400 = [("4:0:0, odd sizes", (3, 1, 131, 5), (77, 9))]     # odd origin and odd scaled width
LADDER, UNEVEN = CASES[0], CASES[1]


def picture_size(cf):
    return (W, H_) if cf else (W400, H400)


def cases(nc):
    return CASES if nc == 3 else CASES_400


def scaling(L, ctx, size, col=1):
    rc = L.vvr_set_compare_scaling(ctx, size[0], size[1], col)
    assert rc == abi.VVR_OK, (size, col, L.vvr_last_error(ctx))


def off(L, ctx):
    scaling(L, ctx, (0, 0), 0)


def rescaled(L, ctx, slot, win, size, col, nc):
    """the picture side of a scaled request: every component of the window as vvr_read_output_scaled delivers it, 16-bit"""
    out = []
    for c in range(nc):
        s = 1 if c else 0
        a = np.full((size[1] >> s, size[0] >> s), 0xaaaa, np.uint16)
        rc = L.vvr_read_output_scaled(ctx, slot, c, win[0] >> s, win[1] >> s, win[2] >> s, win[3] >> s, size[0] >> s, size[1] >> s, col, 2, a.ctypes.data, a.strides[0])
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        out.append(a)
    return out


def as_window(size):
    return (0, 0, size[0], size[1])


# one request of each kind: the request carries the window, the arrays vvr_output_wait writes are sized by the scaled size
def submit_compare(L, ctx, slot, win, size, ref, with_map=True, job=None, bps=2):
    raw = abi.FrameCompare()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    blocks = np.full(abi.compare_map_shape(as_window(size)), 0xaaaaaaaa, np.uint32) if with_map else None
    req = abi.compare_request(slot, job, win, ref, raw, blocks, True, bps)
    return L.vvr_compare_submit(ctx, C.byref(req)), (raw, blocks)


def submit_ssim(L, ctx, slot, win, size, ref, with_map=True, job=None):
    raw = abi.FrameSsim()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    blocks = np.full(abi.ssim_map_shape(as_window(size)), -0x55555556, np.int32) if with_map else None
    req = abi.ssim_request(slot, job, win, ref, raw, blocks, True, 2)
    return L.vvr_ssim_submit(ctx, C.byref(req)), (raw, blocks)


def submit_msssim(L, ctx, slot, win, size, ref, scales, job=None):
    raw = abi.FrameMsssim()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    req = abi.msssim_request(slot, job, win, ref, raw, scales, True, 2)
    return L.vvr_msssim_submit(ctx, C.byref(req)), raw


def submit_xpsnr(L, ctx, slot, win, size, ref, prev=(), block=0, job=None):
    raw = abi.FrameXpsnr()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    shape = abi.xpsnr_blocks(size[0], size[1], block)
    blocks = np.frombuffer(bytearray([SUP.FILL]) * (XX.BLOCK_DTYPE.itemsize * shape[1] * shape[2]), XX.BLOCK_DTYPE)
    req = abi.xpsnr_request(slot, job, win, ref, raw, list(prev), blocks, block, 0, True, 2)
    return L.vvr_xpsnr_submit(ctx, C.byref(req)), (raw, blocks)


def queued(L, ctx, submitted):
    t, keep = submitted
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return XC.collect(L, ctx, t, keep)


def words16(planes):
    return [np.ascontiguousarray(p, np.uint16) for p in planes]


def check_comparison(L, ctx, planes, bd):
    """every content of the comparison tests, built on the rescaled frame, at every case, in every form the values fit, with and without a map"""
    nc = len(planes)
    rng = np.random.default_rng(2100 + bd + nc)
    blocks_seen = set()
    for name, win, size in cases(nc):
        scaling(L, ctx, size)
        part = rescaled(L, ctx, 0, win, size, 1, nc)
        assert [p.shape for p in part] == [(size[1] >> (1 if c else 0), size[0] >> (1 if c else 0)) for c in range(nc)]
        for kind in XC.kinds(nc):
            for bps in (2, 1):
                if bps == 1 and kind != "random" and any(int(p.max()) > 255 for p in part):
                    continue
                ref = XC.reference(kind, rng, part, bd, bps)
                want = compare_ref.compare(part, ref)
                what = "%s: %s at %d bits, %r -> %r" % (name, kind, bd, win, size)
                if kind == "identical":
                    assert sum(want["differing"]) == 0 and not want["map"].any(), what
                if kind.startswith("last"):
                    c = int(kind[4:])
                    assert sum(want["differing"]) == 1 and (want["first_x"][c], want["first_y"][c]) == (want["width"][c] - 1, want["height"][c] - 1), what
                blocks_seen.add(want["map"].shape)
                for form, given in [f for f in SUP.forms(ref) if (f[0] == "8-bit") == (bps == 1)]:
                    for with_map in (True, False):
                        got = queued(L, ctx, submit_compare(L, ctx, 0, win, size, given, with_map))
                        XC.same(got, want, as_window(size), bd, "%s, %s reference, map %d" % (what, form, with_map))
    off(L, ctx)
    assert nc == 1 or blocks_seen == {(2, 4), (1, 2), (1, 1)}, blocks_seen


def check_collocated(L, ctx, planes, bd):
    """the flag reaches the chroma launches: the four values give four different chroma planes on the 2x case, the same luma, and each request
    agrees with its own"""
    name, win, size = LADDER
    seen = []
    rng = np.random.default_rng(2110)
    for col in range(4):
        scaling(L, ctx, size, col)
        part = rescaled(L, ctx, 0, win, size, col, 3)
        seen.append(part)
        for kind in ("identical", "random"):
            ref = XC.reference(kind, rng, part, bd)
            got = queued(L, ctx, submit_compare(L, ctx, 0, win, size, SUP.forms(ref)[0][1]))
            XC.same(got, compare_ref.compare(part, ref), as_window(size), bd, "collocated %d, %s" % (col, kind))
    assert all(np.array_equal(seen[0][0], s[0]) for s in seen)
    assert all(not np.array_equal(seen[a][1], seen[b][1]) for a in range(4) for b in range(a))
    off(L, ctx)


def references(rng, part, bd):
    """`identical` and `random` for the windowed measures: the rescaled frame itself, and samples of the bit depth drawn at random"""
    return [("identical", [p.astype(np.int64) for p in part]), ("random", [rng.integers(0, 1 << bd, p.shape, dtype=np.int64) for p in part])]


def check_windowed_measures(L, ctx, planes, bd):
    """SSIM, MS-SSIM with 2 scales and XPSNR - temporal 0 and 1, block 0 and 8 - on the 2x and the non-integer case"""
    rng = np.random.default_rng(2120 + bd)
    for name, win, size in (LADDER, UNEVEN):
        scaling(L, ctx, size)
        part = rescaled(L, ctx, 0, win, size, 1, 3)
        swin = as_window(size)
        for kind, ref in references(rng, part, bd):
            what = "%s: %s at %d bits" % (name, kind, bd)
            given = [SUP.padded(p, np.uint16, k) for p, k in zip(ref, (3, 5, 7))]
            XS.same(queued(L, ctx, submit_ssim(L, ctx, 0, win, size, given)), ssim_ref.ssim(part, ref, bd), swin, bd, "SSIM, " + what)
            XS.same(queued(L, ctx, submit_ssim(L, ctx, 0, win, size, given, with_map=False)), ssim_ref.ssim(part, ref, bd), swin, bd, "SSIM without a map, " + what)
            want = msssim_ref.msssim(part, ref, bd, 2)
            assert want["width"][1][1:] == [size[0] >> 2] * 2 and want["height"][1][1:] == [size[1] >> 2] * 2
            XM.same(queued(L, ctx, submit_msssim(L, ctx, 0, win, size, given, 2)), want, swin, bd, "MS-SSIM, " + what)
            prev = [rng.integers(0, 1 << bd, part[0].shape, dtype=np.int64)]
            for temporal in (0, 1):
                for block in (0, 8):
                    want = xpsnr_ref.xpsnr_integers(part, ref, prev[:temporal], block, 0)
                    assert want["block"] == (block or 4) and want["blocks_x"] == -(-size[0] // want["block"]) and want["temporal"] == temporal
                    got = queued(L, ctx, submit_xpsnr(L, ctx, 0, win, size, given, [SUP.padded(p, np.uint16, 9) for p in prev[:temporal]], block))
                    XX.same(got, want, swin, bd, "XPSNR, temporal %d, block %d, %s" % (temporal, block, what))
    off(L, ctx)


def check_capture_at_submit(L, ctx, fresh, planes, bd):
    """a scaled request, then ( 0, 0 ), then an unscaled one, both collected afterwards: each means what was set when it was submitted, and the
    unscaled one is the result of a context (`fresh`, the same picture in its slot 0) on which the setter was never called"""
    name, win, size = LADDER
    rng = np.random.default_rng(2130)
    scaling(L, ctx, size)
    part = rescaled(L, ctx, 0, win, size, 1, 3)
    ref = XC.reference("random", rng, part, bd)
    plain = compare_ref.window_planes(planes, win)
    plain_ref = XC.reference("random", rng, plain, bd)
    a = submit_compare(L, ctx, 0, win, size, SUP.forms(ref)[0][1])
    off(L, ctx)
    b = XC.submit(L, ctx, 0, win, SUP.forms(plain_ref)[0][1])
    scaling(L, ctx, (2 * size[0], 2 * size[1]))      # (a request in flight keeps the value it was submitted with)
    XC.same(queued(L, ctx, a), compare_ref.compare(part, ref), as_window(size), bd, "the scaled request")
    got = queued(L, ctx, b)
    XC.same(got, compare_ref.compare(plain, plain_ref), win, bd, "the unscaled request behind it")
    there = XC.queued(L, fresh, 0, win, SUP.forms(plain_ref)[0][1])
    assert bytes(got[0]) == bytes(there[0]) and np.array_equal(got[1], there[1])
    off(L, ctx)


def check_homes(L, ctx, planes, bd):
    """the reference in memory of vvr_host_alloc and of vvr_device_alloc (rows padded), and in pageable memory that is overwritten right after
    the call"""
    name, win, size = UNEVEN
    rng = np.random.default_rng(2140)
    scaling(L, ctx, size)
    part = rescaled(L, ctx, 0, win, size, 1, 3)
    for bps, dt in ((2, np.uint16), (1, np.uint8)):
        ref = XC.reference("random", rng, part, bd, bps)
        want = compare_ref.compare(part, ref)
        given = [SUP.padded(p, dt, 3) for p in ref]
        sub = submit_compare(L, ctx, 0, win, size, given)
        for g in given:
            g.base[...] = 0x33
        XC.same(queued(L, ctx, sub), want, as_window(size), bd, "pageable, %d bytes per sample" % bps)
        for home in ("vvr_host_alloc", "vvr_device_alloc"):
            given, bases = [], []
            for c, p in enumerate(ref):
                stride = p.shape[1] + (3, 5, 7)[c]
                base = getattr(L, home)(ctx, p.shape[0] * stride * bps)
                assert base
                bases.append(base)
                a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                a[...] = 0x44
                a[:, :p.shape[1]] = p
                given.append(a[:, :p.shape[1]])
            XC.same(queued(L, ctx, submit_compare(L, ctx, 0, win, size, given)), want, as_window(size), bd, "%s, %d bytes per sample" % (home, bps))
            if home == "vvr_device_alloc":
                for b_ in bases:
                    L.vvr_device_free(ctx, b_)
    off(L, ctx)


SETTER_REFUSALS = [((208, 0, 1), b"one side is 0"), ((0, 80, 1), b"one side is 0"), ((8194, 80, 1), b"1 .. 8192"), ((208, 8194, 1), b"1 .. 8192"),
                   ((-2, 80, 1), b"1 .. 8192"), ((208, -80, 1), b"1 .. 8192"), ((207, 80, 1), b"odd side"), ((208, 79, 1), b"odd side"),
                   ((208, 80, 4), b"collocated"), ((208, 80, -1), b"collocated"), ((0, 0, 4), b"collocated")]


def check_setter_refusals(L, ctx, planes, bd):
    """every refusal of the setter, with its text; the value set before stays in force: a scaled request behind each still measures at it"""
    name, win, size = LADDER
    scaling(L, ctx, size, 2)
    part = rescaled(L, ctx, 0, win, size, 2, 3)
    want = compare_ref.compare(part, part)
    for args, text in SETTER_REFUSALS:
        assert L.vvr_set_compare_scaling(ctx, *args) == abi.VVR_ERR_PARAMETER, args
        assert text in L.vvr_last_error(ctx) and b"vvr_set_compare_scaling" in L.vvr_last_error(ctx), (args, L.vvr_last_error(ctx))
        XC.same(queued(L, ctx, submit_compare(L, ctx, 0, win, size, words16(part))), want, as_window(size), bd, "behind the refused %r" % (args,))
    assert L.vvr_set_compare_scaling(None, 208, 80, 1) == abi.VVR_ERR_PARAMETER
    off(L, ctx)


def check_submit_refusals(L, ctx, planes, bd):
    """what a submit call refuses under scaling beyond what it refuses without: a size outside 1/8 .. 8 times the window's, ref_slot - each
    kind of request, each with a text that names the call, no ring entry taken: eight further requests are accepted"""
    SUP.write_picture(L, ctx, 1, planes)
    zeros = lambda size: [np.zeros((size[1] >> s, size[0] >> s), np.uint16) for s in (0, 1, 1)]
    kinds = [(b"vvr_compare_submit", lambda win, size, ref: submit_compare(L, ctx, 0, win, size, ref)[0]),
             (b"vvr_ssim_submit", lambda win, size, ref: submit_ssim(L, ctx, 0, win, size, ref)[0]),
             (b"vvr_msssim_submit", lambda win, size, ref: submit_msssim(L, ctx, 0, win, size, ref, 1)[0]),
             (b"vvr_xpsnr_submit", lambda win, size, ref: submit_xpsnr(L, ctx, 0, win, size, ref)[0])]
    # window 16 x 16: 130 > 8 * 16 either way; window 208 x 80: 24 < ceil( 208 / 8 ) = 26 and 8 < 10
    for win, size in [((0, 0, 16, 16), (130, 64)), ((0, 0, 16, 16), (64, 130)), ((0, 0, 208, 80), (24, 16)), ((0, 0, 208, 80), (32, 8))]:
        scaling(L, ctx, size)
        for who, call in kinds:
            rc = call(win, size, zeros(size))
            assert rc == abi.VVR_ERR_PARAMETER and b"1/8 .. 8 times" in L.vvr_last_error(ctx) and who in L.vvr_last_error(ctx), (win, size, who, rc, L.vvr_last_error(ctx))
    # the ends of the range are accepted: 8 x up and 8 x down
    for win, size in [((0, 0, 16, 16), (128, 128)), ((0, 0, 208, 80), (26, 10))]:
        scaling(L, ctx, size)
        queued(L, ctx, submit_compare(L, ctx, 0, win, size, zeros(size)))
    name, win, size = LADDER
    scaling(L, ctx, size)
    for who, call in kinds:
        rc = call(win, size, 1)
        assert rc == abi.VVR_ERR_PARAMETER and b"ref_slot" in L.vvr_last_error(ctx) and who in L.vvr_last_error(ctx), (who, rc, L.vvr_last_error(ctx))
    # the reference's planes are of the scaled size: a stride that holds the window's row alone is below the row
    small = [np.zeros((win[3] >> s, win[2] >> s), np.uint16) for s in (0, 1, 1)]
    rc = submit_compare(L, ctx, 0, win, size, small)[0]
    assert rc == abi.VVR_ERR_PARAMETER and b"stride below" in L.vvr_last_error(ctx)
    # SSIM's 8 x 8 minimum and MS-SSIM's last level look at the scaled size: a window of 16 x 16 scaled to 4 x 4 has no SSIM window, and
    # a window of 4 x 4 scaled to 32 x 32 has; 64 x 64 takes three scales, scaled to 32 x 32 its chroma ends at 4 x 4
    scaling(L, ctx, (4, 4))
    assert submit_ssim(L, ctx, 0, (0, 0, 16, 16), (4, 4), zeros((4, 4)))[0] == abi.VVR_ERR_PARAMETER and b"8 x 8" in L.vvr_last_error(ctx)
    scaling(L, ctx, (32, 32))
    queued(L, ctx, submit_ssim(L, ctx, 0, (0, 0, 4, 4), (32, 32), zeros((32, 32))))
    assert submit_msssim(L, ctx, 0, (0, 0, 64, 64), (32, 32), zeros((32, 32)), 3)[0] == abi.VVR_ERR_PARAMETER and b"last level" in L.vvr_last_error(ctx)
    # the ring is untouched: eight requests still fit
    scaling(L, ctx, size)
    part = rescaled(L, ctx, 0, win, size, 1, 3)
    flight = [submit_compare(L, ctx, 0, win, size, words16(part)) for _ in range(8)]
    assert all(t >= 2 for t, _ in flight) and len(set(t for t, _ in flight)) == 8, [t for t, _ in flight]
    for sub in flight:
        XC.same(queued(L, ctx, sub), compare_ref.compare(part, part), as_window(size), bd, "behind the refusals")
    off(L, ctx)
    # ... and with scaling off ref_slot is what it was
    win = (0, 0, W, H_)
    XC.same(XC.queued(L, ctx, 0, win, 1), compare_ref.compare(planes, planes), win, bd, "ref_slot with scaling off again")


def check_statistics(L, ctx, planes, bd):
    """vvr_get_stats: a scaled comparison is one k_output_compare_scaled and the fold; a scaled SSIM request runs k_rescale - one launch per
    component - ahead of its own kernels"""
    assert L.vvr_enable_stats(ctx, 1) == abi.VVR_OK
    name, win, size = LADDER
    scaling(L, ctx, size)
    part = rescaled(L, ctx, 0, win, size, 1, 3)
    for k in range(2):
        queued(L, ctx, submit_compare(L, ctx, 0, win, size, words16(part)))
    queued(L, ctx, submit_ssim(L, ctx, 0, win, size, words16(part)))
    off(L, ctx)
    XC.queued(L, ctx, 0, win, words16(compare_ref.window_planes(planes, win)))
    got = SUP.launches(L, ctx)
    assert got == {"k_output_compare_scaled": 2, "k_rescale": 3, "k_output_compare": 1, "k_output_compare_sum": 3, "k_output_ssim": 1, "k_output_ssim_sum": 1}, got
    assert L.vvr_enable_stats(ctx, 0) == abi.VVR_OK


# ---- tests

@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_case(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 2000 + bd + cf)
    check_comparison(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_collocated_reaches_the_chroma_planes():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 2010)
    check_collocated(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_ssim_msssim_and_xpsnr_of_the_rescaled_window(bd):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), bd, 1, 2020 + bd)
    check_windowed_measures(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_a_request_keeps_the_value_it_was_submitted_with():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 2030)
    fresh, _ = SUP.ctx_with(L, picture_size(1), 10, 1, 2030)
    check_capture_at_submit(L, ctx, fresh, planes, 10)
    L.vvr_destroy(ctx)
    L.vvr_destroy(fresh)


def test_the_homes_of_a_reference_of_the_scaled_size():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 8, 1, 2040)
    check_homes(L, ctx, planes, 8)
    L.vvr_destroy(ctx)


def test_the_setter_refuses_and_keeps_the_value_set_before():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 2050)
    check_setter_refusals(L, ctx, planes, 10)
    # a 4:0:0 context takes odd sides
    ctx400, _ = SUP.ctx_with(L, picture_size(0), 8, 0, 2051)
    scaling(L, ctx400, (77, 9))
    L.vvr_destroy(ctx400)
    L.vvr_destroy(ctx)


def test_refusals_at_submit_leave_the_ring_alone():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 2060)
    check_submit_refusals(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_statistics_name_the_rescaling():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 2070)
    check_statistics(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_the_slot_is_free_behind_the_rescaling():
    """stream and event operations as the stand-in runtime records them: the request's `read` event - the first the output stream records - is
    the one a picture that later overwrites the slot waits for, as without scaling"""
    from dataclasses import replace
    from vvdec_amd import synth
    import test_output_queue_host as Q
    L = SUP.stub_lib()
    ctx, plans, descs, win = SUP.small_stream(L)
    Wd, Hd = win[2], win[3]
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    s0 = plans[0].slot
    p0 = descs[0].c()
    j0 = L.vvr_submit(ctx, C.byref(p0))
    assert j0 >= 0 and L.vvr_stream_wait_job(ctx, j0, ext, 1) == abi.VVR_OK
    size = (Wd // 2, Hd // 2)
    scaling(L, ctx, size)
    Q._trace(L)
    L.vvt_events_pending(1)
    t, keep = submit_compare(L, ctx, s0, win, size, [np.zeros((size[1] >> s, size[0] >> s), np.uint16) for s in (0, 1, 1)])
    assert t >= 2 and L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY
    ops = Q._trace(L)
    records = [(s, e) for op, s, e in ops if op == 1]
    out_stream = records[-1][0]
    mine = [e for s, e in records if s == out_stream]
    assert len(mine) == 2 and mine[0] != mine[1]
    again = synth.picture_for_plan(replace(plans[0], slot=s0), Wd, Hd, seed=613, tool_flags=T.TOOLS)
    pa = again.c()
    j = L.vvr_submit(ctx, C.byref(pa))
    assert j >= 0 and L.vvr_stream_wait_job(ctx, j, ext, 1) == abi.VVR_OK
    ops = Q._trace(L)
    assert any(op == 0 and e == mine[0] and s != out_stream for op, s, e in ops), "the picture that overwrites the slot did not wait for the request's event"
    L.vvt_events_pending(0)
    XC.collect(L, ctx, t, keep)
    assert L.vvr_sync(ctx) == abi.VVR_OK
    L.vvr_destroy(ctx)


@pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs the reference at build time)")
def test_the_picture_side_is_rescale_plane(tmp_path):
    """the picture side straight from vvdec::rescalePlane instead of vvr_read_output_scaled: the comparison of every case against it reports
    nothing differing, and against it with one sample changed exactly that sample"""
    L = SUP.stub_lib()
    bd = 10
    ctx, planes = SUP.ctx_with(L, picture_size(1), bd, 1, 2080)
    cases_ = []
    for name, win, size in CASES:
        for c in range(3):
            s = 1 if c else 0
            x, y, w, h = (v >> s for v in win)
            cases_.append((planes[c][y:y + h, x:x + w], size[0] >> s, size[1] >> s, c, 1, bd, 1, 0))
    want = rescale_ref.rescale(cases_, T.build_stub(), False, str(tmp_path))
    for n, (name, win, size) in enumerate(CASES):
        part = [np.ascontiguousarray(p, np.uint16) for p in want[3 * n:3 * n + 3]]
        scaling(L, ctx, size, 1)
        XC.same(queued(L, ctx, submit_compare(L, ctx, 0, win, size, part)), compare_ref.compare(part, part), as_window(size), bd, name + ": rescalePlane's frame")
        ref = [p.astype(np.int64) for p in part]
        ref[2][-1, 0] ^= 4
        XC.same(queued(L, ctx, submit_compare(L, ctx, 0, win, size, words16(ref))), compare_ref.compare(part, ref), as_window(size), bd, name + ": one sample off")
    L.vvr_destroy(ctx)


def geometry(L, win, size, nc):
    out = (C.c_longlong * 15)()
    L.vvt_compare_scaled_geometry(win[2], win[3], size[0], size[1], nc, out)
    v = [int(x) for x in out]
    return dict(tile_h=v[0:3], rows_cap=v[3:6], tiles_x=v[6:9], first=v[9:13], lds=v[13], clear=v[14])


def test_the_geometry_of_the_fused_launch():
    """tile height, tile list, LDS and the words cleared ahead of k_output_compare_scaled: worked out by hand for three sizes, and for every
    case what the kernel relies on - a tile height that is a power of two of at most 64 (luma) or 32 (chroma), so that a tile lies in one row of
    blocks; the source rows of a tile within the 128 rows of sums LDS holds; every output row and column in exactly one tile"""
    L = SUP.stub_lib()
    # 1080p to 4K: a source row for every two output rows, 63 / 2 -> 32 + 8 taps = 40 rows of sums (chroma: 31 / 2 -> 16 + 4); 60 x 34 and
    # 30 x 34 tiles - about a thousand each, so the tiles stay 64 and 32 rows high; ( 6 x 3 + 1 ) words for each of 60 x 34 blocks
    g = geometry(L, (0, 0, 1920, 1080), (3840, 2160), 3)
    assert g == dict(tile_h=[64, 32, 32], rows_cap=[40, 20, 20], tiles_x=[60, 30, 30], first=[0, 2040, 3060, 4080], lds=40 * 64 * 4, clear=19 * 2040), g
    # the 2x case of the tests: few tiles, so 16 rows each; 15 / 2 -> 8 + 8 and 8 + 4 rows of sums
    g = geometry(L, LADDER[1], LADDER[2], 3)
    assert g == dict(tile_h=[16, 16, 16], rows_cap=[16, 12, 12], tiles_x=[4, 2, 2], first=[0, 20, 26, 32], lds=16 * 64 * 4, clear=19 * 8), g
    # 8x down: 15 x 8 + 8 = 128 source rows for 16 output rows is the cap; the picture has 80 (chroma: 40)
    g = geometry(L, CASES[3][1], CASES[3][2], 3)
    assert g == dict(tile_h=[16, 16, 16], rows_cap=[80, 40, 40], tiles_x=[1, 1, 1], first=[0, 1, 2, 3], lds=80 * 64 * 4, clear=19), g
    big = [("1080p to 4K", (0, 0, 1920, 1080), (3840, 2160)), ("8x down, large", (0, 0, 1024, 512), (128, 64)), ("8x down, the largest", (0, 0, 8192, 8192), (1024, 1024)),
           ("8x up, the largest", (0, 0, 1024, 1024), (8192, 8192))]
    for nc, cases_ in ((3, CASES + big), (1, CASES_400)):
        for name, win, size in cases_:
            g = geometry(L, win, size, nc)
            assert g["first"][0] == 0 and g["lds"] == 256 * max(g["rows_cap"]) <= 128 * 256 and g["clear"] == (6 * nc + 1) * (-(-size[0] // 64)) * (-(-size[1] // 64)), (name, g)
            for c in range(3):
                if c >= nc:
                    assert g["tile_h"][c] == 0 and g["first"][c + 1] == g["first"][c], (name, g)
                    continue
                s = 1 if c else 0
                th, ow, oh = g["tile_h"][c], size[0] >> s, size[1] >> s
                assert th in (1, 2, 4, 8, 16, 32, 64) and th <= (32 if c else 64), (name, g)
                assert g["tiles_x"][c] == -(-ow // 64) and g["first"][c + 1] - g["first"][c] == g["tiles_x"][c] * (-(-oh // th)), (name, g)
                # the source rows the taps of a tile's output rows reach, by the positions of sampleRateConvCore: within rows_cap
                taps, frac = (4, 5) if c else (8, 4)
                h = win[3] >> s
                scale = ((h << 14) + (oh >> 1)) // oh
                shift = 14 - frac + s
                add = (1 << (shift - 1)) + ((1 << (2 + s)) >> (3 + s))      # (collocated)
                pos = lambda j: ((j * (scale << s) + add) >> shift) >> frac
                for j0 in range(0, oh, th):
                    j1 = min(j0 + th, oh) - 1
                    lo, hi = max(0, pos(j0) - (taps // 2 - 1)), min(h - 1, pos(j1) + taps // 2)
                    assert hi - lo + 1 <= g["rows_cap"][c], (name, c, j0, lo, hi, g)


def test_python_mirror_and_symbols():
    import vvdec_amd
    assert "vvr_set_compare_scaling" in vvdec_amd.EXPORTED_SYMBOLS and hasattr(SUP.stub_lib(), "vvr_set_compare_scaling")
    assert hasattr(vvdec_amd.Reconstructor, "set_compare_scaling") and hasattr(abi, "bind_compare_scaling")
