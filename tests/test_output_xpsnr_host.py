"""CPU: XPSNR of a picture against a reference frame as a request of the output queue (vvr_xpsnr_submit, collected with vvr_output_test /
vvr_output_wait) and the host helpers vvr_xpsnr_blocks and vvr_compare_xpsnr, on the stand-in runtime of tests/hoststub, where
launch_output_xpsnr is a plain loop (vvr_output.inc, host only).  Planes are uploaded with vvr_write_plane.  Expected values: tests/xpsnr_ref.py,
the numpy restatement of the definition in include/vvr.h.  Every comparison of integers is exact.  The helpers take a library and a context,
so tests/test_gpu_output_xpsnr.py runs the same cases on the device."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import compare_ref
import output_support as SUP
import xpsnr_ref
import test_host_glue as T
import test_output_compare_host as XC
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = 208, 80           # four tiles of 64 x 64 across with a 16-wide last one, two down with a 16-high last one
WINDOWS = [(0, 0, 208, 80),       # the whole picture
           (8, 4, 200, 64),       # an offset window
           (2, 2, 70, 34),        # odd chroma sizes (35 x 17), a last cell 2 wide and 2 high
           (0, 0, 16, 16),
           (6, 2, 8, 8)]          # the smallest: filter 2 has four positions
W400, H400 = 136, 8
WINDOWS_400 = [(0, 0, 136, 8),
               (3, 0, 131, 8)]    # an odd origin, and a last block 3 wide at B = 4: positions only in its first columns
BLOCKS = [0, 4, 44, 64, 128, 256]      # by the formula (4 at these sizes); the smallest; off the tile grid; a tile; larger than a tile; larger than the window
PARAMS = list(itertools.product(BLOCKS, (1, 2), (0, 1, 2)))      # block, filter (both forced at this size), temporal
CONTENTS = ["identical", "noise", "random16", "flat", "prev_equal"]
BLOCK_DTYPE = np.dtype(abi.XPSNR_BLOCK_FIELDS)


def picture_size(cf):
    return (W, H_) if cf else (W400, H400)


def windows(nc):
    return WINDOWS if nc == 3 else WINDOWS_400


def submit(L, ctx, slot, win, ref, prev=(), block=0, filter_=0, with_blocks=True, job=None, blocking=True, bps=2):
    """one vvr_xpsnr_submit -> (ticket or error, (the vvr_frame_xpsnr, the records) vvr_output_wait writes, both filled with 0xaa)"""
    raw = abi.FrameXpsnr()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    shape = abi.xpsnr_blocks(win[2], win[3], block)
    blocks = np.frombuffer(bytearray([SUP.FILL]) * (BLOCK_DTYPE.itemsize * shape[1] * shape[2]), BLOCK_DTYPE) if with_blocks and shape else None
    req = abi.xpsnr_request(slot, job, win, ref, raw, list(prev), blocks, block, filter_, blocking, bps)
    return L.vvr_xpsnr_submit(ctx, C.byref(req)), (raw, blocks)


collect = XC.collect


def queued(L, ctx, slot, win, ref, prev=(), **kw):
    t, keep = submit(L, ctx, slot, win, ref, prev, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, keep)


def same(got, want, win, bd, what):
    """every field of the vvr_frame_xpsnr and every field of every record, exactly"""
    raw, blocks = got
    nc = want["num_components"]
    assert (raw.struct_size, raw.bit_depth, raw.num_components) == (C.sizeof(abi.FrameXpsnr), bd, nc), what
    for name in ("temporal", "filter", "block", "blocks_x", "blocks_y", "act_spatial", "act_temporal", "count"):
        assert int(getattr(raw, name)) == want[name], "%s: %s is %r, expected %r" % (what, name, int(getattr(raw, name)), want[name])
    for name in ("width", "height", "samples", "sse"):
        assert [int(v) for v in getattr(raw, name)] == want[name], "%s: %s is %r, expected %r" % (what, name, [int(v) for v in getattr(raw, name)], want[name])
    assert want["width"][0] == win[2] and want["height"][0] == win[3]
    if blocks is not None:
        assert blocks.shape == want["blocks"].shape, what
        for name in BLOCK_DTYPE.names:
            assert np.array_equal(blocks[name], want["blocks"][name]), "%s: %s of the blocks is\n%r, expected\n%r" % (what, name, blocks[name], want["blocks"][name])


def c_xpsnr(L, raw, blocks, a_pic=0., peak=0.):
    out = (C.c_double * 4)(-1., -1., -1., -1.)
    rc = L.vvr_compare_xpsnr(C.byref(raw) if raw is not None else None, blocks.ctypes.data if blocks is not None else None, a_pic, peak, out)
    return rc, list(out)


def close_enough(got, want, what):
    """decibels whose wsse agree to a relative 1e-9: at most 16384 non-negative terms, each a handful of double operations (2^-53 each), give
    a relative error far below that; in decibels, 10 log10( 1 + 1e-9 ) < 4.4e-9"""
    for g, w_ in zip(got, want):
        assert (g == w_) if math.isinf(w_) or w_ == 0 else abs(g - w_) <= 4.4e-9, (what, got, want)


def reference(kind, rng, part, bd, bits=16):
    """the reference planes and the two prev luma planes of a window whose slot planes are `part`, as int64 arrays; `bits`: what the reference's
    samples have to fit"""
    top = (1 << bd) - 1
    ref = [np.minimum(p.astype(np.int64), top) for p in part]
    shape = part[0].shape
    prev = [rng.integers(0, top + 1, shape, dtype=np.int64) for _ in range(2)]
    if kind == "noise":
        ref = [np.clip(p + rng.integers(-8, 9, p.shape), 0, top) for p in ref]
    if kind == "random16":                 # anything the reference's words hold: the sums need 64 bits
        ref = [rng.integers(0, 1 << bits, p.shape, dtype=np.int64) for p in ref]
        prev = [rng.integers(0, 1 << bits, shape, dtype=np.int64) for _ in range(2)]
    if kind == "flat":                     # no activity at all: every block's act sits at its floor
        ref = [np.full(p.shape, top // 2 - c, np.int64) for c, p in enumerate(ref)]
        prev = [ref[0].copy(), ref[0].copy()]
    if kind == "prev_equal":
        ref = [np.clip(p + rng.integers(-3, 4, p.shape), 0, top) for p in ref]
        prev = [ref[0].copy(), ref[0].copy()]
    return ref, prev


def unaligned(plane):
    """the plane as 16-bit words that start at an odd address, rows an odd number of bytes apart"""
    h, w = plane.shape
    stride = 2 * w + 3
    a = np.ndarray((h, w), "<u2", bytearray([0x5b]) * (h * stride + 2), 1, (stride, 2))
    a[...] = plane
    assert a.ctypes.data % 2 == 1
    return a


def forms(ref, prev):
    """the forms a reference and its prev planes are given in: 2-byte samples at padded strides; 2-byte samples at odd addresses and odd strides;
    1-byte samples, when all values fit, from an odd base at an odd byte stride"""
    out = [("16-bit", [SUP.padded(p, np.uint16, k) for p, k in zip(ref, (3, 5, 7))], [SUP.padded(p, np.uint16, k) for p, k in zip(prev, (9, 1))]),
           ("16-bit at odd addresses", [unaligned(p) for p in ref], [unaligned(p) for p in prev])]
    if all(int(p.max()) <= 255 for p in list(ref) + list(prev)):
        def odd(p):
            a = np.full((p.shape[0], p.shape[1] + (3 if p.shape[1] % 2 == 0 else 2)), 0x5b, np.uint8)
            a[:, 1:1 + p.shape[1]] = p
            return a[:, 1:1 + p.shape[1]]
        out.append(("8-bit", [odd(p) for p in ref], [odd(p) for p in prev]))
        assert all(p.strides[0] % 2 == 1 and p.ctypes.data % 2 == 1 for p in out[-1][1] + out[-1][2])
    return out


def check_contents(L, ctx, write, planes, bd):
    """every content at every window: noise at every block size, filter and temporal, the others at a rotating selection of them, in every form
    the values fit, for the picture `planes` (which this leaves in slot 0)"""
    nc = len(planes)
    rng = np.random.default_rng(1500 + bd + nc)
    met = dict(floor=0, eight_bit=0, wide=0, huge=0, empty_block=0, off_grid=0, by_formula=0)
    turn = 0
    for win in windows(nc):
        part = compare_ref.window_planes(planes, win)
        for kind in CONTENTS:
            ref, prev = reference(kind, rng, part, bd, 8 if bd == 8 and kind == "random16" and win[2] <= 16 else 16)
            chosen = PARAMS if kind == "noise" else [PARAMS[(turn + 7 * k) % len(PARAMS)] for k in range(4)]
            turn += 1
            for block, flt, temporal in chosen:
                want = xpsnr_ref.xpsnr_integers(part, ref, prev[:temporal], block, flt)
                what = "%s at %d bits, window %r, block %d, filter %d, temporal %d" % (kind, bd, win, block, flt, temporal)
                assert want["block"] == (block or 4) and want["count"] >= 4, what
                if kind == "identical":
                    assert want["sse"] == [0, 0, 0] and all(math.isinf(v) for v in xpsnr_ref.xpsnr(want, bd)[:nc]), what
                    met["huge"] += 1
                if kind == "random16":
                    met["wide"] += want["act_spatial"] > 1 << 32 or max(want["sse"]) > 1 << 32
                if kind == "flat":
                    assert want["act_spatial"] == 0 and want["act_temporal"] == 0 and want["count"] > 0, what
                    met["floor"] += 1
                if kind == "prev_equal":
                    assert want["act_temporal"] == 0 and (want["act_spatial"] > 0), what
                met["empty_block"] += int((want["blocks"]["count"] == 0).any())
                met["off_grid"] += block == 44 and want["blocks_x"] > 1
                met["by_formula"] += block == 0
                given = forms(ref, prev[:temporal])
                for name, r, p in given if kind != "noise" or block == 44 else given[:1]:
                    met["eight_bit"] += name == "8-bit"
                    got = queued(L, ctx, 0, win, r, p, block=block, filter_=flt)
                    same(got, want, win, bd, what + ", %s reference" % name)
                    rc, db = c_xpsnr(L, *got)
                    assert rc == abi.VVR_OK, what
                    close_enough(db, xpsnr_ref.xpsnr(want, bd), what)
        # (without records nothing but the result is written)
        got = queued(L, ctx, 0, win, [np.ascontiguousarray(p, np.uint16) for p in part], with_blocks=False)
        same(got, xpsnr_ref.xpsnr_integers(part, part), win, bd, "no records, window %r" % (win,))
    assert met["floor"] and met["huge"] and met["by_formula"] and (bd > 8 or met["eight_bit"]) and met["empty_block"], met
    assert nc == 1 or (met["wide"] and met["off_grid"]), met


def check_consequences(L, ctx, write, planes, bd):
    """sse equals a vvr_compare_submit of the same request; the totals do not depend on the block size; the activity does not depend on the slot"""
    nc = len(planes)
    rng = np.random.default_rng(1510 + bd)
    other = SUP.noisy(planes, bd, 1511)
    for win in windows(nc):
        part = compare_ref.window_planes(planes, win)
        ref, prev = reference("random16", rng, part, bd)
        r16, p16 = forms(ref, prev)[0][1:]
        cmp_raw, _ = XC.queued(L, ctx, 0, win, r16, with_map=False)
        totals = []
        for block in BLOCKS:
            raw, _ = queued(L, ctx, 0, win, r16, p16, block=block, filter_=2)
            assert [int(v) for v in raw.sse] == [int(v) for v in cmp_raw.sse], (win, block)
            totals.append(([int(v) for v in raw.sse], int(raw.act_spatial), int(raw.act_temporal), int(raw.count)))
        assert all(t == totals[0] for t in totals), (win, totals)
        write(ctx, 0, other)
        raw, _ = queued(L, ctx, 0, win, r16, p16, block=64, filter_=2)
        assert (int(raw.act_spatial), int(raw.act_temporal), int(raw.count)) == totals[0][1:], win
        assert [int(v) for v in raw.sse] != totals[0][0], win
        write(ctx, 0, planes)


def check_anchor(L, ctx, write):
    """the CPU anchor of the definition, on a context of 208 x 80 at 10 bits in 4:2:0 (which this leaves holding the anchor's slot planes)"""
    slot, ref, prev = xpsnr_ref.anchor_planes()
    write(ctx, 0, slot)
    win = (0, 0, 208, 80)
    for flt, count, act in ((1, 16068, 51902667), (2, 3876, 23347468)):
        for temporal, act_t in ((1, (5518206, 2572495)[flt - 1]), (2, (9621541, 4562354)[flt - 1])):
            raw, _ = queued(L, ctx, 0, win, ref, prev[:temporal], block=64, filter_=flt)
            assert ([int(v) for v in raw.sse], int(raw.count), int(raw.act_spatial), int(raw.act_temporal)) == ([66503, 16628, 16624], count, act, act_t), (flt, temporal)
    for (block, flt, temporal), geometry, want in (((64, 1, 1), (64, 4, 2), [66.705086, 66.703637, 66.704496, 66.704747]),
                                                   ((0, 1, 1), (4, 52, 20), [66.113881, 66.090385, 66.091844, 66.106279]),
                                                   ((44, 2, 2), (44, 5, 2), [63.957842, 63.957782, 63.958692, 63.957974])):
        got = queued(L, ctx, 0, win, ref, prev[:temporal], block=block, filter_=flt)
        assert (got[0].block, got[0].blocks_x, got[0].blocks_y) == geometry
        same(got, xpsnr_ref.xpsnr_integers(slot, ref, prev[:temporal], block, flt), win, 10, "the anchor")
        rc, db = c_xpsnr(L, *got)
        assert rc == abi.VVR_OK and all(abs(g - w_) < 5e-7 for g, w_ in zip(db, want)), (db, want)


def ref_slot_case(L, ctx, slot, ref_slot, win, ps, pr, bd, what):
    """the prev planes in host memory: the same two for both directions"""
    prev = [np.ascontiguousarray(np.random.default_rng(1520 + k).integers(0, 1 << bd, ps[0].shape), np.uint16) for k in range(2)]
    for block, flt, temporal in ((0, 1, 2), (64, 2, 1), (44, 2, 0)):
        want = xpsnr_ref.xpsnr_integers(ps, pr, prev[:temporal], block, flt)
        same(queued(L, ctx, slot, win, ref_slot, prev[:temporal], block=block, filter_=flt), want, win, bd, what)


def stats_case(L, ctx, planes, bd):
    """vvr_get_stats: one k_output_xpsnr per request and nothing else; none with statistics off"""
    win = SUP.RING_WIN
    part = compare_ref.window_planes(planes, win)
    ref, prev = reference("noise", np.random.default_rng(5), part, bd)
    r16, p16 = forms(ref, prev)[0][1:]

    def request(k):
        def run():
            same(queued(L, ctx, 0, win, r16, p16[:k], filter_=1 + k % 2), xpsnr_ref.xpsnr_integers(part, ref, prev[:k], 0, 1 + k % 2), win, bd, "with statistics on")
        return run

    def verify(got):
        assert got == {"k_output_xpsnr": 3}, got
    return [request(k) for k in range(3)], verify, lambda: queued(L, ctx, 0, win, r16, p16)


def ring_request(L, ctx, planes, win, part, ref, bd):
    """against the ring's reference with two prev planes of this request's own, blocks of 44, the second filter"""
    _, prev = reference("noise", np.random.default_rng(6), part, bd)
    r16, p16 = forms(ref, prev)[0][1:]
    want = xpsnr_ref.xpsnr_integers(part, ref, prev, 44, 2)
    return lambda: submit(L, ctx, 0, win, r16, p16, block=44, filter_=2), lambda t, keep, what: same(collect(L, ctx, t, keep), want, win, bd, what)


# ---- tests

def test_the_structs_mirror_the_header(tmp_path):
    """sizeof / offsetof of the structs as gcc sees include/vvr.h == their ctypes mirrors; explicit pads only: the size is the sum of the fields"""
    names = [("vvr_xpsnr_block", abi.XpsnrBlock), ("vvr_frame_xpsnr", abi.FrameXpsnr), ("vvr_xpsnr_request", abi.XpsnrRequest)]
    SUP.assert_mirrors(tmp_path, names)
    for _, mirror in names:
        assert C.sizeof(mirror) == sum(C.sizeof(f[1]) for f in mirror._fields_) and C.sizeof(mirror) % 8 == 0
    assert (C.sizeof(abi.XpsnrBlock), C.sizeof(abi.FrameXpsnr), C.sizeof(abi.XpsnrRequest)) == (48, 128, 136) and BLOCK_DTYPE.itemsize == 48
    assert [BLOCK_DTYPE.fields[f[0]][1] for f in abi.XpsnrBlock._fields_] == [getattr(abi.XpsnrBlock, f[0]).offset for f in abi.XpsnrBlock._fields_]
    assert abi.VVR_ABI_VERSION == 5


def test_the_anchor_comes_out_of_the_restatement():
    """tests/xpsnr_ref.py alone: the totals and decibels the definition was checked with"""
    slot, ref, prev = xpsnr_ref.anchor_planes()
    for flt, count, act, act_t in ((1, 16068, 51902667, (5518206, 9621541)), (2, 3876, 23347468, (2572495, 4562354))):
        for temporal in (1, 2):
            r = xpsnr_ref.xpsnr_integers(slot, ref, prev[:temporal], 64, flt)
            assert (r["sse"], r["count"], r["act_spatial"], r["act_temporal"]) == ([66503, 16628, 16624], count, act, act_t[temporal - 1])
    for (block, flt, temporal), want in (((64, 1, 1), [66.705086, 66.703637, 66.704496, 66.704747]), ((0, 1, 1), [66.113881, 66.090385, 66.091844, 66.106279]),
                                         ((44, 2, 2), [63.957842, 63.957782, 63.958692, 63.957974])):
        got = xpsnr_ref.xpsnr(xpsnr_ref.xpsnr_integers(slot, ref, prev[:temporal], block, flt), 10)
        assert all(abs(g - w_) < 5e-7 for g, w_ in zip(got, want)), (got, want)


def test_block_sizes_and_the_geometry_call():
    L = SUP.stub_lib()
    for (w, h), b in (((3840, 2160), 128), ((1920, 1080), 64), ((1280, 720), 44), ((7680, 4320), 256), ((256, 128), 8), ((208, 80), 4)):
        assert xpsnr_ref.resolve_block(w, h) == b and abi.xpsnr_blocks(w, h)[0] == b
    out = [C.c_uint32(77) for _ in range(3)]

    def call(w, h, block, args=None):
        a = args or [C.byref(v) for v in out]
        return L.vvr_xpsnr_blocks(w, h, block, *a), tuple(v.value for v in out)

    for w, h, block in [(3840, 2160, 0), (1280, 720, 0), (208, 80, 0), (208, 80, 44), (8, 8, 4), (8, 8, 1 << 20), (512, 512, 4), (8192, 8192, 64), (131, 8, 4)]:
        b = block or xpsnr_ref.resolve_block(w, h)
        assert call(w, h, block) == (abi.VVR_OK, (b, -(-w // b), -(-h // b))) and abi.xpsnr_blocks(w, h, block) == (b, -(-w // b), -(-h // b))
    before = call(208, 80, 0)[1]
    for w, h, block in [(7, 8, 0), (8, 7, 0), (208, 80, 6), (208, 80, 2), (516, 512, 4), (8192, 8192, 60)]:      # (129 x 128 and 137 x 137 blocks)
        assert call(w, h, block) == (abi.VVR_ERR_PARAMETER, before) and abi.xpsnr_blocks(w, h, block) is None
    for k in range(3):
        a = [C.byref(v) for v in out]
        a[k] = None
        assert call(208, 80, 0, a) == (abi.VVR_ERR_PARAMETER, before)
    assert xpsnr_ref.resolve_filter(2048, 1152) == 1 and xpsnr_ref.resolve_filter(2048, 1154) == 2 and xpsnr_ref.resolve_filter(3840, 2160) == 2


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1530 + bd + cf)
    check_contents(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_what_follows_from_the_definition(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1540)
    check_consequences(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


def test_the_anchor_on_the_stand_in_runtime():
    L = SUP.stub_lib()
    ctx, _ = SUP.ctx_with(L, picture_size(1), 10, 1, 1541)
    check_anchor(L, ctx, SUP.writer(L))
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference_with_prev_planes_on_the_host(bd, cf):
    L = SUP.stub_lib()
    ctx, a = SUP.ctx_with(L, picture_size(cf), bd, cf, 1550)
    SUP.check_ref_slot("xpsnr", L, ctx, SUP.writer(L), a, SUP.noisy(a, bd, 1551), bd)
    L.vvr_destroy(ctx)


def test_the_three_homes_of_the_planes():
    """pageable memory (overwritten right after vvr_xpsnr_submit; one staging copy for the reference and the prev planes together), memory of
    vvr_host_alloc (no staging copy), a registered range (read in place); prev planes beside a ref_slot likewise; mixed homes and a prev plane
    partly inside a range are refused"""
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1560)
    SUP.write_picture(L, ctx, 1, SUP.noisy(planes, 10, 1561))
    rng = np.random.default_rng(1562)

    def h2d():
        n, b = C.c_size_t(), C.c_size_t()
        L.vvt_take_h2d(C.byref(n), C.byref(b))
        return n.value, b.value

    for win in WINDOWS[:3]:
        part = compare_ref.window_planes(planes, win)
        for bps in (2, 1):
            dt = np.uint16 if bps == 2 else np.uint8
            ref, prev = reference("random16", rng, part, 10, 8 * bps)
            want = xpsnr_ref.xpsnr_integers(part, ref, prev, 44, 1)
            what = "window %r, %d bytes per sample" % (win, bps)
            given, gprev = [SUP.padded(p, dt, 3) for p in ref], [SUP.padded(p, dt, 5) for p in prev]
            h2d()
            t, keep = submit(L, ctx, 0, win, given, gprev, block=44, filter_=1)
            assert t >= 2 and h2d()[0] == 1
            for g in given + gprev:
                g.base[...] = 0x33
            same(collect(L, ctx, t, keep), want, win, 10, "pageable, " + what)
            keepalive = []

            def pinned(n):
                return L.vvr_host_alloc(ctx, n)

            def registered(n):
                buf = np.zeros(n + 64, np.uint8)
                keepalive.append(buf)
                assert L.vvr_device_register(ctx, buf.ctypes.data, buf.nbytes) == abi.VVR_OK
                return buf.ctypes.data

            for home, alloc in (("vvr_host_alloc", pinned), ("a registered range", registered)):
                placed, bases = [], []
                for c, p in enumerate(ref + prev):
                    stride = p.shape[1] + (3, 5, 7, 9, 11)[c]
                    base = alloc(p.shape[0] * stride * bps)
                    assert base
                    bases.append(base)
                    a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                    a[...] = 0x44
                    a[:, :p.shape[1]] = p
                    placed.append(a[:, :p.shape[1]])
                h2d()
                t, keep = submit(L, ctx, 0, win, placed[:3], placed[3:], block=44, filter_=1)
                assert t >= 2, L.vvr_last_error(ctx)
                assert h2d()[0] == 0, "planes in pinned or device memory are not staged"
                same(collect(L, ctx, t, keep), want, win, 10, "%s, %s" % (home, what))
                if bps == 2:      # (a slot holds 16-bit words, and so do the prev planes beside it)
                    other = compare_ref.window_planes(SUP.noisy(planes, 10, 1561), win)
                    t, keep = submit(L, ctx, 0, win, 1, placed[3:4], block=44, filter_=1)
                    assert t >= 2, L.vvr_last_error(ctx)
                    same(collect(L, ctx, t, keep), xpsnr_ref.xpsnr_integers(part, other, prev[:1], 44, 1), win, 10, "ref_slot with prev in %s, %s" % (home, what))
                if home == "a registered range":
                    for mixed in ((placed[:3], [placed[3], placed[4].copy()]), ([placed[0], placed[1].copy(), placed[2]], placed[3:]), ([p.copy() for p in placed[:3]], placed[3:])):
                        t, _ = submit(L, ctx, 0, win, mixed[0], mixed[1])
                        assert t == abi.VVR_ERR_PARAMETER and b"mixed" in L.vvr_last_error(ctx) and b"vvr_xpsnr_submit" in L.vvr_last_error(ctx)
                    assert L.vvr_device_unregister(ctx, bases[4]) == abi.VVR_OK
                    assert L.vvr_device_register(ctx, bases[4], 1) == abi.VVR_OK
                    t, _ = submit(L, ctx, 0, win, placed[:3], placed[3:])
                    assert t == abi.VVR_ERR_PARAMETER and b"a prev plane lies partly inside" in L.vvr_last_error(ctx) and b"vvr_xpsnr_submit" in L.vvr_last_error(ctx)
                    t, _ = submit(L, ctx, 0, win, placed[:3], placed[3:4])      # (not looked at beyond `temporal`)
                    assert t >= 2 and L.vvr_output_wait(ctx, t) == abi.VVR_OK
                    for b_ in bases:
                        assert L.vvr_device_unregister(ctx, b_) == abi.VVR_OK
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1570)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    SUP.tickets_and_the_ring("xpsnr", L, ctx, planes, 10, ext)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernel():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1571)
    SUP.statistics("xpsnr", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_alone():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1572)
    SUP.write_picture(L, ctx, 1, planes)
    win = (8, 4, 200, 64)
    part = [np.ascontiguousarray(p) for p in compare_ref.window_planes(planes, win)]
    prev = [part[0].copy(), part[0].copy()]
    keep = abi.FrameXpsnr()

    refused = SUP.refuser(L, ctx, "xpsnr", lambda ref=part, w_=win, prev_=prev: abi.xpsnr_request(0, None, w_, ref, keep, prev_))

    # what only this request is refused for
    for w, h in [(6, 8), (8, 6), (2, 2), (6, 80), (208, 6)]:
        refused(b"below 8 x 8", ref=1, w_=(0, 0, w, h))
    refused(b"temporal must be", temporal=3)
    refused(b"temporal must be", temporal=255)
    refused(b"filter must be", filter=3)
    for block in (1, 2, 6, 63, 0xffffffff):
        refused(b"block must be 0 or a multiple of 4", block=block)
    for k in range(2):
        refused(b"missing prev plane or stride", **{"pplane%d" % k: None})
        refused(b"missing prev plane or stride", **{"pstride%d" % k: part[0].shape[1] * 2 - 1})
    req = abi.xpsnr_request(0, None, win, part, keep, prev[:1])      # (prev[1] is not looked at with temporal 1)
    req.prev[1], req.prev_stride_bytes[1] = None, 0
    t = L.vvr_xpsnr_submit(ctx, C.byref(req))
    assert t >= 2 and L.vvr_output_wait(ctx, t) == abi.VVR_OK
    # everything a comparison request is refused for
    refused(b"struct_size", struct_size=C.sizeof(abi.XpsnrRequest) - 8)
    refused(b"struct_size", struct_size=C.sizeof(abi.CompareRequest))
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
    bufs = [np.zeros(p.nbytes + 64, np.uint8) for p in part]
    for b_ in bufs:
        assert L.vvr_device_register(ctx, b_.ctypes.data, b_.nbytes) == abi.VVR_OK
    inside = [np.frombuffer(b_, np.uint16, p.size).reshape(p.shape) for b_, p in zip(bufs, part)]
    refused(b"mixed", ref=[inside[0], part[1], inside[2]], prev_=[])
    refused(b"mixed", ref=inside)      # (the prev planes are on the host)
    assert L.vvr_device_unregister(ctx, bufs[0].ctypes.data) == abi.VVR_OK
    assert L.vvr_device_register(ctx, bufs[0].ctypes.data, 1) == abi.VVR_OK
    refused(b"partly inside", ref=inside, prev_=[])
    for b_ in bufs:
        assert L.vvr_device_unregister(ctx, b_.ctypes.data) == abi.VVR_OK
    assert L.vvr_slot_picture_size(ctx, 1, W - 8, H_) == abi.VVR_OK
    refused(b"different sizes", ref=1)
    assert L.vvr_slot_picture_size(ctx, 1, W, H_) == abi.VVR_OK
    # a 4:0:0 context: odd windows are fine, planes 1 and 2 are not looked at
    ctx400, p400 = SUP.ctx_with(L, picture_size(0), 8, 0, 1573)
    refused(b"outside the picture", c=ctx400, ref=[p400[0]], w_=(0, 0, W400 + 1, 8), prev_=[])
    refused(b"below 8 x 8", c=ctx400, ref=[p400[0]], w_=(0, 0, W400, 7), prev_=[])
    L.vvr_destroy(ctx400)
    # more than 16384 blocks: 516 x 512 at B = 4 is 129 x 128 of them; 512 x 512 is accepted
    big = SUP.make_ctx(L, 520, 512, 8, 0)
    flat = [np.zeros((512, 520), np.uint16)]
    SUP.write_picture(L, big, 0, flat)
    refused(b"more than 16384 blocks", c=big, ref=[flat[0][:, :516]], w_=(0, 0, 516, 512), prev_=[], block=4)
    got = queued(L, big, 0, (0, 0, 512, 512), [flat[0][:, :512]], block=4, filter_=1)
    assert (got[0].blocks_x, got[0].blocks_y, int(got[0].count)) == (128, 128, 510 * 510) and got[1].shape == (16384,)
    L.vvr_destroy(big)
    assert L.vvr_xpsnr_submit(None, None) == abi.VVR_ERR_PARAMETER and L.vvr_xpsnr_submit(ctx, None) == abi.VVR_ERR_PARAMETER
    # the ring is untouched: eight requests still fit
    want = xpsnr_ref.xpsnr_integers(part, part, prev)
    SUP.eight_still_fit(L, ctx, lambda n: submit(L, ctx, 0, win, part if n % 2 else 1, prev), lambda t, got: same(collect(L, ctx, t, got), want, win, 10, "behind the refusals"))
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("xpsnr", SUP.stub_lib())


def failing(L, ctx, slot, win, job, ref_slot):
    zeros = XC.zeros_or_slot(win, None)
    return submit(L, ctx, slot, win, zeros if ref_slot is None else ref_slot, zeros[:1], job=job)


def delivered(keep):
    assert (keep[0].block, keep[0].blocks_x, keep[0].blocks_y, int(keep[0].count)) == (8, 32, 16, 254 * 126)


SUP.register("xpsnr", b"vvr_xpsnr_submit", ring_request, stats=stats_case, ref_slot=ref_slot_case, cases=windows, failing=failing,
             untouched=lambda k: bytes(k[0]) == bytes([SUP.FILL]) * C.sizeof(abi.FrameXpsnr) and k[1].tobytes() == bytes([SUP.FILL]) * k[1].nbytes, delivered=delivered)


def _hand(bd, nc, flt, w, h, records):
    raw = abi.FrameXpsnr()
    raw.struct_size, raw.bit_depth, raw.num_components, raw.filter, raw.block, raw.blocks_x, raw.blocks_y = C.sizeof(abi.FrameXpsnr), bd, nc, flt, 64, len(records), 1
    blocks = np.zeros(len(records), BLOCK_DTYPE)
    for k, (sse, act_s, act_t, count) in enumerate(records):
        blocks[k] = (sse, act_s, act_t, count, 0)
    for c in range(nc):
        raw.width[c], raw.height[c] = w >> (1 if c else 0), h >> (1 if c else 0)
        raw.samples[c] = raw.width[c] * raw.height[c]
    want = dict(blocks=blocks, filter=flt, num_components=nc, width=list(raw.width), height=list(raw.height), samples=list(raw.samples))
    return raw, blocks, want


def test_decibels_from_records_built_by_hand_and_the_overrides():
    L = SUP.stub_lib()
    rng = np.random.default_rng(1580)
    many = [([int(v) for v in rng.integers(0, 1 << 40, 3)], int(rng.integers(0, 1 << 36)), int(rng.integers(0, 1 << 34)), int(rng.integers(1, 1 << 14))) for _ in range(300)]
    cases = [("one block at the floor", 10, 3, 1, 128, 64, [([9, 4, 1], 0, 0, 100)]),
             ("a block without positions", 8, 3, 2, 128, 64, [([9, 4, 1], 0, 0, 0), ([100, 0, 7], 1000, 50, 10)]),
             ("nothing differs", 9, 3, 1, 64, 64, [([0, 0, 0], 700, 5, 62 * 62)]),
             ("chroma alone differs", 10, 3, 2, 64, 64, [([0, 5, 0], 70000, 5, 31 * 31)]),
             ("4:0:0", 8, 1, 1, 136, 8, [([33, 0, 0], 5000, 90, 6 * 62), ([1 << 50, 0, 0], 1 << 45, 1 << 44, 6 * 62)]),
             ("many blocks", 10, 3, 2, 3840, 2160, many)]
    for what, bd, nc, flt, w, h, records in cases:
        raw, blocks, want = _hand(bd, nc, flt, w, h, records)
        for a_pic, peak in ((0., 0.), (1.0, 0.), (0., 255. * 4), (7.5e5, 1020.), (-1., -1.)):
            rc, got = c_xpsnr(L, raw, blocks, a_pic, peak)
            assert rc == abi.VVR_OK, what
            close_enough(got, xpsnr_ref.xpsnr(want, bd, a_pic, peak), (what, a_pic, peak))
            # each wsse to a relative 1e-9: the decibels back to wsse
            ref_w = xpsnr_ref.block_wsse(want, bd, a_pic)
            pk = peak if peak > 0 else (1 << bd) - 1
            for c in range(nc):
                if ref_w[c]:
                    assert abs(pk * pk * want["samples"][c] / 10 ** (got[c] / 10) / ref_w[c] - 1) < 1e-9, (what, c)
        rc, got = c_xpsnr(L, raw, blocks)
        if what == "nothing differs":
            assert got == [math.inf] * 4
        if what == "chroma alone differs":
            assert got[0] == got[2] == math.inf and got[1] < got[3] < math.inf
        if what == "4:0:0":
            assert got[1] == got[2] == 0. and got[0] == got[3]
        if what == "one block at the floor":      # act = max( 1, 16 ) = 16, a_pic = 2^11 * sqrt( 8294400 / 8192 )
            w_k = math.sqrt(2048 * math.sqrt(8294400 / 8192.)) / 16
            assert abs(got[0] - 10 * math.log10(1023 ** 2 * 8192 / (w_k * 9))) < 1e-9
    # refusals: the output stays untouched
    raw, blocks, _ = _hand(10, 3, 1, 128, 64, [([9, 4, 1], 0, 0, 100)])
    untouched = [-1.] * 4
    assert c_xpsnr(L, None, blocks) == (abi.VVR_ERR_PARAMETER, untouched) and c_xpsnr(L, raw, None) == (abi.VVR_ERR_PARAMETER, untouched)
    assert L.vvr_compare_xpsnr(C.byref(raw), blocks.ctypes.data, 0., 0., None) == abi.VVR_ERR_PARAMETER
    for field, value in (("struct_size", C.sizeof(abi.FrameXpsnr) - 8), ("bit_depth", 7), ("bit_depth", 11), ("blocks_x", 0), ("blocks_y", 0), ("filter", 0), ("filter", 3)):
        bad = abi.FrameXpsnr.from_buffer_copy(bytes(raw))
        setattr(bad, field, value)
        assert c_xpsnr(L, bad, blocks) == (abi.VVR_ERR_PARAMETER, untouched), field
    bad = abi.FrameXpsnr.from_buffer_copy(bytes(raw))
    bad.samples[0] = 0
    assert c_xpsnr(L, bad, blocks) == (abi.VVR_ERR_PARAMETER, untouched)


def test_python_mirror_and_symbols():
    import vvdec_amd
    assert all(s in vvdec_amd.EXPORTED_SYMBOLS for s in ("vvr_xpsnr_submit", "vvr_xpsnr_blocks", "vvr_compare_xpsnr"))
    assert hasattr(vvdec_amd.Reconstructor, "xpsnr")
    assert abi.xpsnr_blocks(208, 80) == (4, 52, 20) and abi.xpsnr_blocks(208, 80, 44) == (44, 5, 2) and abi.xpsnr_blocks(3840, 2160) == (128, 30, 17)
