"""CPU: the 3-D LUT stage of the RGB formats of the output queue (vvr_set_output_lut3d, vvr_output_lut3d_preset) and the .cube reader / writer of
the Python package, on the stand-in runtime of tests/hoststub, where launch_output_rgb is a plain loop (vvr_output.inc, host only).  The expected
bytes come from tests/lut3d_ref.py, a numpy restatement of the stage as include/vvr.h defines it, applied the way tests/test_output_transform_host.py
builds its expectation: for plain windows to the crop of the picture the test wrote, with grain or a size to the planes of the planar16 request of
the same window, size, grain and seed.  The preset's nodes are compared with float64 formulas written from the standards.  All comparisons of
frames are of bytes.  The helpers take a library and a context, so tests/output_lut3d_on_the_device.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import colour_transform_ref as X
import interleaved_ref as IR
import lut3d_ref as U
import output_support as SUP
import rgb_ref
import test_film_grain_host as H
import test_host_glue as T
import test_output_interleaved_host as I
import test_output_queue_host as Q
import test_output_rgb_host as R
import test_output_semiplanar_host as S
import test_output_transform_host as TH
from vvdec_amd import abi

pytestmark = T.pytestmark
W, H_ = S.W, S.H_
STRAIGHT = R.STRAIGHT
FORMATS = list(U.PLANAR) + IR.FORMATS           # every RGB format: three planar, rgbf32, six interleaved
COLOUR = TH.COLOUR
same = I.same_planes


def _setup(L, bd, seed):
    return S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(seed), bd)


def set_lut(L, ctx, lut):
    """lut: None or (n, nodes)"""
    if lut is None:
        rc = L.vvr_set_output_lut3d(ctx, 0, None)
    else:
        a = abi.lut3d_nodes(*lut)
        rc = L.vvr_set_output_lut3d(ctx, lut[0], a.ctypes.data)      # (copied: a may go)
    assert rc == abi.VVR_OK, L.vvr_last_error(ctx)


def both_ways(L, ctx, win, fmt, col, want, what, device, size=None, grain=False, seed=None):
    """the request into pageable memory (padded rows) and into device memory with rows back to back, compared with `want`"""
    if seed is not None:
        assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    same(Q.queued(L, ctx, 0, win, fmt, 3, size=size, col=col, grain=grain), want, what + ", pageable")
    device(L, ctx, 0, win, fmt, 3, want, what + ", device", seed=seed, size=size, grain=grain, stride_kind="row", mis=0, col=col)


def stores(b, fmt):
    """the planes of `fmt` from what lut3d_ref.base gives"""
    return [X.store(e, fmt) for e in b["e"]] if fmt in U.PLANAR else IR.pack(*IR.values(b, fmt), fmt)


# ---- the cases; tests/output_lut3d_on_the_device.py runs them on the device

def random_groups():
    """(window, collocated, colour, with a transform, n): every window of STRAIGHT (rows stored whole and pair by pair) at every chroma position,
    with and without a transform ahead of the LUT; the three sizes and the colour descriptions rotate.  Every group runs every RGB format."""
    out = []
    for win in STRAIGHT:
        for c in range(4):
            for xf in (False, True):
                out.append((win, (bool(c & 1), bool(c & 2)), R.COLOURS[len(out) % 8], xf, U.SIZES[len(out) % 3]))
    return out


def check_random(L, ctx, picture, bd, device=S.device_request, seed=700):
    rng = np.random.default_rng(seed + bd)
    assert I.set_norm(L, ctx, None) == abi.VVR_OK
    for win, col, colour, xf, n in random_groups():
        transform = X.random_transform(rng, bd) if xf else None
        nodes = U.random_lut(rng, n)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        TH.set_transform(L, ctx, transform)
        set_lut(L, ctx, (n, nodes))
        b = U.base(S.crop(picture, win), bd, colour[0], bool(colour[1]), col, n, nodes, transform)
        for fmt in FORMATS:
            what = "%s at %d bits under a random %d-point LUT, window %r collocated %r colour %r transform %r" % (fmt, bd, n, win, col, colour, xf)
            both_ways(L, ctx, win, fmt, col, stores(b, fmt), what, device)
    # behind a rescale, and - bit depths with grain - behind grain and a rescale: the stage reads the planes of `tmp`
    for k, (win, size, grain, fmt, col, colour) in enumerate(TH.random_cases(bd)[36:]):
        n, xf = U.SIZES[k % 3], bool(k & 1)
        transform = X.random_transform(rng, bd) if xf else None
        nodes = U.random_lut(rng, n)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        TH.set_transform(L, ctx, None)
        set_lut(L, ctx, None)
        assert L.vvr_set_film_grain_seed(ctx, 6500 + k) == abi.VVR_OK
        planes = Q.queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=grain)
        TH.set_transform(L, ctx, transform)
        set_lut(L, ctx, (n, nodes))
        want = U.frame(planes, bd, fmt, colour[0], bool(colour[1]), col, n, nodes, transform)
        what = "%s at %d bits under a random %d-point LUT, window %r size %r grain %r transform %r" % (fmt, bd, n, win, size, grain, xf)
        both_ways(L, ctx, win, fmt, col, want, what, device, size=size, grain=grain, seed=6500 + k)
    TH.set_transform(L, ctx, None)
    set_lut(L, ctx, None)


def check_extremes(L, ctx, picture, bd, device=S.device_request):
    """n = 17, the largest S: all nodes 65535 (the largest sum, 65535 * 4096 + 2048, gives 65535 again), all nodes 0, and 0 / 65535 by node parity"""
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    TH.set_transform(L, ctx, None)
    fmts = ["rgb16", "rgb8", "rgbf16", "rgb10a2", "rgbf32", "bgr24"]
    for name, nodes in (("65535", np.full(3 * 17 ** 3, 65535, np.uint16)), ("0", np.zeros(3 * 17 ** 3, np.uint16)), ("parity", U.parity(17))):
        set_lut(L, ctx, (17, nodes))
        for k, fmt in enumerate(fmts):
            win = STRAIGHT[k % 3]
            b = U.base(S.crop(picture, win), bd, COLOUR[0], bool(COLOUR[1]), (True, False), 17, nodes)
            if name != "parity":
                assert all((e == int(name)).all() for e in b["e"])
            else:
                assert all(len(np.unique(e)) > 100 for e in b["e"])
            both_ways(L, ctx, win, fmt, (True, False), stores(b, fmt), "%s at %d bits, a 17-point LUT with nodes %s" % (fmt, bd, name), device)
    set_lut(L, ctx, None)


def grey_picture(picture, bd):
    return [picture[0], np.full_like(picture[1], 1 << (bd - 1)), np.full_like(picture[2], 1 << (bd - 1))]


def check_grey(L, ctx, picture, bd, write, device=S.device_request):
    """chroma at mid-level everywhere: R = G = B, the three fractions tie in every pixel; a LUT whose six neighbours of a node all differ, so any
    rule for ties that moved weight would show"""
    grey = grey_picture(picture, bd)
    write(ctx, 0, grey)
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    TH.set_transform(L, ctx, None)
    for k, (win, fmt) in enumerate(zip(STRAIGHT, ("rgb16", "rgba16f", "rgb8"))):
        n = U.SIZES[k]
        nodes = U.neighbours_differ(n)
        planes = S.crop(grey, win)
        col = (bool(k & 1), bool(k & 2))
        r, g, b_ = rgb_ref.matrix_int(planes[0], rgb_ref.upsample(planes[1], bd, col), rgb_ref.upsample(planes[2], bd, col), COLOUR[0], bool(COLOUR[1]), bd, bd)[0]
        assert np.array_equal(r, g) and np.array_equal(g, b_) and len(np.unique(r)) > 100
        set_lut(L, ctx, (n, nodes))
        b = U.base(planes, bd, COLOUR[0], bool(COLOUR[1]), col, n, nodes)
        both_ways(L, ctx, win, fmt, col, stores(b, fmt), "%s at %d bits, a grey picture under a %d-point LUT" % (fmt, bd, n), device)
    set_lut(L, ctx, None)
    write(ctx, 0, picture)


def sync_reads(L, ctx, win, bd):
    """the synchronous calls on the window: vvr_read_output of every component, vvr_read_output_grain (bit depths with a bank)"""
    x, y, w, h = win
    out = []
    for c in range(3):
        s = 1 if c else 0
        a = np.zeros((h >> s, w >> s), np.uint16)
        assert L.vvr_read_output(ctx, 0, c, x >> s, y >> s, w >> s, h >> s, 2, a.ctypes.data, a.strides[0]) == abi.VVR_OK, L.vvr_last_error(ctx)
        out.append(a)
    if bd != 9:
        assert L.vvr_set_film_grain_seed(ctx, 77) == abi.VVR_OK
        rc, planes = H.read_grain(L, ctx, 0, win, 2, 3)
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        out += list(planes)
    return out


def check_snapshot_and_scope(L, ctx, picture, bd, p010=True):
    """a request takes the LUT that is set when it is submitted - two of different sizes in flight; the other formats and the synchronous calls
    never see it; NULL restores the plain bytes"""
    rng = np.random.default_rng(710 + bd)
    win, col = (2, 6, 202, 38), (True, False)
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    TH.set_transform(L, ctx, None)
    set_lut(L, ctx, None)
    plain = {fmt: Q.queued(L, ctx, 0, win, fmt, 3, col=col) for fmt in ["rgb16", "rgba8", "planar16"] + (["p010"] if p010 else []) + (["nv12"] if bd == 8 else [])}
    same(plain["rgb16"], rgb_ref.rgb(S.crop(picture, win), bd, "rgb16", COLOUR[0], bool(COLOUR[1]), col), "plain rgb16")
    plain_sync = sync_reads(L, ctx, win, bd)
    la, lb = (17, U.random_lut(rng, 17)), (65, U.random_lut(rng, 65))
    want = [U.frame(S.crop(picture, win), bd, "rgb16", COLOUR[0], bool(COLOUR[1]), col, *lut) for lut in (la, lb)]
    assert not all(np.array_equal(a, b) for a, b in zip(*want))
    set_lut(L, ctx, la)
    t0, o0 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    set_lut(L, ctx, lb)
    t1, o1 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    others = [(fmt, Q.submit(L, ctx, 0, win, fmt, 3, col=col)) for fmt in plain if not fmt.startswith("rgb")]
    set_lut(L, ctx, None)
    t2, o2 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    t3, o3 = Q.submit(L, ctx, 0, win, "rgba8", 3, col=col)
    assert min(t0, t1, t2, t3) >= 0, L.vvr_last_error(ctx)
    same(Q.collect(L, ctx, t2, o2), plain["rgb16"], "rgb16 after vvr_set_output_lut3d( NULL )")
    same(Q.collect(L, ctx, t3, o3), plain["rgba8"], "rgba8 after vvr_set_output_lut3d( NULL )")
    same(Q.collect(L, ctx, t0, o0), want[0], "the first of two requests in flight (17 points)")
    same(Q.collect(L, ctx, t1, o1), want[1], "the second of two requests in flight (65 points)")
    for fmt, (t, o) in others:
        assert t >= 0, L.vvr_last_error(ctx)
        same(Q.collect(L, ctx, t, o), plain[fmt], "%s with a LUT set" % fmt)
    set_lut(L, ctx, lb)
    same(sync_reads(L, ctx, win, bd), plain_sync, "the synchronous calls with a LUT set")
    set_lut(L, ctx, None)


# ---- the restatement

def test_the_restatement_on_values_worked_by_hand():
    assert [int(U.widen(v, 8)) for v in (0, 1, 255)] == [0, 257, 65535] and [int(U.widen(v, 10)) for v in (0, 1, 512, 1023)] == [0, 64, 32800, 65535]
    for bd in (8, 9, 10):      # correctly rounded: 65535 / M is no half-integer multiple anywhere
        M = (1 << bd) - 1
        v = np.arange(M + 1)
        assert np.array_equal(U.widen(v, bd), np.floor(v * 65535 / M + 0.5).astype(np.int64))
        # ... and the multiplication the kernel takes the division as: ( x * ( 2^39 / M + 1 ) ) >> 39 (Python integers: no overflow)
        assert all((x * ((1 << 39) // M + 1)) >> 39 == x // M for x in (int(t) * 65535 + (M >> 1) for t in v))
    n, s = 17, 12
    lut = np.zeros((n, n, n, 3), np.int64)      # [jb, jg, jr]
    lut[0, 0, 0], lut[0, 0, 1], lut[0, 1, 1], lut[1, 1, 1], lut[1, 0, 0], lut[1, 0, 1] = (100, 0, 0), (1100, 0, 7), (2100, 0, 0), (4100, 0, 0), (9, 9, 9), (50000, 0, 0)
    # r = 3000 > g = 2000 > b = 1000 inside cell 0: c1 steps along R, c2 along G
    e = U.interpolate([np.array([3000]), np.array([2000]), np.array([1000])], n, lut.reshape(-1))
    assert int(e[0][0]) == (100 * 1096 + 1100 * 1000 + 2100 * 1000 + 4100 * 1000 + 2048) >> s and int(e[2][0]) == (7 * 1000 + 2048) >> s and int(e[1][0]) == 0
    # r > b > g: c1 steps along R, c2 along B - node ( 1, 0, 1 )
    e = U.interpolate([np.array([3000]), np.array([1000]), np.array([2000])], n, lut.reshape(-1))
    assert int(e[0][0]) == (100 * 1096 + 1100 * 1000 + 50000 * 1000 + 4100 * 1000 + 2048) >> s
    # the top of the range: 65535 lies in the last cell, f = S - 1, and all nodes equal give that value back
    top = U.interpolate([np.array([65535])] * 3, n, np.full(3 * n ** 3, 65535))
    assert [int(c[0]) for c in top] == [65535] * 3
    for size in U.SIZES:
        assert (size - 1) << U.shift(size) == 65536
    assert len(set(tuple(U.neighbours_differ(17).reshape(17, 17, 17, 3)[j]) for j in [(5, 5, 5), (4, 5, 5), (6, 5, 5), (5, 4, 5), (5, 6, 5), (5, 5, 4), (5, 5, 6)])) == 7


def test_the_random_groups_meet_every_instantiation_of_the_kernel():
    """4 chroma positions x 2 kinds of store x with / without a transform, each with every format; every size with and without a transform"""
    met = set((col, win[2] % 8 == 0, xf) for win, col, _, xf, _ in random_groups())
    assert len(met) == 16
    assert set((n, xf) for _, _, _, xf, n in random_groups()) == set((n, xf) for n in U.SIZES for xf in (False, True))
    assert len(FORMATS) == 10 and len(TH.random_cases(10)[36:]) == 2 and len(TH.random_cases(8)[36:]) == 2


# ---- the queue

@pytest.mark.parametrize("bd", [10, 8])
def test_random_luts(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 720 + bd)
    check_random(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_extremes(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 730 + bd)
    check_extremes(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_ties_need_no_rule(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 740 + bd)
    check_grey(L, ctx, picture, bd, lambda c, slot, p: SUP.write_picture(L, c, slot, p))
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_snapshot_and_scope(bd):
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, bd, 750 + bd)
    check_snapshot_and_scope(L, ctx, picture, bd)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_lut_in_force():
    L = SUP.stub_lib()
    ctx, picture, bank = _setup(L, 10, 760)
    win, col = (8, 4, 200, 64), (True, False)
    assert L.vvr_set_output_colour(ctx, *COLOUR) == abi.VVR_OK
    rng = np.random.default_rng(761)
    first = (33, U.random_lut(rng, 33))
    want = U.frame(S.crop(picture, win), 10, "rgb16", COLOUR[0], bool(COLOUR[1]), col, *first)
    set_lut(L, ctx, first)
    other = U.random_lut(rng, 65)
    for n, nodes, text in [(16, other, b"17, 33 or 65"), (32, other, b"17, 33 or 65"), (0, other, b"17, 33 or 65"), (33, None, b"nodes is NULL"),
                           (-17, other, b"17, 33 or 65"), (66, other, b"17, 33 or 65"), (17, None, b"nodes is NULL")]:
        rc = L.vvr_set_output_lut3d(ctx, n, None if nodes is None else nodes.ctypes.data)
        assert rc == abi.VVR_ERR_PARAMETER and b"vvr_set_output_lut3d" in L.vvr_last_error(ctx) and text in L.vvr_last_error(ctx), (n, rc, L.vvr_last_error(ctx))
        same(Q.queued(L, ctx, 0, win, "rgb16", 3, col=col), want, "after a refused call (n = %d)" % n)
    assert L.vvr_set_output_lut3d(None, 0, None) == abi.VVR_ERR_PARAMETER
    # a LUT in a 4:0:0 context: set, and never met - RGB is refused there as ever
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    set_lut(L, ctx400, first)
    assert L.vvr_set_output_colour(ctx400, 1, 0) == abi.VVR_OK
    shapes, dt = abi.output_plane_shapes(win, "rgb16", None, 3)
    req = abi.output_request(0, None, win, "rgb16", None, col, False, True, [np.zeros(s, dt) for s in shapes])
    assert L.vvr_output_submit(ctx400, C.byref(req)) == abi.VVR_ERR_PARAMETER and b"no chroma" in L.vvr_last_error(ctx400)
    L.vvr_destroy(ctx400)
    L.vvr_destroy(ctx)


# ---- the preset

PRESETS = [(16, 9, X.TO_SRGB, 1000., 100.), (18, 9, X.TO_BT709, 1000., 100.), (18, 9, X.TO_SRGB, 1000., 1000.)]      # PQ 1000 -> 100 cd/m2, HLG on a 100 and a 1000 cd/m2 display


def c_preset(L, n, tc, cp, target, src, dst):
    nodes = np.zeros(3 * n ** 3, np.uint16)
    rc = L.vvr_output_lut3d_preset(nodes.ctypes.data, n, tc, cp, target, src, dst)
    return rc, nodes


@pytest.mark.parametrize("tc,cp,target,src,dst", PRESETS)
def test_preset_nodes_are_the_standards_formulas(tc, cp, target, src, dst):
    """every node equal to the float64 restatement, or 1 apart where a pow of libm and of numpy differ in their last place and a rounding flips;
    fewer than 1 % of the nodes may differ at all"""
    L = SUP.stub_lib()
    rc, nodes = c_preset(L, 17, tc, cp, target, src, dst)
    assert rc == abi.VVR_OK
    ref = U.preset(17, tc, cp, target, src, dst)
    d = np.abs(nodes.astype(np.int64) - ref)
    share = float((d != 0).mean())
    print("transfer %d primaries %d target %d, %g -> %g cd/m2: %.4f %% of the nodes differ, by at most %d" % (tc, cp, target, src, dst, 100 * share, int(d.max())))
    assert int(d.max()) <= 1 and share < 0.01, (int(d.max()), share)
    cube = nodes.reshape(17, 17, 17, 3)
    assert (cube[0, 0, 0] == 0).all() and len(np.unique(nodes)) > 1000
    if tc == 18:      # HLG: the nominal peak - scene light 1 in every channel - is display white
        assert (cube[16, 16, 16] == 65535).all()


def test_pq_preset_on_the_grey_axis_is_the_per_channel_preset():
    """luminance of grey is the channel value: on jr = jg = jb the curve on luminance is the per-channel curve of vvr_output_transform_preset
    taken at the node's value.  The per-channel side is the integer pipeline of the transform with the matrix and enc of the C preset; its
    stage 1 is q16 of the float64 formula at the node's value, because the nodes' values j * S / 65535 are not on the grid v / ( 2^bd - 1 ) of the
    preset's lin table (tests/test_output_transform_host.py holds that table to the same formula within 1).  Units and bounds:
      BT.709 primaries, linear target: stages 2 and 3 are exact (unit matrix, enc[i] = 64 i), so the two agree within 1 in 16-bit codes (rgb16);
      BT.2020 primaries to sRGB: within 1 in the 8-bit codes rgb8 stores, and in 16-bit codes within 21.25 + 0.5 - the distance of the
      per-channel integer pipeline from the real-valued one that test_output_transform_host.ACCURACY asserts (the Q14 matrix and the
      interpolated OETF), plus the rounding of the node, which is the real-valued result rounded once"""
    L = SUP.stub_lib()
    e = np.minimum(np.arange(17) * 4096, 65535) / 65535
    lin = np.floor(X.linear_light(e, 16, 1000., 100.) * 65535 + 0.5).astype(np.int64)      # stage 1 at the nodes' values
    for cp, target, bounds in ((1, X.TO_LINEAR, {"rgb16": 1}), (9, X.TO_SRGB, {"rgb8": 1, "rgb16": TH.ACCURACY[(16, 9, X.TO_SRGB)][1] + 0.5})):
        rc, nodes = c_preset(L, 17, 16, cp, target, 1000., 100.)
        rc2, t = TH.c_preset(L, 16, cp, target, (1000., 100.), 10)
        assert rc == abi.VVR_OK and rc2 == abi.VVR_OK
        _, m, enc = abi.output_transform_arrays(t)
        per_channel = X.stages([np.arange(17)] * 3, lin, m, enc)
        grey = nodes.reshape(17, 17, 17, 3)[np.arange(17), np.arange(17), np.arange(17)].astype(np.int64)
        for fmt, bound in bounds.items():
            for k in range(3):
                a, b = X.store(grey[:, k], fmt).astype(np.int64), X.store(per_channel[k], fmt).astype(np.int64)
                print("primaries %d target %d channel %d: largest distance %d codes of %s (bound %g)" % (cp, target, k, int(np.abs(a - b).max()), fmt, bound))
                assert np.abs(a - b).max() <= bound, (cp, target, fmt, k, a, b)


def test_preset_refuses_what_it_does_not_know():
    L = SUP.stub_lib()
    for args in [(16, 16, 9, 0, 1000., 100.), (0, 16, 9, 0, 1000., 100.), (129, 16, 9, 0, 1000., 100.), (17, 1, 9, 0, 1000., 100.), (17, 14, 9, 0, 1000., 100.),
                 (17, 16, 5, 0, 1000., 100.), (17, 18, 12, 0, 1000., 100.), (17, 16, 9, 3, 1000., 100.), (17, 16, 9, -1, 1000., 100.), (17, 16, 9, 0, 0., 100.),
                 (17, 16, 9, 0, 1000., -1.), (17, 16, 9, 0, 10001., 100.), (17, 16, 9, 0, float("nan"), 100.), (17, 18, 9, 0, 1000., 0.), (17, 18, 9, 0, 1000., float("nan"))]:
        nodes = np.full(3 * 17 ** 3, 0x5a5a, np.uint16)
        assert L.vvr_output_lut3d_preset(nodes.ctypes.data, *args) == abi.VVR_ERR_PARAMETER, args
        assert (nodes == 0x5a5a).all(), args
    assert L.vvr_output_lut3d_preset(None, 17, 16, 9, 0, 1000., 100.) == abi.VVR_ERR_PARAMETER
    assert c_preset(L, 33, 18, 9, 1, 0., 1000.)[0] == abi.VVR_OK      # (HLG ignores the source peak)


# ---- .cube files and the Python mirror

def test_cube_round_trip(tmp_path):
    import vvdec_amd
    for n in U.SIZES[:2]:
        nodes = U.random_lut(np.random.default_rng(770 + n), n)
        nodes[:4] = (0, 1, 65534, 65535)
        path = str(tmp_path / ("random%d.cube" % n))
        vvdec_amd.write_cube(path, n, nodes, title="random")
        n2, back = vvdec_amd.read_cube(path)
        assert n2 == n and back.dtype == np.uint16 and np.array_equal(back, nodes)


def test_cube_written_by_hand(tmp_path):
    import vvdec_amd
    path = str(tmp_path / "hand.cube")
    with open(path, "w") as f:
        f.write('# a grade\nTITLE "by hand"\n\nLUT_3D_SIZE 17\nDOMAIN_MIN 0.0 0.0 0.0\nDOMAIN_MAX 1.0 1.0 1.0\n')
        for jb in range(17):
            for jg in range(17):
                for jr in range(17):
                    f.write("%g %g\t%g   # node\n" % (jr / 16, jg / 16 * 1.5 - 0.25, jb / 16))      # (G leaves 0 .. 1 at both ends: clipped)
    n, nodes = vvdec_amd.read_cube(path)
    cube = nodes.reshape(17, 17, 17, 3)
    assert n == 17 and nodes.shape == (3 * 17 ** 3,)
    assert cube[3, 2, 1].tolist() == [4096, 0, 12288] and cube[16, 16, 16].tolist() == [65535] * 3 and cube[0, 8, 16].tolist() == [65535, 32768, 0]
    for text in ("LUT_3D_SIZE 16\n", "LUT_3D_SIZE 17\nDOMAIN_MAX 2 2 2\n", "LUT_3D_SIZE 17\n0 0 0\n", "LUT_1D_SIZE 17\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(ValueError):
            vvdec_amd.read_cube(path)


def test_python_mirror_of_the_symbols():
    import vvdec_amd
    assert "vvr_set_output_lut3d" in vvdec_amd.EXPORTED_SYMBOLS and "vvr_output_lut3d_preset" in vvdec_amd.EXPORTED_SYMBOLS
    assert hasattr(SUP.stub_lib(), "vvr_set_output_lut3d") and hasattr(SUP.stub_lib(), "vvr_output_lut3d_preset")
    assert hasattr(vvdec_amd.Reconstructor, "set_output_lut3d") and abi.LUT3D_SIZES == U.SIZES
    assert abi.lut3d_nodes(17, np.zeros((17, 17, 17, 3))).shape == (3 * 17 ** 3,)
    with pytest.raises(AssertionError):
        abi.lut3d_nodes(17, np.zeros(5))
