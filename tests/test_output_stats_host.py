"""CPU: light-level statistics as requests of the output queue (vvr_stats_submit, collected with vvr_output_test / vvr_output_wait) and the host
helper vvr_light_level, on the stand-in runtime of tests/hoststub, where launch_output_stats is a plain loop (vvr_output.inc, host only).  Planes
are uploaded with vvr_write_plane.  Expected values: np.bincount of the cropped luma; np.bincount, minimum and maximum over tests/rgb_ref.py's
"rgb16" planes of the crop (the numpy restatement of the definition in include/vvr.h).  Every comparison of statistics is exact.  The helpers take
a library and a context, so tests/test_gpu_output_stats.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import colour_transform_ref as X
import lut3d_ref as U
import output_support as SUP
import rgb_ref
import test_host_glue as T
import test_output_lut3d_host as LH
import test_output_queue_host as Q
import test_output_rgb_host as R
import test_output_semiplanar_host as S
from vvdec_amd import abi, stream, synth

pytestmark = T.pytestmark
W, H_ = 208, 80
# the smallest windows at which the kernels can go wrong (a workgroup of the RGB mode owns 64 x 32 samples, a lane 8 of a row)
WINDOWS = [(0, 0, 208, 80),       # several tiles in both directions, whole stores, a partial last tile
           (8, 4, 200, 64),       # offset origin, taps clamped to the window not to the picture
           (2, 2, 70, 34),        # width not a multiple of 8: the pair-by-pair instantiation; one tile plus a 6 x 2 remainder
           (0, 0, 2, 2)]          # the smallest window
COLOURS = [(1, 0), (9, 1)]        # BT.709 limited, BT.2020 full
CONTENTS = ["random", "flat", "runs", "extremes"]
# the 4:0:0 context of luma mode: windows at odd offsets and of odd sizes, rows that end inside a lane's 8 samples, one sample
W400, H400 = 136, 8
WINDOWS_400 = [(0, 0, 136, 8), (3, 1, 131, 5), (129, 7, 7, 1), (5, 2, 1, 1)]


def cases():
    """(window, collocated, colour): every window at every chroma position; the colour descriptions alternate"""
    out = []
    for win in WINDOWS:
        for c in range(4):
            out.append((win, (bool(c & 1), bool(c & 2)), COLOURS[(len(out) + len(out) // 4) % 2]))
    return out


def picture(kind, rng, w, h, bd, cf=1):
    """random: over the full range, with 0 and 2^bd - 1 in every plane.  flat: one value per plane.  runs: luma alternates every 5 samples of a row -
    runs that change inside a lane's 8 samples - over flat chroma.  extremes: Cb and Cr 0 and the maximum, changing at chroma column 20 and chroma row 10 -
    inside every window but the smallest - under luma at the maximum and, in every other stripe of 16 columns, at 0 (luma at the maximum alone
    clips R, G and B to the maximum only): each of R, G and B clips to 0 and to the maximum."""
    top = (1 << bd) - 1
    shapes = [(h >> s, w >> s) for s in ((0, 1, 1) if cf else (0,))]
    if kind == "random":
        return SUP.random_planes(rng, w, h, bd, cf)
    if kind == "flat":
        return [np.full(s, v, np.uint16) for s, v in zip(shapes, (3 * (top + 1) // 8 + 1, (top + 1) // 2 - 7, (top + 1) // 2 + 9))]
    if kind == "runs":
        luma = np.where((np.arange(w) // 5) % 2 == 0, top // 3, 2 * top // 3 + 1).astype(np.uint16)
        return [np.tile(luma, (h, 1))] + [np.full(s, (top + 1) // 2, np.uint16) for s in shapes[1:]]
    assert kind == "extremes"
    planes = [np.tile(np.where((np.arange(w) // 16) % 2 == 0, top, 0).astype(np.uint16), (h, 1))]
    if cf:
        cb, cr = np.zeros(shapes[1], np.uint16), np.zeros(shapes[2], np.uint16)
        cb[:, 20:] = top
        cr[:10, :] = top
        planes += [cb, cr]
    return planes


def crop(planes, win):
    x, y, w, h = win
    return [p[y >> s:(y + h) >> s, x >> s:(x + w) >> s] for p, s in zip(planes, (0, 1, 1))] if len(planes) == 3 else [planes[0][y:y + h, x:x + w]]


def expected(planes, bd, mode, colour=None, col=None):
    """the statistics of the planes of a window as numpy counts them"""
    zero = np.zeros(1024, np.int64)
    want = dict(hist_y=np.bincount(planes[0].ravel(), minlength=1024), hist_maxrgb=zero, max_c=[0, 0, 0], min_c=[0, 0, 0])
    if mode == abi.STATS_RGB:
        rgb = [p.astype(np.int64) for p in rgb_ref.rgb(planes, bd, "rgb16", colour[0], bool(colour[1]), col)]
        want.update(hist_maxrgb=np.bincount(np.maximum(np.maximum(rgb[0], rgb[1]), rgb[2]).ravel(), minlength=1024),
                    max_c=[int(p.max()) for p in rgb], min_c=[int(p.min()) for p in rgb])
    return want


def submit(L, ctx, slot, win, mode, col=(True, False), job=None, blocking=True):
    """one vvr_stats_submit -> (ticket or error, the vvr_frame_stats vvr_output_wait writes, filled with 0xaa)"""
    raw = abi.FrameStats()
    C.memset(C.addressof(raw), 0xaa, C.sizeof(raw))
    req = abi.stats_request(slot, job, win, mode, col, blocking, raw)
    return L.vvr_stats_submit(ctx, C.byref(req)), raw


def collect(L, ctx, ticket, raw):
    rc = L.vvr_output_wait(ctx, ticket)
    assert rc == abi.VVR_OK, (rc, L.vvr_last_error(ctx))
    return raw


def queued(L, ctx, slot, win, mode, **kw):
    t, raw = submit(L, ctx, slot, win, mode, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, raw)


def same(raw, want, win, bd, mode, what):
    """every field of the vvr_frame_stats, exactly"""
    assert (raw.struct_size, raw.mode, raw.bit_depth, raw.pad, raw.width, raw.height, raw.samples) == (C.sizeof(abi.FrameStats), mode, bd, 0, win[2], win[3], win[2] * win[3]), what
    for name in ("hist_y", "hist_maxrgb"):
        got = np.ctypeslib.as_array(getattr(raw, name)).astype(np.int64)
        assert np.array_equal(got, want[name]), "%s: %s differs in %d bins, first at %d" % (what, name, int((got != want[name]).sum()), int(np.argmax(got != want[name])))
        assert not got[1 << bd:].any()
    assert list(raw.max_c) == want["max_c"] and list(raw.min_c) == want["min_c"], "%s: max %r min %r, expected %r %r" % (what, list(raw.max_c), list(raw.min_c), want["max_c"], want["min_c"])
    assert int(want["hist_y"].sum()) == raw.samples and (mode == abi.STATS_LUMA or int(want["hist_maxrgb"].sum()) == raw.samples)


def check_content(L, ctx, planes, bd, kind):
    """both modes on every case for the picture in slot 0; what each kind of content is there for is asserted of the expectation too"""
    top = (1 << bd) - 1
    for win, col, colour in cases():
        what = "%s at %d bits, window %r collocated %r colour %r" % (kind, bd, win, col, colour)
        part = crop(planes, win)
        assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
        want = expected(part, bd, abi.STATS_RGB, colour, col)
        if kind == "flat":
            assert want["hist_y"].max() == win[2] * win[3] and want["hist_maxrgb"].max() == win[2] * win[3], "one bin holds every sample"
        if kind == "extremes" and win[2] > 2:
            assert want["max_c"] == [top] * 3 and want["min_c"] == [0] * 3
        if kind == "runs" and win[2] > 2:
            assert np.count_nonzero(want["hist_y"]) == 2 and np.count_nonzero(want["hist_maxrgb"]) >= 2
        same(queued(L, ctx, 0, win, abi.STATS_RGB, col=col), want, win, bd, abi.STATS_RGB, what + ", RGB mode")
        same(queued(L, ctx, 0, win, abi.STATS_LUMA, col=col), expected(part, bd, abi.STATS_LUMA), win, bd, abi.STATS_LUMA, what + ", luma mode")


def check_400(L, ctx, planes, bd):
    for win in WINDOWS_400:
        same(queued(L, ctx, 0, win, abi.STATS_LUMA), expected(crop(planes, win), bd, abi.STATS_LUMA), win, bd, abi.STATS_LUMA, "4:0:0, window %r" % (win,))


def check_flat_512x256(L, ctx, write):
    """one flat frame: a bin of 131 072, more than 16 bits - a workgroup's own count (2048 in RGB mode) would hide a 16-bit counter"""
    planes = picture("flat", None, 512, 256, 10)
    write(ctx, 0, planes)
    assert L.vvr_set_output_colour(ctx, 9, 0) == abi.VVR_OK
    win = (0, 0, 512, 256)
    want = expected(planes, 10, abi.STATS_RGB, (9, 0), (True, False))
    assert want["hist_y"].max() == 131072 and want["hist_maxrgb"].max() == 131072
    same(queued(L, ctx, 0, win, abi.STATS_RGB), want, win, 10, abi.STATS_RGB, "flat 512x256, RGB mode")
    same(queued(L, ctx, 0, win, abi.STATS_LUMA), expected(planes, 10, abi.STATS_LUMA), win, 10, abi.STATS_LUMA, "flat 512x256, luma mode")


def small_picture_in_a_larger_slot(L, ctx, write, rng):
    """a 256x144 context, slot 1 declared to hold a 200x72 picture: windows are windows of the picture, its edge is where the taps clamp"""
    full = SUP.random_planes(rng, 256, 144, 10, 1)
    write(ctx, 1, full)
    assert L.vvr_slot_picture_size(ctx, 1, 200, 72) == abi.VVR_OK
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    pic = [full[0][:72, :200], full[1][:36, :100], full[2][:36, :100]]
    win = (0, 0, 200, 72)
    same(queued(L, ctx, 1, win, abi.STATS_RGB), expected(pic, 10, abi.STATS_RGB, (1, 0), (True, False)), win, 10, abi.STATS_RGB, "200x72 in 256x144")
    t, _ = submit(L, ctx, 1, (0, 0, 202, 72), abi.STATS_RGB)
    assert t == abi.VVR_ERR_PARAMETER and b"outside the picture" in L.vvr_last_error(ctx)


def stats_case(L, ctx, planes, bd):
    """vvr_get_stats: one k_output_stats (and one k_output_stats_sum) per request of either mode; none with statistics off"""
    win = SUP.RING_WIN

    def request(mode):
        def run():
            same(queued(L, ctx, 0, win, mode), expected(crop(planes, win), bd, mode, (1, 0), (True, False)), win, bd, mode, "with statistics on")
        return run

    def verify(got):
        assert got.get("k_output_stats") == 3 and got.get("k_output_stats_sum") == 3 and "k_output_rgb" not in got, got
    return [request(mode) for mode in (abi.STATS_RGB, abi.STATS_LUMA, abi.STATS_RGB)], verify, lambda: queued(L, ctx, 0, win, abi.STATS_RGB)


def rgb_requests_around_a_statistics_request(L, ctx, planes, bd):
    """an RGB output request before and after a statistics request stores the bytes it stores without one"""
    win, col = (2, 2, 70, 34), (False, True)
    want = rgb_ref.rgb(crop(planes, win), bd, "rgb16", 1, False, col)
    t0, o0 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    t1, raw = submit(L, ctx, 0, win, abi.STATS_RGB, col=col)
    t2, o2 = Q.submit(L, ctx, 0, win, "rgb16", 3, col=col)
    assert min(t0, t1, t2) >= 2, L.vvr_last_error(ctx)
    R.same_bytes(Q.collect(L, ctx, t2, o2), want, "behind a statistics request")
    same(collect(L, ctx, t1, raw), expected(crop(planes, win), bd, abi.STATS_RGB, (1, 0), col), win, bd, abi.STATS_RGB, "between two RGB requests")
    R.same_bytes(Q.collect(L, ctx, t0, o0), want, "ahead of a statistics request")


def colour_snapshot(L, ctx, planes, bd):
    """vvr_set_output_colour behind vvr_stats_submit does not change the request in flight"""
    win, col = (8, 4, 200, 64), (True, True)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    t0, r0 = submit(L, ctx, 0, win, abi.STATS_RGB, col=col)
    assert L.vvr_set_output_colour(ctx, 9, 1) == abi.VVR_OK
    t1, r1 = submit(L, ctx, 0, win, abi.STATS_RGB, col=col)
    assert min(t0, t1) >= 2
    w0, w1 = [expected(crop(planes, win), bd, abi.STATS_RGB, colour, col) for colour in ((1, 0), (9, 1))]
    assert not np.array_equal(w0["hist_maxrgb"], w1["hist_maxrgb"])
    same(collect(L, ctx, t1, r1), w1, win, bd, abi.STATS_RGB, "second")
    same(collect(L, ctx, t0, r0), w0, win, bd, abi.STATS_RGB, "first")


def ring_request(L, ctx, planes, win, part, ref, bd):
    """luma and RGB statistics in turn (the colour description is BT.709, limited range)"""
    modes = []

    def start():
        modes.append(len(modes) % 2)
        t, raw = submit(L, ctx, 0, win, modes[-1])
        return t, (raw, modes[-1])

    def finish(t, keep, what):
        raw, mode = keep
        same(collect(L, ctx, t, raw), expected(part, bd, mode, (1, 0), (True, False)), win, bd, mode, what)
    return start, finish


# ---- the PQ EOTF and vvr_light_level restated

def light_level(hist, max_c, bd, samples, transfer, percentile_e4):
    M = (1 << bd) - 1
    hist = [int(v) for v in hist]
    max_code = max(v for v in range(1024) if hist[v])
    cum, pct_code = 0, None
    for v in range(1024):
        cum += hist[v]
        if pct_code is None and cum * 10000 >= percentile_e4 * samples:
            pct_code = v
    out = dict(max_code=max_code, pct_code=pct_code, max_nits=0., pct_nits=0., avg_nits=0., maxscl_nits=[0., 0., 0.])
    if transfer == 16:
        eotf = lambda code: float(X.pq_eotf(np.float64(code) / M))
        total = 0.
        for v in range(1024):
            if hist[v]:
                total += hist[v] * eotf(v)
        out.update(max_nits=eotf(max_code), pct_nits=eotf(pct_code), avg_nits=total / samples, maxscl_nits=[eotf(c) for c in max_c])
    return out


def frame_stats(hist, max_c, bd, samples=None, mode=abi.STATS_RGB):
    st = abi.FrameStats()
    st.struct_size, st.mode, st.bit_depth, st.width, st.height = C.sizeof(abi.FrameStats), mode, bd, 1, 1
    st.samples = sum(int(v) for v in hist) if samples is None else samples
    for v in range(1024):
        st.hist_maxrgb[v] = int(hist[v])
    for k in range(3):
        st.max_c[k] = max_c[k]
    return st


def c_light_level(L, st, transfer, percentile_e4):
    out = abi.LightLevel()
    C.memset(C.addressof(out), 0xaa, C.sizeof(out))
    rc = L.vvr_light_level(C.byref(st) if st is not None else None, transfer, percentile_e4, C.byref(out))
    return rc, out


def same_light_level(got, want, what):
    assert (got.struct_size, got.max_code, got.pct_code) == (C.sizeof(abi.LightLevel), want["max_code"], want["pct_code"]), (what, got.max_code, got.pct_code, want)
    pairs = [(got.max_nits, want["max_nits"]), (got.pct_nits, want["pct_nits"]), (got.avg_nits, want["avg_nits"])] + list(zip(got.maxscl_nits, want["maxscl_nits"]))
    for g, w_ in pairs:
        # relative 1e-9: orders of magnitude above the summation error of at most 1024 positive doubles (1024 x 2^-53 = 1.1e-13) and the few ulp by
        # which pow differs between libm and numpy, and far below one 10-bit PQ code step (about 1 % of the value)
        assert g == w_ or abs(g - w_) <= 1e-9 * abs(w_), (what, g, w_)


def loop_from_statistics_to_the_lut(L, ctx, write, rng):
    """the loop of the header: a frame whose content peaks well below the container's 10000 cd/m2 -> statistics -> vvr_light_level -> its pct_nits
    as src_peak_nits of vvr_output_lut3d_preset -> vvr_set_output_lut3d -> an RGB8 request.  Its bytes are those of tests/lut3d_ref.py under
    the same LUT, built in Python from the measured peak; they differ from the bytes under the static 10000-nit LUT."""
    bd, win, col, colour = 10, (0, 0, W, H_), (True, False), (9, 0)
    planes = [rng.integers(64, 520, (H_, W), dtype=np.uint16), rng.integers(490, 534, (H_ // 2, W // 2), dtype=np.uint16), rng.integers(490, 534, (H_ // 2, W // 2), dtype=np.uint16)]
    write(ctx, 0, planes)
    assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
    LH.set_lut(L, ctx, None)
    raw = queued(L, ctx, 0, win, abi.STATS_RGB, col=col)
    want = expected(planes, bd, abi.STATS_RGB, colour, col)
    same(raw, want, win, bd, abi.STATS_RGB, "the frame of the loop")
    rc, ll = c_light_level(L, raw, 16, 9995)
    assert rc == abi.VVR_OK
    same_light_level(ll, light_level(want["hist_maxrgb"], want["max_c"], bd, W * H_, 16, 9995), "the frame of the loop")
    assert 10 < ll.pct_nits < 400, "the content peaks well below the container's peak"
    frames = {}
    for name, peak in (("measured", ll.pct_nits), ("static", 10000.)):
        rc, nodes = LH.c_preset(L, 17, 16, 9, abi.XFORM_TO_SRGB, peak, 100.)
        assert rc == abi.VVR_OK
        built = U.preset(17, 16, 9, abi.XFORM_TO_SRGB, peak, 100.)
        assert np.abs(nodes.astype(np.int64) - built).max() <= 1      # (a pow of libm and of numpy may differ in the last place and flip a rounding: test_output_lut3d_host)
        LH.set_lut(L, ctx, (17, nodes))
        frames[name] = Q.queued(L, ctx, 0, win, "rgb8", 3, col=col)
        R.same_bytes(frames[name], U.frame(planes, bd, "rgb8", colour[0], bool(colour[1]), col, 17, nodes), "rgb8 under the %s LUT" % name)
    assert any(not np.array_equal(a, b) for a, b in zip(frames["measured"], frames["static"]))
    LH.set_lut(L, ctx, None)


# ---- tests

def test_the_structs_mirror_the_header(tmp_path):
    """sizeof / offsetof of the three structs as gcc sees include/vvr.h == their ctypes mirrors (vvr_abi_sizeof does not list them: they are
    guarded by their own struct_size)"""
    names = [("vvr_frame_stats", abi.FrameStats), ("vvr_stats_request", abi.StatsRequest), ("struct vvr_light_level", abi.LightLevel)]
    SUP.assert_mirrors(tmp_path, names)
    assert C.sizeof(abi.FrameStats) == 32 + 8192 + 24


def test_the_cases_meet_every_instantiation_of_the_kernel():
    """RGB mode is compiled once per (chroma position, kind of store): 8 instantiations, each met by two windows with values compared; both colour
    descriptions meet every window"""
    met = {}
    for win, col, colour in cases():
        met.setdefault((col, win[2] % 8 == 0), set()).add(win)
    assert len(met) == 8 and all(len(w) == 2 for w in met.values())
    assert all(set(c for w, _, c in cases() if w == win) == set(COLOURS) for win in WINDOWS)
    # luma mode: rows that end inside a lane's 8 samples and rows that do not, and more than one workgroup (16 384 samples each)
    assert any(w % 8 for _, _, w, _ in WINDOWS) and any(w % 8 == 0 for _, _, w, _ in WINDOWS) and W * H_ > 16384


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("bd", [10, 8, 9])
def test_statistics_of_every_case(bd, kind):
    L = SUP.stub_lib()
    planes = picture(kind, np.random.default_rng(900 + bd), W, H_, bd)
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    SUP.write_picture(L, ctx, 0, planes)
    check_content(L, ctx, planes, bd, kind)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_luma_mode_in_a_400_context(bd):
    L = SUP.stub_lib()
    planes = picture("random", np.random.default_rng(910 + bd), W400, H400, bd, 0)
    ctx = SUP.make_ctx(L, W400, H400, bd, 0)
    SUP.write_picture(L, ctx, 0, planes)
    check_400(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_a_flat_512x256_frame_needs_32_bit_counts():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, 512, 256, 10, 1)
    check_flat_512x256(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p))
    L.vvr_destroy(ctx)


def test_the_picture_in_the_slot_not_the_slot():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, 256, 144, 10, 1)
    small_picture_in_a_larger_slot(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(920))
    L.vvr_destroy(ctx)


def _random_ctx(L, seed, bd=10):
    planes = picture("random", np.random.default_rng(seed), W, H_, bd)
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    SUP.write_picture(L, ctx, 0, planes)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    return ctx, planes


def test_tickets_are_shared_with_output_and_hash_requests():
    L = SUP.stub_lib()
    ctx, planes = _random_ctx(L, 921)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    SUP.tickets_and_the_ring("stats", L, ctx, planes, 10, ext)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernel():
    L = SUP.stub_lib()
    ctx, planes = _random_ctx(L, 922)
    SUP.statistics("stats", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_rgb_requests_around_a_statistics_request_store_the_same_bytes():
    L = SUP.stub_lib()
    ctx, planes = _random_ctx(L, 923)
    rgb_requests_around_a_statistics_request(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_a_request_takes_the_colour_description_set_when_it_is_submitted():
    L = SUP.stub_lib()
    ctx, planes = _random_ctx(L, 924)
    colour_snapshot(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_the_seed_chain_and_the_colour_state_alone():
    L = SUP.stub_lib()
    rng = np.random.default_rng(925)
    Wg, Hg = S.W, S.H_      # (film grain needs a frame wider than 128: the pictures of the grain tests)
    ctx, pic, bank = S.setup(L, lambda w, h: SUP.make_ctx(L, w, h, 10, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, 10)
    win = (8, 4, 200, 64)
    keep = abi.FrameStats()

    def refused(text, c=ctx, **kw):
        req = abi.stats_request(0, None, win, abi.STATS_RGB, (True, False), True, keep)
        for k, v in kw.items():
            setattr(req, k, v)
        rc = L.vvr_stats_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c) and b"vvr_stats_submit" in L.vvr_last_error(c), (kw, rc, L.vvr_last_error(c))

    refused(b"no colour description set")
    assert L.vvr_set_output_colour(ctx, 9, 1) == abi.VVR_OK
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, win, "planar16", 3, grain=True)
    assert L.vvr_set_film_grain_seed(ctx, 9) == abi.VVR_OK
    refused(b"struct_size", struct_size=C.sizeof(abi.StatsRequest) - 8)
    refused(b"no such slot", slot=7)
    refused(b"no such slot", slot=-1)
    refused(b"job must be", job=-2)
    refused(b"unknown mode", mode=2)
    refused(b"unknown mode", mode=255)
    refused(b"stats is NULL", stats=None)
    for x, y, w, h in [(Wg - 100, 0, 200, 64), (0, Hg - 2, 8, 4), (-2, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, 8, -2), (1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)]:
        refused(b"outside the picture, empty, or odd", x=x, y=y, w=w, h=h)
    ctx400 = SUP.make_ctx(L, W400, H400, 8, 0)
    assert L.vvr_set_output_colour(ctx400, 1, 0) == abi.VVR_OK
    refused(b"no chroma", c=ctx400, x=0, y=0, w=8, h=8)
    L.vvr_destroy(ctx400)
    assert L.vvr_stats_submit(None, None) == abi.VVR_ERR_PARAMETER and L.vvr_stats_submit(ctx, None) == abi.VVR_ERR_PARAMETER
    # the ring is untouched: eight requests still fit; the chain too: the first grained frame is the frame of seed 9; and the colour description
    flight = [Q.submit(L, ctx, 0, win, "planar16", 3, grain=True)] + [submit(L, ctx, 0, win, abi.STATS_RGB) for _ in range(7)]
    assert all(t >= 2 for t, _ in flight) and len(set(t for t, _ in flight)) == 8, [t for t, _ in flight]
    assert all(np.array_equal(a, b) for a, b in zip(Q.collect(L, ctx, flight[0][0], flight[0][1]), first))
    want = expected(crop(pic, win), 10, abi.STATS_RGB, (9, 1), (True, False))
    for t, raw in flight[1:]:
        same(collect(L, ctx, t, raw), want, win, 10, abi.STATS_RGB, "behind the refusals")
    L.vvr_destroy(ctx)


def test_not_ready_while_the_picture_is_with_its_worker():
    """as the hash request's test: the host stage of a B picture is held on its worker thread; a request without `blocking` comes back
    VVR_NOT_READY and takes no ring entry, the same request with `blocking` is accepted and delivers the statistics of the picture"""
    L = SUP.stub_lib()
    Wd, Hd = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = SUP.stream_ctx(L, Wd, Hd, nslots)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=611, tool_flags=T.TOOLS) for pl in plans[:2]]
    pics = [d.c() for d in descs]
    assert L.vvr_submit(ctx, C.byref(pics[0])) >= 0
    L.vvt_slow_b_pictures(300000)
    win = (0, 0, Wd, Hd)
    try:
        j1 = L.vvr_submit(ctx, C.byref(pics[1]))
        assert j1 >= 0
        for mode in (abi.STATS_RGB, abi.STATS_LUMA):
            t, _ = submit(L, ctx, plans[1].slot, win, mode, job=j1, blocking=False)
            assert t == abi.VVR_NOT_READY, (mode, t, L.vvr_last_error(ctx))
        t, _ = submit(L, ctx, plans[1].slot, win, abi.STATS_RGB, blocking=False)       # job -1: pictures are still with the workers
        assert t == abi.VVR_NOT_READY
        flight = [submit(L, ctx, plans[1].slot, win, abi.STATS_RGB, job=j1) for _ in range(8)]       # (no entry was lost to the attempts above)
    finally:
        L.vvt_slow_b_pictures(0)
    assert all(t >= 2 for t, _ in flight), [t for t, _ in flight]
    got = [collect(L, ctx, t, raw) for t, raw in flight]
    assert L.vvr_wait(ctx, j1) == abi.VVR_OK
    planes = Q.sync_read(L, ctx, plans[1].slot, win, 2, 3)
    for raw in got:
        same(raw, expected(planes, 10, abi.STATS_RGB, (1, 0), (True, False)), win, 10, abi.STATS_RGB, "the B picture")
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("stats", SUP.stub_lib())


def delivered(raw):
    assert raw.samples == raw.width * raw.height == 256 * 128


SUP.register("stats", b"vvr_stats_submit", ring_request, stats=stats_case,
             failing=lambda L, ctx, slot, win, job, ref_slot: submit(L, ctx, slot, win, abi.STATS_RGB if ref_slot is None else abi.STATS_LUMA, job=job),
             untouched=lambda raw: bytes(raw) == b"\xaa" * C.sizeof(abi.FrameStats), delivered=delivered)



HAND = [("a single bin", {700: 4321}, [700, 650, 12], 10),
        ("two bins at the boundary", {100: 9995, 900: 5}, [900, 880, 100], 10),
        ("three bins", {3: 1, 100: 9994, 200: 5}, [200, 190, 180], 8),
        ("the ends of the range", {0: 7, 511: 13}, [511, 0, 0], 9)]


@pytest.mark.parametrize("what,bins,max_c,bd", HAND)
def test_light_level_on_histograms_built_by_hand(what, bins, max_c, bd):
    L = SUP.stub_lib()
    hist = np.zeros(1024, np.int64)
    for v, n in bins.items():
        hist[v] = n
    st = frame_stats(hist, max_c, bd)
    for transfer in (16, 0):
        for pe4 in (1, 5000, 9994, 9995, 9996, 10000):
            rc, got = c_light_level(L, st, transfer, pe4)
            assert rc == abi.VVR_OK and got.transfer == transfer
            same_light_level(got, light_level(hist, max_c, bd, int(hist.sum()), transfer, pe4), "%s, transfer %d, percentile %d" % (what, transfer, pe4))
    if what == "two bins at the boundary":      # the >= : 99.95 % of 10000 samples is reached by the 9995 of the first bin, 99.96 % is not
        assert c_light_level(L, st, 0, 9995)[1].pct_code == 100 and c_light_level(L, st, 0, 9996)[1].pct_code == 900
        assert c_light_level(L, st, 0, 1)[1].pct_code == 100 and c_light_level(L, st, 0, 10000)[1].pct_code == 900
    if what == "three bins":
        assert c_light_level(L, st, 0, 1)[1].pct_code == 3 and c_light_level(L, st, 0, 2)[1].pct_code == 100 and c_light_level(L, st, 0, 10000)[1].pct_code == 200


def test_pq_checkpoints_of_the_restatement():
    """ST 2084: code 0 is 0 cd/m2, full scale 10000, E' = 0.5 about 92.2 (BT.2100)"""
    assert float(X.pq_eotf(np.float64(0))) == 0 and abs(float(X.pq_eotf(np.float64(1))) - 10000) < 1e-6 and abs(float(X.pq_eotf(np.float64(0.5))) - 92.2457) < 1e-3


def test_light_level_refusals_leave_the_result_untouched():
    L = SUP.stub_lib()
    hist = np.zeros(1024, np.int64)
    hist[100] = 10
    untouched = b"\xaa" * C.sizeof(abi.LightLevel)

    def refused(st, transfer=16, pe4=9995):
        rc, out = c_light_level(L, st, transfer, pe4)
        assert rc == abi.VVR_ERR_PARAMETER and bytes(out) == untouched

    good = frame_stats(hist, [100, 100, 100], 10)
    assert c_light_level(L, good, 16, 9995)[0] == abi.VVR_OK
    assert L.vvr_light_level(C.byref(good), 16, 9995, None) == abi.VVR_ERR_PARAMETER
    refused(None)
    for transfer in (18, 1, 14, -1):      # (HLG is relative: its presets ignore the source peak)
        refused(good, transfer=transfer)
    for pe4 in (0, 10001):
        refused(good, pe4=pe4)
    refused(frame_stats(hist, [100] * 3, 10, mode=abi.STATS_LUMA))
    refused(frame_stats(hist, [100] * 3, 10, samples=11))
    refused(frame_stats(np.zeros(1024, np.int64), [0] * 3, 10))
    refused(frame_stats(hist, [100] * 3, 12))
    bad = frame_stats(hist, [100] * 3, 10)
    bad.struct_size -= 8
    refused(bad)


def test_the_loop_from_statistics_to_the_lut():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    loop_from_statistics_to_the_lut(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(930))
    L.vvr_destroy(ctx)


def test_python_mirror_of_the_modes_and_symbols():
    import vvdec_amd
    assert (abi.STATS_LUMA, abi.STATS_RGB) == (0, 1) and abi.STATS_MODES == {"luma": 0, "rgb": 1}
    assert "vvr_stats_submit" in vvdec_amd.EXPORTED_SYMBOLS and "vvr_light_level" in vvdec_amd.EXPORTED_SYMBOLS
    assert all(hasattr(vvdec_amd.Reconstructor, f) for f in ("stats_submit", "stats_wait")) and callable(vvdec_amd.light_level)
    L = SUP.stub_lib()
    assert L.vvr_abi_sizeof(18) == 0      # (no new index: the structs carry their struct_size)
