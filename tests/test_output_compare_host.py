"""CPU: a picture compared with a reference frame as a request of the output queue (vvr_compare_submit, collected with vvr_output_test /
vvr_output_wait) and the host helper vvr_compare_psnr, on the stand-in runtime of tests/hoststub, where launch_output_compare is a plain loop
(vvr_output.inc, host only).  Planes are uploaded with vvr_write_plane.  Expected values: tests/compare_ref.py, the numpy restatement of the
definition in include/vvr.h.  Every comparison of integers is exact.  The helpers take a library and a context, so
tests/test_gpu_output_compare.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import compare_ref
import output_support as SUP
import test_host_glue as T
import test_output_queue_host as Q
from vvdec_amd import abi, synth

pytestmark = T.pytestmark
W, H_ = 208, 80           # four blocks across with a 16-wide last one, two down with a 16-high last one
WINDOWS = [(0, 0, 208, 80), (8, 4, 200, 64), (2, 2, 70, 34), (0, 0, 2, 2)]
W400, H400 = 136, 8
WINDOWS_400 = [(0, 0, 136, 8), (3, 1, 131, 5), (129, 7, 7, 1), (5, 2, 1, 1)]
CONTENTS = ["identical", "last", "random", "partial", "two_hits"]


def picture_size(cf):
    return (W, H_) if cf else (W400, H400)


def windows(nc):
    return WINDOWS if nc == 3 else WINDOWS_400


def submit(L, ctx, slot, win, ref, with_map=True, job=None, blocking=True, bps=2):
    """one vvr_compare_submit -> (ticket or error, (the vvr_frame_compare, the map) vvr_output_wait writes, both filled with 0xaa)"""
    raw = abi.FrameCompare()
    C.memset(C.addressof(raw), SUP.FILL, C.sizeof(raw))
    blocks = np.full(abi.compare_map_shape(win), 0xaaaaaaaa, np.uint32) if with_map else None
    req = abi.compare_request(slot, job, win, ref, raw, blocks, blocking, bps)
    return L.vvr_compare_submit(ctx, C.byref(req)), (raw, blocks)


def collect(L, ctx, ticket, keep):
    rc = L.vvr_output_wait(ctx, ticket)
    assert rc == abi.VVR_OK, (rc, L.vvr_last_error(ctx))
    return keep


def queued(L, ctx, slot, win, ref, **kw):
    t, keep = submit(L, ctx, slot, win, ref, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, keep)


def same(got, want, win, bd, what):
    """every field of the vvr_frame_compare and every word of the map, exactly"""
    raw, blocks = got
    nc = want["num_components"]
    assert (raw.struct_size, raw.bit_depth, raw.num_components, raw.pad, raw.pad2) == (C.sizeof(abi.FrameCompare), bd, nc, 0, 0), what
    for name in ("width", "height", "samples", "differing", "sse", "sad", "max_abs", "first_x", "first_y"):
        assert [int(v) for v in getattr(raw, name)] == want[name], "%s: %s is %r, expected %r" % (what, name, [int(v) for v in getattr(raw, name)], want[name])
    assert want["width"][0] == win[2] and want["height"][0] == win[3]
    if blocks is not None:
        assert np.array_equal(blocks.astype(np.int64), want["map"]), "%s: the map is\n%r, expected\n%r" % (what, blocks, want["map"])
        assert int(blocks.astype(np.int64).sum()) == sum(want["differing"])


def reference(kind, rng, part, bd, bytes_per_sample=2):
    """the reference planes of a window whose slot planes are `part`, as int64 arrays; what the content is there for is asserted of it"""
    ref = [p.astype(np.int64) for p in part]
    nc = len(part)
    if kind == "identical":
        return ref
    if kind.startswith("last"):        # one sample differs at the LAST position of the window, in component `c`
        c = int(kind[4:])
        ref[c][-1, -1] ^= 1
        return ref
    if kind == "random":               # about half of the samples differ, by anything the reference's format holds
        top = 0xffff if bytes_per_sample == 2 else 0xff
        for c in range(nc):
            other = rng.integers(0, top + 1, ref[c].shape, dtype=np.int64)
            ref[c] = np.where((rng.random(ref[c].shape) < 0.5) & (ref[c] <= top), ref[c], other)
        return ref
    if kind == "partial":              # differences only inside the partial right-hand and bottom blocks
        for c in range(nc):
            side = 32 if c else 64
            h, w = ref[c].shape
            jj, ii = np.mgrid[0:h, 0:w]
            mask = ((ii >= w // side * side) & (w % side != 0)) | ((jj >= h // side * side) & (h % side != 0))
            ref[c] = np.where(mask, ref[c] ^ 3, ref[c])
        return ref
    assert kind == "two_hits"          # one hit in row 0 of block (1, 0), one in row 1 of block (0, 0): the former is the first
    for c in range(nc):
        side = 32 if c else 64
        h, w = ref[c].shape
        if w > side + 5 and h > 1:
            ref[c][0, side + 5] ^= 1
            ref[c][1, 3] ^= 1
    return ref


def kinds(nc):
    return [k for k in CONTENTS if k != "last"] + ["last%d" % c for c in range(nc)]


def check_contents(L, ctx, planes, bd):
    """every content at every window in every form, for the picture `planes` in slot 0"""
    nc = len(planes)
    rng = np.random.default_rng(1300 + bd + nc)
    met_two_hits = 0
    for win in windows(nc):
        part = compare_ref.window_planes(planes, win)
        for kind in kinds(nc):
            for bps in (2, 1):
                if bps == 1 and kind != "random" and any(int(p.max()) > 255 for p in part):
                    continue
                ref = reference(kind, rng, part, bd, bps)
                want = compare_ref.compare(part, ref)
                if kind == "identical":
                    assert sum(want["differing"]) == 0 and want["first_x"] == [compare_ref.NONE] * 3 and not want["map"].any()
                if kind.startswith("last"):
                    c = int(kind[4:])
                    assert want["differing"][c] == 1 and sum(want["differing"]) == 1 and (want["first_x"][c], want["first_y"][c]) == (want["width"][c] - 1, want["height"][c] - 1)
                if kind == "two_hits" and want["differing"][0]:
                    met_two_hits += 1
                    assert (want["first_x"][0], want["first_y"][0]) == (69, 0) and want["differing"][0] == 2 and want["map"][0, 0] >= 1 and want["map"][0, 1] >= 1
                for name, given in [f for f in SUP.forms(ref) if (f[0] == "8-bit") == (bps == 1)]:
                    same(queued(L, ctx, 0, win, given), want, win, bd, "%s at %d bits, window %r, %s reference" % (kind, bd, win, name))
        # (without a map nothing but the result is written)
        want = compare_ref.compare(part, part)
        got = queued(L, ctx, 0, win, [np.ascontiguousarray(p, np.uint16) for p in part], with_map=False)
        same(got, want, win, bd, "no map, window %r" % (win,))
    assert met_two_hits >= 2


def check_all_ones_reference(L, ctx, write, nc, bd):
    """slot 0 holds zeros, the reference 0xffff: every d * d is 4 294 836 225 and every sum needs 64 bits"""
    w, h = (W, H_) if nc == 3 else (W400, H400)
    zero = [np.zeros((h >> s, w >> s), np.uint16) for s in ((0, 1, 1) if nc == 3 else (0,))]
    write(ctx, 0, zero)
    for win in windows(nc):
        part = compare_ref.window_planes(zero, win)
        ref = [np.full(p.shape, 0xffff, np.int64) for p in part]
        want = compare_ref.compare(part, ref)
        assert want["sse"][:nc] == [n * 4294836225 for n in want["samples"][:nc]] and want["sad"][:nc] == [n * 65535 for n in want["samples"][:nc]]
        assert win[2] * win[3] < 4096 or want["sse"][0] > 1 << 32
        for name, given in SUP.forms(ref):
            same(queued(L, ctx, 0, win, given), want, win, bd, "zeros against 0xffff, window %r" % (win,))


def check_outside(L, ctx, write, planes, bd):
    """samples that differ only just outside the window, on each of its four sides: nothing is reported - with the reference given as planes (the
    window of the undisturbed picture) and as a second slot (the undisturbed picture in slot 1)"""
    nc = len(planes)
    write(ctx, 1, planes)
    for win in windows(nc):
        x, y, w, h = win
        other = [p.copy() for p in planes]
        sides = 0
        for c, p in enumerate(other):
            s = 1 if c and nc == 3 else 0
            x0, y0, x1, y1 = x >> s, y >> s, (x + w) >> s, (y + h) >> s
            if x0 > 0:
                p[:, x0 - 1] ^= 1
            if y0 > 0:
                p[y0 - 1, :] ^= 1
            if x1 < p.shape[1]:
                p[:, x1] ^= 1
            if y1 < p.shape[0]:
                p[y1, :] ^= 1
            sides += (x0 > 0) + (y0 > 0) + (x1 < p.shape[1]) + (y1 < p.shape[0])
        assert sides >= 2 * nc or win[:2] == (0, 0)
        write(ctx, 0, other)
        part = compare_ref.window_planes(planes, win)
        want = compare_ref.compare(part, part)
        same(queued(L, ctx, 0, win, [np.ascontiguousarray(p, np.uint16) for p in part]), want, win, bd, "outside window %r" % (win,))
        same(queued(L, ctx, 0, win, 1), want, win, bd, "outside window %r, against slot 1" % (win,))
        # (the whole picture, when the window is not it, does differ)
        full = (0, 0, planes[0].shape[1], planes[0].shape[0])
        if sides:
            got = queued(L, ctx, 0, full, 1)
            same(got, compare_ref.compare(other, planes), full, bd, "the disturbed picture against slot 1")
            assert got[0].differing[0] > 0
    write(ctx, 0, planes)


def ref_slot_case(L, ctx, slot, ref_slot, win, ps, pr, bd, what):
    same(queued(L, ctx, slot, win, ref_slot), compare_ref.compare(ps, pr), win, bd, what)


def stats_case(L, ctx, planes, bd):
    """vvr_get_stats: one k_output_compare and one k_output_compare_sum per request; none with statistics off"""
    win = SUP.RING_WIN
    part = compare_ref.window_planes(planes, win)
    ref = reference("random", np.random.default_rng(5), part, bd)

    def request():
        same(queued(L, ctx, 0, win, SUP.forms(ref)[0][1]), compare_ref.compare(part, ref), win, bd, "with statistics on")

    def verify(got):
        assert got == {"k_output_compare": 3, "k_output_compare_sum": 3}, got
    return [request] * 3, verify, request


def ring_request(L, ctx, planes, win, part, ref, bd):
    given, want = SUP.forms(ref)[0][1], compare_ref.compare(part, ref)
    return lambda: submit(L, ctx, 0, win, given), lambda t, keep, what: same(collect(L, ctx, t, keep), want, win, bd, what)


def c_psnr(L, raw, peak):
    out = (C.c_double * 4)(-1., -1., -1., -1.)
    return L.vvr_compare_psnr(C.byref(raw) if raw is not None else None, peak, out), list(out)


def check_psnr(L, raw, want, bd, what):
    for peak in (0., float(255 << (bd - 8)), 1.0):
        rc, got = c_psnr(L, raw, peak)
        assert rc == abi.VVR_OK
        ref = compare_ref.psnr(want, bd, peak)
        for g, w_ in zip(got, ref):
            # 1e-9 dB: a handful of double operations and one log10, each good to an ulp (of values below 200)
            assert g == w_ or abs(g - w_) <= 1e-9, (what, peak, got, ref)


# ---- tests

def test_the_structs_mirror_the_header(tmp_path):
    """sizeof / offsetof of the structs as gcc sees include/vvr.h == their ctypes mirrors (vvr_abi_sizeof does not list them: they are guarded by
    their own struct_size)"""
    names = [("vvr_frame_compare", abi.FrameCompare), ("vvr_compare_request", abi.CompareRequest)]
    SUP.assert_mirrors(tmp_path, names)
    assert C.sizeof(abi.FrameCompare) == 176
    L = SUP.stub_lib()
    assert L.vvr_abi_sizeof(18) == 0      # (no new index)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1200 + bd + cf)
    check_contents(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_sums_that_need_64_bits(bd, cf):
    L = SUP.stub_lib()
    ctx, _ = SUP.ctx_with(L, picture_size(cf), bd, cf, 1210)
    check_all_ones_reference(L, ctx, SUP.writer(L), 3 if cf else 1, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_differences_just_outside_the_window_are_not_reported(bd, cf):
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(cf), bd, cf, 1220)
    check_outside(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference(bd, cf):
    L = SUP.stub_lib()
    ctx, a = SUP.ctx_with(L, picture_size(cf), bd, cf, 1230)
    b = [np.where(np.random.default_rng(1231 + c).random(p.shape) < 0.3, p ^ 5, p).astype(np.uint16) for c, p in enumerate(a)]
    SUP.check_ref_slot("compare", L, ctx, SUP.writer(L), a, b, bd)
    L.vvr_destroy(ctx)


def test_a_slot_holding_values_above_the_bit_depth_is_read_as_it_lies():
    """16-bit words written from outside: nothing is masked on either side"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(1240)
    planes = [rng.integers(0, 1 << 16, (H_ >> s, W >> s), dtype=np.uint16) for s in (0, 1, 1)]
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    SUP.write_picture(L, ctx, 0, planes)
    for win in WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps in (2, 1):
            ref = reference("random", rng, part, 10, bps)
            for name, given in [f for f in SUP.forms(ref) if (f[0] == "8-bit") == (bps == 1)]:
                same(queued(L, ctx, 0, win, given), compare_ref.compare(part, ref), win, 10, "16-bit words in the slot, window %r, %s" % (win, name))
    L.vvr_destroy(ctx)


def test_the_three_homes_of_a_reference():
    """pageable memory (overwritten right after vvr_compare_submit: the result is that of the planes as they were), memory of vvr_host_alloc (no
    staging copy), memory of vvr_device_alloc and a registered range (read in place: nothing is copied to the device)"""
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1250)
    rng = np.random.default_rng(1251)

    def h2d():
        n, b = C.c_size_t(), C.c_size_t()
        L.vvt_take_h2d(C.byref(n), C.byref(b))
        return n.value, b.value

    for win in WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps in (2, 1):
            ref = reference("random", rng, part, 10, bps)
            want = compare_ref.compare(part, ref)
            dt = np.uint16 if bps == 2 else np.uint8
            what = "window %r, %d bytes per sample" % (win, bps)
            # pageable: one copy through the entry's staging; the caller's planes are free at once
            given = [SUP.padded(p, dt, 3) for p in ref]
            h2d()
            t, keep = submit(L, ctx, 0, win, given)
            assert t >= 2 and h2d()[0] == 1
            for g in given:
                g.base[...] = 0x33
            same(collect(L, ctx, t, keep), want, win, 10, "pageable, " + what)
            del given
            # in another place: vvr_host_alloc, vvr_device_alloc, a registered range
            keepalive = []

            def pinned(n):
                return L.vvr_host_alloc(ctx, n)

            def device(n):
                return L.vvr_device_alloc(ctx, n)

            def registered(n):
                buf = np.zeros(n + 64, np.uint8)
                keepalive.append(buf)
                assert L.vvr_device_register(ctx, buf.ctypes.data, buf.nbytes) == abi.VVR_OK
                return buf.ctypes.data

            for home, alloc in (("vvr_host_alloc", pinned), ("vvr_device_alloc", device), ("a registered range", registered)):
                given, bases = [], []
                for c, p in enumerate(ref):
                    stride = p.shape[1] + (3, 5, 7)[c]      # (with one byte per sample: an odd stride for an even row and the other way round)
                    base = alloc(p.shape[0] * stride * bps)
                    assert base
                    bases.append(base)
                    a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                    a[...] = 0x44
                    a[:, :p.shape[1]] = p
                    given.append(a[:, :p.shape[1]])
                h2d()
                t, keep = submit(L, ctx, 0, win, given)
                assert t >= 2, L.vvr_last_error(ctx)
                assert h2d()[0] == 0, "a reference in pinned or device memory is not staged"
                same(collect(L, ctx, t, keep), want, win, 10, "%s, %s" % (home, what))
                if home == "a registered range":
                    # device planes mixed with host planes; a plane partly inside a range
                    mixed = [given[0], given[1].copy(), given[2]]
                    t, _ = submit(L, ctx, 0, win, mixed)
                    assert t == abi.VVR_ERR_PARAMETER and b"mixed" in L.vvr_last_error(ctx) and b"vvr_compare_submit" in L.vvr_last_error(ctx)
                    assert L.vvr_device_unregister(ctx, bases[0]) == abi.VVR_OK
                    assert L.vvr_device_register(ctx, bases[0], 1) == abi.VVR_OK      # (the smallest luma plane has two rows)
                    t, _ = submit(L, ctx, 0, win, given)
                    assert t == abi.VVR_ERR_PARAMETER and b"partly inside" in L.vvr_last_error(ctx) and b"vvr_compare_submit" in L.vvr_last_error(ctx)
                    for b_ in bases:
                        assert L.vvr_device_unregister(ctx, b_) == abi.VVR_OK
                elif home == "vvr_device_alloc":
                    for b_ in bases:
                        L.vvr_device_free(ctx, b_)
    # the ring is untouched by the refusals: eight requests fit
    part = compare_ref.window_planes(planes, WINDOWS[0])
    flight = [submit(L, ctx, 0, WINDOWS[0], [np.ascontiguousarray(p) for p in part]) for _ in range(8)]
    assert all(t >= 2 for t, _ in flight)
    for t, keep in flight:
        same(collect(L, ctx, t, keep), compare_ref.compare(part, part), WINDOWS[0], 10, "behind the refusals")
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1260)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    SUP.tickets_and_the_ring("compare", L, ctx, planes, 10, ext)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernels():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1261)
    SUP.statistics("compare", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_leave_the_ring_alone():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1262)
    SUP.write_picture(L, ctx, 1, planes)
    win = (8, 4, 200, 64)
    part = [np.ascontiguousarray(p) for p in compare_ref.window_planes(planes, win)]
    keep = abi.FrameCompare()

    refused = SUP.refuser(L, ctx, "compare", lambda ref=part, w_=win: abi.compare_request(0, None, w_, ref, keep))

    refused(b"struct_size", struct_size=C.sizeof(abi.CompareRequest) - 8)
    refused(b"no such slot", slot=7)
    refused(b"no such slot", slot=-1)
    refused(b"no such ref_slot", ref=5)
    refused(b"no such ref_slot", ref_slot=-2)
    refused(b"the slot itself", ref=0)
    refused(b"job must be", job=-2)
    refused(b"result is NULL", result=None)
    for x, y, w, h in [(W - 100, 0, 200, 64), (0, H_ - 2, 8, 4), (-2, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, 8, -2), (1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)]:
        refused(b"outside the picture, empty, or odd", ref=1, w_=(x, y, w, h))
    refused(b"ref_bytes_per_sample", ref_bytes_per_sample=0)
    refused(b"ref_bytes_per_sample", ref_bytes_per_sample=4)
    for k in range(3):
        refused(b"missing reference plane or stride", **{"plane%d" % k: None})
        refused(b"missing reference plane or stride", **{"stride%d" % k: part[k].shape[1] * 2 - 1})
    # pictures of different sizes in the two slots
    assert L.vvr_slot_picture_size(ctx, 1, W - 8, H_) == abi.VVR_OK
    refused(b"different sizes", ref=1)
    assert L.vvr_slot_picture_size(ctx, 1, W, H_) == abi.VVR_OK
    # a 4:0:0 context: odd windows are fine, planes 1 and 2 are not looked at
    ctx400, p400 = SUP.ctx_with(L, picture_size(0), 8, 0, 1263)
    refused(b"outside the picture", c=ctx400, ref=[p400[0]], w_=(0, 0, W400 + 1, 4))
    L.vvr_destroy(ctx400)
    assert L.vvr_compare_submit(None, None) == abi.VVR_ERR_PARAMETER and L.vvr_compare_submit(ctx, None) == abi.VVR_ERR_PARAMETER
    # the ring is untouched: eight requests still fit
    want = compare_ref.compare(part, part)
    SUP.eight_still_fit(L, ctx, lambda n: submit(L, ctx, 0, win, part if n % 2 else 1), lambda t, got: same(collect(L, ctx, t, got), want, win, 10, "behind the refusals"))
    L.vvr_destroy(ctx)


def test_not_ready_while_the_picture_is_with_its_worker():
    """the host stage of a B picture is held on its worker thread (and the stand-in is slowed down): a request without `blocking` comes back
    VVR_NOT_READY and takes no ring entry - for its job, and with ref_slot for any picture still with the workers; with `blocking` it is accepted
    and delivers the comparison of the pictures"""
    L = SUP.stub_lib()
    ctx, plans, descs, win = SUP.small_stream(L)
    pics = [d.c() for d in descs[:2]]
    j0 = L.vvr_submit(ctx, C.byref(pics[0]))
    assert j0 >= 0
    L.vvt_slow_b_pictures(300000)
    L.vvt_set_delay(1000)
    s0, s1 = plans[0].slot, plans[1].slot
    ref = [np.zeros((win[3] >> s, win[2] >> s), np.uint16) for s in (0, 1, 1)]
    try:
        j1 = L.vvr_submit(ctx, C.byref(pics[1]))
        assert j1 >= 0
        t, _ = submit(L, ctx, s1, win, ref, job=j1, blocking=False)
        assert t == abi.VVR_NOT_READY, (t, L.vvr_last_error(ctx))
        t, _ = submit(L, ctx, s1, win, ref, blocking=False)       # job -1: pictures are still with the workers
        assert t == abi.VVR_NOT_READY
        t, _ = submit(L, ctx, s0, win, s1, job=j0, blocking=False)      # its own job has been handed over, but who uses ref_slot is not known yet
        assert t == abi.VVR_NOT_READY
        flight = [submit(L, ctx, s1, win, ref if n % 2 else s0, job=j1) for n in range(8)]       # (no entry was lost to the attempts above)
    finally:
        L.vvt_slow_b_pictures(0)
        L.vvt_set_delay(0)
    assert all(t >= 2 for t, _ in flight), [t for t, _ in flight]
    got = [collect(L, ctx, t, keep) for t, keep in flight]
    assert L.vvr_wait(ctx, j1) == abi.VVR_OK
    p0, p1 = Q.sync_read(L, ctx, s0, win, 2, 3), Q.sync_read(L, ctx, s1, win, 2, 3)
    for n, g in enumerate(got):
        same(g, compare_ref.compare(p1, ref if n % 2 else p0), win, 10, "the B picture, request %d" % n)
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("compare", SUP.stub_lib())


def zeros_or_slot(win, ref_slot):
    """the reference of a request on a picture of a stream: planes of zeros, or the slot"""
    return [np.zeros((win[3] >> s, win[2] >> s), np.uint16) for s in (0, 1, 1)] if ref_slot is None else ref_slot


def delivered(keep):
    assert keep[0].samples[0] == 256 * 128


SUP.register("compare", b"vvr_compare_submit", ring_request, stats=stats_case, ref_slot=ref_slot_case, cases=windows,
             failing=lambda L, ctx, slot, win, job, ref_slot: submit(L, ctx, slot, win, zeros_or_slot(win, ref_slot), job=job),
             untouched=lambda keep: bytes(keep[0]) == bytes([SUP.FILL]) * C.sizeof(abi.FrameCompare) and (keep[1] == 0xaaaaaaaa).all(), delivered=delivered)


def test_later_pictures_into_either_slot_wait_for_the_request():
    """stream and event operations as the stand-in runtime records them: the output stream waits for the picture's completion event; the
    request's own event is recorded behind its first kernel; an I picture that later overwrites `slot`, and one that overwrites `ref_slot`, each
    wait for exactly that event on their lane"""
    from dataclasses import replace
    L = SUP.stub_lib()
    ctx, plans, descs, win = SUP.small_stream(L)
    Wd, Hd = win[2], win[3]
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    s0 = plans[0].slot
    s1 = next(pl.slot for pl in plans if pl.slot != s0)
    p0 = descs[0].c()
    j0 = L.vvr_submit(ctx, C.byref(p0))
    assert j0 >= 0 and L.vvr_stream_wait_job(ctx, j0, ext, 1) == abi.VVR_OK
    for target in (s0, s1):
        Q._trace(L)
        L.vvt_events_pending(1)                     # (nothing the device was given has finished: events that are complete would be dropped, not waited for)
        t, keep = submit(L, ctx, s0, win, s1)
        assert t >= 2 and L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY
        ops = Q._trace(L)
        waits, records = [(s, e) for op, s, e in ops if op == 0], [(s, e) for op, s, e in ops if op == 1]
        out_stream = records[-1][0]
        assert any(s == out_stream for s, _ in waits), "the output stream did not wait for the event of the picture in the slot"
        mine = [e for s, e in records if s == out_stream]
        read_event = mine[0]                        # the first record of the request: behind its first kernel, before the fold and the copy
        assert len(mine) == 2 and mine[1] != read_event
        again = synth.picture_for_plan(replace(plans[0], slot=target), Wd, Hd, seed=612 + target, tool_flags=T.TOOLS)      # an I picture: no references
        pa = again.c()
        j = L.vvr_submit(ctx, C.byref(pa))
        assert j >= 0 and L.vvr_stream_wait_job(ctx, j, ext, 1) == abi.VVR_OK      # (handed to the device)
        ops = Q._trace(L)
        assert any(op == 0 and e == read_event and s != out_stream for op, s, e in ops), "the picture that overwrites slot %d did not wait for the request's event" % target
        L.vvt_events_pending(0)
        collect(L, ctx, t, keep)
    assert L.vvr_sync(ctx) == abi.VVR_OK
    L.vvr_destroy(ctx)


HAND = [("luma only differs", 10, 3, [100, 25, 25], [7, 0, 0]),
        ("every component", 8, 3, [8294400, 2073600, 2073600], [123456789, 1234567, 7654321]),
        ("sums above 2^53", 10, 3, [1 << 26, 1 << 24, 1 << 24], [(1 << 26) * 4294836225, (1 << 24) * 4294836225, 3]),
        ("nothing differs", 9, 3, [64, 16, 16], [0, 0, 0]),
        ("4:0:0", 8, 1, [1088, 0, 0], [99, 0, 0])]


@pytest.mark.parametrize("what,bd,nc,samples,sse", HAND)
def test_psnr_on_sums_built_by_hand(what, bd, nc, samples, sse):
    L = SUP.stub_lib()
    raw = abi.FrameCompare()
    raw.struct_size, raw.bit_depth, raw.num_components = C.sizeof(abi.FrameCompare), bd, nc
    for c in range(3):
        raw.samples[c], raw.sse[c] = samples[c], sse[c]
    want = dict(num_components=nc, samples=samples, sse=sse)
    check_psnr(L, raw, want, bd, what)
    rc, got = c_psnr(L, raw, 0.)
    if what == "nothing differs":
        assert got == [float("inf")] * 4
    if what == "luma only differs":
        assert got[1] == got[2] == float("inf") and got[0] < got[3] < float("inf")
    if what == "4:0:0":
        assert got[1] == got[2] == 0. and got[0] == got[3]
        assert abs(got[0] - 10 * np.log10(255. * 255. * 1088 / 99)) < 1e-9


def test_psnr_of_a_request_and_its_refusals():
    L = SUP.stub_lib()
    ctx, planes = SUP.ctx_with(L, picture_size(1), 10, 1, 1270)
    win = WINDOWS[0]
    part = compare_ref.window_planes(planes, win)
    ref = reference("random", np.random.default_rng(1271), part, 10)
    want = compare_ref.compare(part, ref)
    raw, _ = queued(L, ctx, 0, win, SUP.forms(ref)[0][1])
    check_psnr(L, raw, want, 10, "a request")
    L.vvr_destroy(ctx)
    untouched = [-1.] * 4
    assert c_psnr(L, None, 0.) == (abi.VVR_ERR_PARAMETER, untouched)
    assert L.vvr_compare_psnr(C.byref(raw), 0., None) == abi.VVR_ERR_PARAMETER
    for field, value in (("struct_size", C.sizeof(abi.FrameCompare) - 8), ("bit_depth", 7), ("bit_depth", 12)):
        bad = abi.FrameCompare.from_buffer_copy(bytes(raw))
        setattr(bad, field, value)
        assert c_psnr(L, bad, 0.) == (abi.VVR_ERR_PARAMETER, untouched)
    bad = abi.FrameCompare.from_buffer_copy(bytes(raw))
    bad.samples[0] = 0
    assert c_psnr(L, bad, 0.) == (abi.VVR_ERR_PARAMETER, untouched)


def test_python_mirror_and_symbols():
    import vvdec_amd
    assert "vvr_compare_submit" in vvdec_amd.EXPORTED_SYMBOLS and "vvr_compare_psnr" in vvdec_amd.EXPORTED_SYMBOLS
    assert all(hasattr(vvdec_amd.Reconstructor, f) for f in ("compare", "psnr"))
    assert abi.compare_map_shape((0, 0, 208, 80)) == (2, 4) and abi.compare_map_shape((2, 2, 70, 34)) == (1, 2) and abi.compare_map_shape((0, 0, 64, 64)) == (1, 1)
