"""CPU: the semi-planar formats of the output queue (VVR_OUT_NV12, VVR_OUT_P010) and destinations in device memory (vvr_device_alloc,
vvr_device_register, vvr_output_stream_wait) on the stand-in runtime of tests/hoststub, where any buffer serves as device memory and the
launchers of the output stage are plain loops (vvr_output.inc, host only).  The expected bytes never come from the code under test alone: for
plain windows they are the picture the test wrote, cropped, interleaved and shifted in numpy; with grain or a size they are the same numpy
rearrangement of the planar16 request's planes, which their own tests pin to vvdec::FilmGrain and vvdec::rescalePlane.  The helpers take a
library and a context, so tests/test_gpu_output_semiplanar.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import test_film_grain_host as H
import test_host_glue as T
import test_output_queue_host as Q
from vvdec_amd import abi, stream, synth

pytestmark = T.pytestmark
FILL = SUP.FILL
W, H_ = 448, 160
# (2, 6, 202, 38): chroma rows of 101 samples - odd, rows that straddle a lane's piece, a chroma origin at an odd sample
WINDOWS = [(0, 0, 448, 160), (8, 4, 200, 64), (2, 6, 202, 38), (6, 2, 144, 34)]
SIZES = [None, (300, 96), (134, 26)]
VARIANTS = [(10, "p010"), (8, "p010"), (9, "p010"), (8, "nv12")]


def cases(bd):
    """(window, size, grain): every window plain and at both sizes; with grain (bit depths 8 and 10; all four windows are wider than 128), alone
    and with each size"""
    out = [(win, size, False) for win in WINDOWS for size in SIZES]
    if bd != 9:
        out += [(win, size, True) for win in WINDOWS for size in SIZES]
    return out


def semi(planes, fmt, bd):
    """three planes of samples -> the two planes of nv12 / p010: luma; Cb0, Cr0, Cb1, Cr1, ...; p010 shifts into the high bits"""
    y, cb, cr = [np.asarray(p).astype(np.uint16) for p in planes]
    cbcr = np.empty((cb.shape[0], 2 * cb.shape[1]), np.uint16)
    cbcr[:, 0::2], cbcr[:, 1::2] = cb, cr
    if fmt == "nv12":
        return [y.astype(np.uint8), cbcr.astype(np.uint8)]
    return [(y << (16 - bd)).astype(np.uint16), (cbcr << (16 - bd)).astype(np.uint16)]


def crop(picture, win):
    x, y, w, h = win
    return [p[y >> s:(y + h) >> s, x >> s:(x + w) >> s] for p, s in zip(picture, (0, 1, 1))]


def expected(L, ctx, picture, slot, win, size, grain, seed, fmt, bd):
    """plain windows: from the picture that was written; else from the planar16 request of the same window, size, grain and seed"""
    if size is None and not grain:
        return semi(crop(picture, win), fmt, bd)
    assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    return semi(Q.queued(L, ctx, slot, win, "planar16", 3, size=size, grain=grain), fmt, bd)


STRIDES = ("row", "row+6", "256")


def layout(shapes, dt, stride_kind):
    """per plane (rows, row bytes, stride bytes, bytes from the first to behind the last sample)"""
    item = np.dtype(dt).itemsize
    out = []
    for r, n in shapes:
        row = n * item
        stride = row if stride_kind == "row" else row + 6 if stride_kind == "row+6" else -(-row // 256) * 256
        out.append((r, row, stride, (r - 1) * stride + row))
    return out


class DevicePlanes:
    """destination planes in 'device memory' of the stand-in runtime: numpy buffers, each plane's extent registered with the context"""

    def __init__(self, L, ctx, win, fmt, size, ncomp, stride_kind="row", mis=0, register=True):
        self.L, self.ctx = L, ctx
        shapes, self.dt = abi.output_plane_shapes(win, fmt, size, ncomp)
        self.raw, self.off, self.views, self.geo, self.registered = [], [], [], layout(shapes, self.dt, stride_kind), []
        item = np.dtype(self.dt).itemsize
        for (r, n), (_, row, stride, extent) in zip(shapes, self.geo):
            raw = np.full(extent + 256, FILL, np.uint8)
            off = (-raw.ctypes.data) % 64 + 64 + mis
            self.raw.append(raw)
            self.off.append(off)
            self.views.append(np.ndarray((r, n), self.dt, buffer=raw, offset=off, strides=(stride, item)))
            if register:
                assert L.vvr_device_register(ctx, raw.ctypes.data + off, extent) == abi.VVR_OK, L.vvr_last_error(ctx)
                self.registered.append(raw.ctypes.data + off)

    def unregister(self):
        for p in self.registered:
            assert self.L.vvr_device_unregister(self.ctx, p) == abi.VVR_OK, self.L.vvr_last_error(self.ctx)
        self.registered = []

    def check(self, want, what):
        check_planes(self.raw, self.off, self.geo, want, what)


def check_planes(raws, offs, geo, want, what):
    """the rows hold `want`, and not a byte around a row or a plane has changed (raws: the buffers as uint8 arrays, filled with FILL beforehand)"""
    for k, (raw, off, (r, row, stride, extent)) in enumerate(zip(raws, offs, geo)):
        exp = np.full(raw.shape, FILL, np.uint8)
        w_ = np.ascontiguousarray(want[k]).view(np.uint8).reshape(r, row)
        for j in range(r):
            exp[off + j * stride:off + j * stride + row] = w_[j]
        if not np.array_equal(raw, exp):
            inside = np.zeros(raw.shape, bool)
            for j in range(r):
                inside[off + j * stride:off + j * stride + row] = True
            bad = raw != exp
            assert False, "%s plane %d: %d bytes of the rows differ, %d bytes outside the rows changed" % (what, k, int((bad & inside).sum()), int((bad & ~inside).sum()))


def submit_device(L, ctx, slot, win, fmt, ncomp, size=None, grain=False, job=None, stride_kind="row", mis=0, col=(True, False)):
    d = DevicePlanes(L, ctx, win, fmt, size, ncomp, stride_kind, mis)
    req = abi.output_request(slot, job, win, fmt, size, col, grain, True, d.views)
    return L.vvr_output_submit(ctx, C.byref(req)), d


def device_request(L, ctx, slot, win, fmt, ncomp, want, what, seed=None, **kw):
    if seed is not None:
        assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
    t, d = submit_device(L, ctx, slot, win, fmt, ncomp, **kw)
    assert t >= 0, (what, t, L.vvr_last_error(ctx))
    assert L.vvr_output_wait(ctx, t) == abi.VVR_OK, L.vvr_last_error(ctx)
    d.check(want, what)
    d.unregister()


def check_matrix(L, ctx, picture, bd, fmt, device=device_request):
    """every case into pageable destinations with padded rows, into memory of vvr_host_alloc and into device memory at every stride and base
    (device: one request into device memory, checked - here a registered range of the stand-in runtime)"""
    for n, (win, size, grain) in enumerate(cases(bd)):
        what = "%s at %d bits, window %r size %r grain %r" % (fmt, bd, win, size, grain)
        seed = 3000 + n
        want = expected(L, ctx, picture, 0, win, size, grain, seed, fmt, bd)
        for alloc in (None, lambda nb: L.vvr_host_alloc(ctx, nb)):
            assert L.vvr_set_film_grain_seed(ctx, seed) == abi.VVR_OK
            got = Q.queued(L, ctx, 0, win, fmt, 3, size=size, grain=grain, alloc=alloc)      # (checks the padding of every row)
            assert len(got) == 2
            for k in range(2):
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s, %s, plane %d: %d samples differ" % (what, "pinned" if alloc else "pageable", k, int((got[k] != want[k]).sum()))
        for stride_kind in STRIDES:
            for mis in (0, 2):
                device(L, ctx, 0, win, fmt, 3, want, "%s, device, stride %s, base + %d" % (what, stride_kind, mis), seed=seed, size=size, grain=grain, stride_kind=stride_kind, mis=mis)


def setup(L, mk_ctx, write, rng, bd):
    ctx = mk_ctx(W, H_)
    picture = film_grain_ref.grain_picture(rng, W, H_, bd, 1)
    write(ctx, 0, picture)
    bank = abi.film_grain_bank(**H._bank(rng))
    if bd != 9:
        assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    return ctx, picture, bank


@pytest.mark.parametrize("bd,fmt", VARIANTS)
def test_semiplanar_matrix(bd, fmt):
    L = SUP.stub_lib()
    ctx, picture, bank = setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(40 + bd), bd)
    check_matrix(L, ctx, picture, bd, fmt)
    L.vvr_destroy(ctx)


def test_device_requests_copy_nothing_in_wait():
    """the stand-in's kernels and copies run inside vvr_output_submit: the rows are in place when it returns, and what the test writes over them
    afterwards survives vvr_output_wait; memory of vvr_device_alloc serves like a registered range"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(51)
    ctx, picture, bank = setup(L, lambda w, h: SUP.make_ctx(L, w, h, 10, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, 10)
    win = (2, 6, 202, 38)
    want = semi(crop(picture, win), "p010", 10)
    for stride_kind in STRIDES:
        t, d = submit_device(L, ctx, 0, win, "p010", 3, stride_kind=stride_kind)
        assert t >= 0, L.vvr_last_error(ctx)
        d.check(want, "before vvr_output_wait, stride " + stride_kind)
        for raw in d.raw:
            raw[...] = 0x55
        assert L.vvr_output_wait(ctx, t) == abi.VVR_OK
        assert all((raw == 0x55).all() for raw in d.raw), "vvr_output_wait wrote into a device destination"
        d.unregister()
    # memory of the context: both planes in one allocation
    shapes, dt = abi.output_plane_shapes(win, "p010", None, 3)
    nbytes = [r * n * 2 for r, n in shapes]
    base = L.vvr_device_alloc(ctx, 256 + sum(nbytes) + 256)
    assert base
    mem = np.frombuffer((C.c_char * (256 + sum(nbytes) + 256)).from_address(base), np.uint8)
    mem[...] = FILL
    outs = [np.ndarray(shapes[0], dt, buffer=mem, offset=256), np.ndarray(shapes[1], dt, buffer=mem, offset=256 + nbytes[0])]
    req = abi.output_request(0, None, win, "p010", None, (True, False), False, True, outs)
    t = L.vvr_output_submit(ctx, C.byref(req))
    assert t >= 0, L.vvr_last_error(ctx)
    assert L.vvr_output_wait(ctx, t) == abi.VVR_OK
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1])
    assert (mem[:256] == FILL).all() and (mem[256 + sum(nbytes):] == FILL).all()
    L.vvr_device_free(ctx, base)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_existing_formats_into_device_memory(bd):
    """planar16, planar8 and packed10 into registered ranges: the bytes of the same requests into pageable memory"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(52 + bd)
    ctx, picture, bank = setup(L, lambda w, h: SUP.make_ctx(L, w, h, bd, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, bd)
    n = 0
    for fmt in ["planar16", "packed10"] + (["planar8"] if bd == 8 else []):
        for win in [(0, 0, 448, 160), (8, 4, 200, 64)] + ([(2, 6, 202, 38)] if fmt != "packed10" else []):
            for size, grain in [(None, False), ((296, 96), False), (None, True), ((296, 96), True)]:
                for stride_kind, mis in (("row", 0), ("row+6", 2), ("256", 0), ("row", 2)):
                    n += 1
                    assert L.vvr_set_film_grain_seed(ctx, 4000 + n) == abi.VVR_OK
                    want = Q.queued(L, ctx, 0, win, fmt, 3, size=size, grain=grain)
                    device_request(L, ctx, 0, win, fmt, 3, want, "%s %r %r grain %r stride %s base + %d" % (fmt, win, size, grain, stride_kind, mis), seed=4000 + n, size=size, grain=grain, stride_kind=stride_kind, mis=mis)
    L.vvr_destroy(ctx)


def test_refusals_of_formats_and_ranges():
    L = SUP.stub_lib()
    rng = np.random.default_rng(53)
    ctx = SUP.make_ctx(L, W, H_, 10, 1)
    SUP.write_picture(L, ctx, 0, film_grain_ref.grain_picture(rng, W, H_, 10, 1))
    win = (8, 4, 200, 64)

    def refused(text, c=ctx, fmt="p010", mutate=None, ncomp=3, outs=None):
        shapes, dt = abi.output_plane_shapes(win, fmt, None, ncomp)
        outs = outs or [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(0, None, win, fmt, None, (True, False), False, True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c), (text, rc, L.vvr_last_error(c))

    refused(b"8-bit output of a stream with more than 8 bits per sample", fmt="nv12")          # (VVR_OUT_PLANAR8's wording)
    ctx400 = SUP.make_ctx(L, W, H_, 8, 0)
    for fmt in ("nv12", "p010"):
        refused(b"no chroma to interleave", c=ctx400, fmt=fmt)
    L.vvr_destroy(ctx400)
    refused(b"stride below the output's row", mutate=lambda r: r.dst_stride_bytes.__setitem__(1, 2 * 200 - 2))      # (the interleaved row: 2 * 100 samples of 2 bytes)
    refused(b"missing plane", mutate=lambda r: r.dst.__setitem__(1, None))
    for f in (3, 4, 15, 18, 255):
        refused(b"unknown format", mutate=lambda r, f=f: setattr(r, "format", f))
    # dst[2] and its stride are ignored
    shapes, dt = abi.output_plane_shapes(win, "p010", None, 3)
    outs = [np.zeros(s, dt) for s in shapes]
    req = abi.output_request(0, None, win, "p010", None, (True, False), False, True, outs)
    req.dst[2], req.dst_stride_bytes[2] = None, 0
    t = L.vvr_output_submit(ctx, C.byref(req))
    assert t >= 0 and L.vvr_output_wait(ctx, t) == abi.VVR_OK
    # ranges
    d = DevicePlanes(L, ctx, win, "p010", None, 3)
    base, extent = d.registered[0], d.geo[0][3]
    for p, n in ((base, extent), (base + 16, 32), (base - 8, 16), (base + extent - 2, 64), (base - 64, extent + 128)):
        assert L.vvr_device_register(ctx, p, n) == abi.VVR_ERR_PARAMETER and b"overlaps" in L.vvr_last_error(ctx)
    assert L.vvr_device_register(ctx, None, 64) == abi.VVR_ERR_PARAMETER and L.vvr_device_register(ctx, base + extent, 0) == abi.VVR_ERR_PARAMETER
    other = np.zeros(4096, np.uint8)
    assert L.vvr_device_unregister(ctx, other.ctypes.data) == abi.VVR_ERR_PARAMETER and b"unknown pointer" in L.vvr_last_error(ctx)
    assert L.vvr_device_unregister(ctx, base + 2) == abi.VVR_ERR_PARAMETER and b"unknown pointer" in L.vvr_last_error(ctx)
    L.vvr_device_free(ctx, other.ctypes.data)
    assert b"vvr_device_free: unknown pointer" in L.vvr_last_error(ctx)
    L.vvr_device_free(ctx, base)                                     # (the caller's memory: not freed, not forgotten)
    assert b"vvr_device_free: registered memory" in L.vvr_last_error(ctx)
    own = L.vvr_device_alloc(ctx, 4096)
    assert own and L.vvr_device_unregister(ctx, own) == abi.VVR_ERR_PARAMETER and b"vvr_device_free" in L.vvr_last_error(ctx)
    L.vvr_device_free(ctx, own)
    assert L.vvr_device_unregister(ctx, own) == abi.VVR_ERR_PARAMETER and b"unknown pointer" in L.vvr_last_error(ctx)
    # a plane half inside a range: the luma plane's range is cut short / starts late
    d.unregister()
    half = DevicePlanes(L, ctx, win, "p010", None, 3, register=False)
    b0, e0, b1, e1 = half.raw[0].ctypes.data + half.off[0], half.geo[0][3], half.raw[1].ctypes.data + half.off[1], half.geo[1][3]
    assert L.vvr_device_register(ctx, b1, e1) == abi.VVR_OK
    for p, n in ((b0, e0 // 2), (b0 + 64, e0 - 64), (b0 + 64, 64)):
        assert L.vvr_device_register(ctx, p, n) == abi.VVR_OK
        refused(b"partly inside a device range", outs=half.views)
        assert L.vvr_device_unregister(ctx, p) == abi.VVR_OK
    # device and pageable planes mixed (plane 1 registered, plane 0 not), and the other way round
    refused(b"mixed with planes in host memory", outs=half.views)
    assert L.vvr_device_unregister(ctx, b1) == abi.VVR_OK and L.vvr_device_register(ctx, b0, e0) == abi.VVR_OK
    refused(b"mixed with planes in host memory", outs=half.views)
    pinned = [np.frombuffer((C.c_char * (a.size * 2)).from_address(L.vvr_host_alloc(ctx, a.size * 2)), np.uint16).reshape(a.shape) for a in half.views]
    refused(b"mixed with planes in host memory", outs=[half.views[0], pinned[1]])
    # in flight: the range cannot be unregistered until the ticket is retired
    assert L.vvr_device_register(ctx, b1, e1) == abi.VVR_OK
    req = abi.output_request(0, None, win, "p010", None, (True, False), False, True, half.views)
    t = L.vvr_output_submit(ctx, C.byref(req))
    assert t >= 0, L.vvr_last_error(ctx)
    for p in (b0, b1):
        assert L.vvr_device_unregister(ctx, p) == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    assert L.vvr_output_wait(ctx, t) == abi.VVR_OK
    assert L.vvr_device_unregister(ctx, b0) == abi.VVR_OK and L.vvr_device_unregister(ctx, b1) == abi.VVR_OK
    # tickets of vvr_output_stream_wait
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    assert L.vvr_output_stream_wait(ctx, t, ext) == abi.VVR_ERR_PARAMETER and b"unknown or retired ticket" in L.vvr_last_error(ctx)      # retired
    assert L.vvr_output_stream_wait(ctx, 12345, ext) == abi.VVR_ERR_PARAMETER and L.vvr_output_stream_wait(ctx, -1, ext) == abi.VVR_ERR_PARAMETER
    L.vvr_destroy(ctx)


def test_stream_wait_is_one_wait_for_the_completion_event():
    """the stand-in's trace: vvr_output_stream_wait puts exactly one wait, for the event the request recorded last on the output stream (behind
    its last kernel or copy), on the caller's stream and nothing else; the request is still not complete for the host afterwards (nothing
    waited for it) and the ticket stays.  Device and host destinations alike.  Eight device requests in flight, the ninth is VVR_ERR_BUSY."""
    L = SUP.stub_lib()
    rng = np.random.default_rng(54)
    ctx, picture, bank = setup(L, lambda w, h: SUP.make_ctx(L, w, h, 10, 1), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), rng, 10)
    win = (2, 6, 202, 38)
    want = semi(crop(picture, win), "p010", 10)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    for device in (True, False):
        Q._trace(L)
        L.vvt_events_pending(1)
        if device:
            t, d = submit_device(L, ctx, 0, win, "p010", 3, stride_kind="row+6")
        else:
            t, outs = Q.submit(L, ctx, 0, win, "p010", 3)
        assert t >= 0, L.vvr_last_error(ctx)
        records = [(s, e) for op, s, e in Q._trace(L) if op == 1]
        out_stream, done = records[-1]
        assert len(records) >= 2 and all(s == out_stream for s, _ in records)
        assert L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY
        assert L.vvr_output_stream_wait(ctx, t, ext) == abi.VVR_OK
        ops = Q._trace(L)
        assert len(ops) == 1 and ops[0][0] == 0 and ops[0][2] == done and ops[0][1] != out_stream, ops
        assert L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY      # (the host has waited for nothing; the ticket stays)
        assert L.vvr_output_stream_wait(ctx, t, ext) == abi.VVR_OK and Q._trace(L) == ops
        L.vvt_events_pending(0)
        if device:
            assert L.vvr_output_wait(ctx, t) == abi.VVR_OK
            d.check(want, "device")
            d.unregister()
        else:
            got = Q.collect(L, ctx, t, outs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the ring
    assert L.vvr_set_film_grain_seed(ctx, 78) == abi.VVR_OK
    wins = [WINDOWS[n % 4] for n in range(8)]
    wants = [semi(Q.queued(L, ctx, 0, w_, "planar16", 3, grain=True), "p010", 10) for w_ in wins]
    assert L.vvr_set_film_grain_seed(ctx, 78) == abi.VVR_OK
    flight = [submit_device(L, ctx, 0, w_, "p010", 3, grain=True, stride_kind=STRIDES[n % 3], mis=2 * (n & 1)) for n, w_ in enumerate(wins)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    t9, d9 = submit_device(L, ctx, 0, win, "p010", 3, grain=True)
    assert t9 == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    d9.unregister()
    for n, (t, d) in enumerate(flight):
        assert L.vvr_output_wait(ctx, t) == abi.VVR_OK
        d.check(wants[n], "request %d of eight" % n)
        d.unregister()
    L.vvr_destroy(ctx)


def test_stream_wait_of_a_request_whose_job_failed():
    """a request submitted after its job is known to have failed: vvr_output_stream_wait gives the job's status and enqueues nothing"""
    L = SUP.stub_lib()
    Wd, Hd = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = SUP.stream_ctx(L, Wd, Hd, nslots)
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=611, tool_flags=T.TOOLS, p_intra=0.3) for pl in plans[:2]]
    pics = [d.c() for d in descs]
    j0 = L.vvr_submit(ctx, C.byref(pics[0]))
    L.vvt_fail_leaf_waits(1)
    j1 = L.vvr_submit(ctx, C.byref(pics[1]))
    assert L.vvr_wait(ctx, j0) == abi.VVR_OK and L.vvr_wait(ctx, j1) == abi.VVR_ERR_DEVICE
    L.vvt_fail_leaf_waits(0)
    t, d = submit_device(L, ctx, plans[1].slot, (0, 0, Wd, Hd), "p010", 3, job=j1)
    assert t >= 0, L.vvr_last_error(ctx)
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    Q._trace(L)
    assert L.vvr_output_stream_wait(ctx, t, ext) == abi.VVR_ERR_DEVICE and Q._trace(L) == []
    assert L.vvr_output_wait(ctx, t) == abi.VVR_ERR_DEVICE
    assert all((raw == FILL).all() for raw in d.raw)
    d.unregister()
    L.vvr_destroy(ctx)


def test_python_mirror_of_the_formats():
    assert abi.OUT_FORMATS["nv12"] == 16 and abi.OUT_FORMATS["p010"] == 17
    assert abi.output_plane_shapes((2, 6, 202, 38), "p010", None, 3) == ([(38, 202), (19, 202)], np.uint16)
    assert abi.output_plane_shapes((2, 6, 202, 38), "nv12", (134, 26), 3) == ([(26, 134), (13, 134)], np.uint8)
    assert abi.output_plane_shapes((0, 0, 448, 160), "p010", (302, 98), 3)[0] == [(98, 302), (49, 302)]
    assert abi.output_plane_shapes((0, 0, 6, 6), "nv12", (10, 6), 3)[0] == [(6, 10), (3, 10)]
