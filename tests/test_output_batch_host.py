"""CPU: many regions of one picture as a batch in one request (vvr_output_submit_batch) on the stand-in runtime of tests/hoststub, where the
launchers of the output stage are plain loops with the loop over the regions that is blockIdx.z on the device (vvr_output.inc, host only).

The definition the cases hold the call to: region i receives exactly the bytes vvr_output_submit stores for the same request with x, y =
origin[2 i], origin[2 i + 1] and dst[k] advanced by i * batch_stride_bytes[k]; no other byte of the destination changes.  Expected bytes never
come from the code under test: the crop of the written picture at the region's origin goes through tests/resample_ref.py (or, with no filter
set, through vvdec::rescalePlane of the drop-in library, tests/rescale_ref.py, as the tests of vvr_read_output_scaled take it) and then through
rgb_ref / interleaved_ref / colour_transform_ref / lut3d_ref.  Every comparison is of bytes, over the whole destination buffer with its guard
bytes.  The case functions take a library and a context, so tests/test_gpu_output_batch.py and tests/batch_on_the_device.py run them on the
device."""
import ctypes as C

import numpy as np
import pytest

import colour_transform_ref as X
import interleaved_ref
import lut3d_ref as U
import output_support as SUP
import resample_ref as R
import rescale_ref
import rgb_ref
import test_host_glue as T
import test_output_interleaved_host as I
import test_output_lut3d_host as LH
import test_output_queue_host as Q
import test_output_resample_host as N
import test_output_semiplanar_host as S
import test_output_transform_host as TH
from vvdec_amd import abi

pytestmark = T.pytestmark
need_ref = pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs /root/reference at build time)")
W, H_ = N.W, N.H_
FILL = SUP.FILL
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))      # the ImageNet normalisation
WHO = b"vvr_output_submit_batch: "
# the geometries of the issue's table: (window size, output size or None, origins)
STRAIGHT = ((48, 32), None, [(0, 0), (160, 48), (2, 2), (4, 2), (2, 2)])      # flush bottom-right; odd chroma origin; overlapping; a duplicate
SECOND = ((96, 48), (28, 12), [(0, 0), (112, 32), (2, 6), (50, 16)])          # non-integer ratio, chroma 48 x 24 -> 14 x 6, one launch per plane
WIDE = ((160, 64), (132, 40), [(0, 0), (48, 16), (24, 8)])                    # more than one tile across (RSM_TW = 64), the last one narrow
TWO_LAUNCH = ((64, 80), (16, 8), [(0, 0), (144, 0), (70, 0)])                 # h > 4 * out_h for luma and chroma: the two-launch form
DCTIF = ((64, 32), (96, 48), [(0, 0), (144, 48), (34, 10)])
LIMIT = ((16, 16), None, [(16 * (i % 13), 16 * (i // 13 % 5)) for i in range(256)])      # 65 places on a grid, wrapping with duplicates


def picture(bd, seed=0):
    return N.content("noise", W, H_, bd, 3, 600 + seed)


# ---- where the destinations live: .ptr, .read() -> the bytes as a uint8 array, .close()

class Pageable:
    name = "pageable"

    def __init__(self, L, ctx, nbytes):
        self.a = np.full(nbytes, FILL, np.uint8)
        self.ptr = self.a.ctypes.data

    def read(self):
        return self.a

    def close(self):
        pass


class Pinned(Pageable):
    name = "vvr_host_alloc"

    def __init__(self, L, ctx, nbytes):
        self.ptr = L.vvr_host_alloc(ctx, nbytes)
        assert self.ptr
        self.a = np.frombuffer((C.c_char * nbytes).from_address(self.ptr), np.uint8)
        self.a[...] = FILL


class Registered(Pageable):
    """'device memory' of the stand-in runtime: a numpy buffer registered with the context"""
    name = "device"

    def __init__(self, L, ctx, nbytes):
        Pageable.__init__(self, L, ctx, nbytes)
        self.L, self.ctx = L, ctx
        assert L.vvr_device_register(ctx, self.ptr, nbytes) == abi.VVR_OK, L.vvr_last_error(ctx)

    def close(self):
        assert self.L.vvr_device_unregister(self.ctx, self.ptr) == abi.VVR_OK, self.L.vvr_last_error(self.ctx)


HOMES = (Pageable, Pinned, Registered)


class Dest:
    """the destination of one batch inside one buffer of a home, 256 bytes of guard on both sides, the first plane at a multiple of 64 bytes
    + mis.  layout "packed": a contiguous ( N, planes, rows, row ) array - rows back to back, batch stride = the region's bytes; "padded": rows
    of row + 6 bytes, planes in areas of their own, batch stride = the plane's extent + batch_pad.  check(): every region's rows hold `want`
    and no other byte of the buffer has changed"""

    def __init__(self, L, ctx, n, wsize, fmt, size, home=Pageable, layout="packed", batch_pad=10, mis=0):
        shapes, dt = abi.output_plane_shapes((0, 0) + tuple(wsize), fmt, size, 3)
        item = np.dtype(dt).itemsize
        self.n, self.dt, self.shapes = n, dt, shapes
        self.rows = [r for r, _ in shapes]
        self.row = [m * item for _, m in shapes]
        if layout == "packed":
            self.stride = list(self.row)
            planes = [r * b for r, b in zip(self.rows, self.row)]
            self.poff = [sum(planes[:k]) for k in range(len(shapes))]
            self.bstride = [sum(planes)] * len(shapes)
            end = n * sum(planes)
        else:
            self.stride = [b + 6 for b in self.row]
            self.extent = [(r - 1) * s + b for r, s, b in zip(self.rows, self.stride, self.row)]
            self.bstride = [e + batch_pad for e in self.extent]
            self.poff, end = [], 0
            for k in range(len(shapes)):
                self.poff.append(end)
                end += (n - 1) * self.bstride[k] + self.extent[k] + 70
        self.mem = home(L, ctx, end + 1024)
        self.base = 256 + (-(self.mem.ptr + 256)) % 64 + mis
        self.end = end

    def request(self, slot, wsize, fmt, size, col, job=None, blocking=True, origins=()):
        r = abi.OutputRequest()
        r.struct_size, r.slot, r.job = C.sizeof(abi.OutputRequest), slot, -1 if job is None else job
        r.x, r.y, r.w, r.h = 0, 0, wsize[0], wsize[1]
        r.out_w, r.out_h = size or (0, 0)
        r.collocated = int(bool(col[0])) | int(bool(col[1])) << 1
        r.format, r.grain, r.blocking = abi.OUT_FORMATS[fmt], 0, 1 if blocking else 0
        for k in range(len(self.shapes)):
            r.dst[k], r.dst_stride_bytes[k] = self.mem.ptr + self.base + self.poff[k], self.stride[k]
        b, keep = abi.output_batch(origins, self.bstride)
        return r, b, keep

    def check(self, want, what):
        """want: per region the planes of the format"""
        got = self.mem.read()
        exp, inside = np.full(got.shape, FILL, np.uint8), np.zeros(got.shape, bool)
        assert len(want) == self.n, what
        for i, planes in enumerate(want):
            assert len(planes) == len(self.shapes), what
            for k, p in enumerate(planes):
                p = np.ascontiguousarray(p)
                assert p.dtype == np.dtype(self.dt) and p.shape == tuple(self.shapes[k]), (what, i, k, p.dtype, p.shape)
                b = p.view(np.uint8).reshape(self.rows[k], self.row[k])
                first = self.base + self.poff[k] + i * self.bstride[k]
                for j in range(self.rows[k]):
                    exp[first + j * self.stride[k]:first + j * self.stride[k] + self.row[k]] = b[j]
                    inside[first + j * self.stride[k]:first + j * self.stride[k] + self.row[k]] = True
        bad = got != exp
        if bad.any():
            at = int(np.flatnonzero(bad)[0]) - self.base
            assert False, "%s, %s: %d bytes of the regions differ, %d bytes outside them changed (first at byte %d of the destination)" % (
                what, self.mem.name, int((bad & inside).sum()), int((bad & ~inside).sum()), at)

    def untouched(self, what):
        assert (self.mem.read() == FILL).all(), what + ": the destination was written"

    def close(self):
        self.mem.close()


def submit(L, ctx, slot, origins, wsize, fmt, size=None, col=(True, False), job=None, blocking=True, **kw):
    """one vvr_output_submit_batch -> (ticket or error, the destination)"""
    d = Dest(L, ctx, len(origins), wsize, fmt, size, **kw)
    req, b, keep = d.request(slot, wsize, fmt, size, col, job, blocking, origins)
    return L.vvr_output_submit_batch(ctx, C.byref(req), C.byref(b)), d


def collect(L, ctx, t, d, want, what):
    rc = L.vvr_output_wait(ctx, t)
    assert rc == abi.VVR_OK, (what, rc, L.vvr_last_error(ctx))
    d.check(want, what)
    d.close()


def batch(L, ctx, slot, origins, wsize, fmt, want, what, **kw):
    t, d = submit(L, ctx, slot, origins, wsize, fmt, **kw)
    assert t >= 2, (what, t, L.vvr_last_error(ctx))
    collect(L, ctx, t, d, want, what)


# ---- expected bytes

def store(frame, bd, fmt, col, norm=None, transform=None, lut=None):
    """one 4:2:0 frame -> the planes of `fmt` as the existing host tests of the formats compute them"""
    if lut is not None:
        return U.frame(frame, bd, fmt, 1, False, col, lut[0], lut[1], transform, norm)
    if fmt in rgb_ref.DTYPES:
        return X.rgb(frame, bd, fmt, 1, False, col, transform) if transform is not None else rgb_ref.rgb(frame, bd, fmt, 1, False, col)
    return interleaved_ref.frame(frame, bd, fmt, 1, False, col, transform, norm)


def frames(pic, origins, wsize, filt=None, size=None, bd=10, col=(True, False), dctif=None):
    """the 4:2:0 frame of every region: the crop at its origin - the region's window is the plane - resampled by the restatement (dctif: a
    function ( list of crops ) -> list of frames for the context with no filter set)"""
    crops = [S.crop(pic, o + tuple(wsize)) for o in origins]
    if size is None or tuple(size) == tuple(wsize):
        return crops
    if filt:
        return [R.resample(c, filt, size, bd, col) for c in crops]
    return dctif(crops)


def expected(pic, origins, wsize, fmt, filt=None, size=None, bd=10, col=(True, False), norm=None, transform=None, lut=None, dctif=None):
    return [store(f, bd, fmt, col, norm, transform, lut) for f in frames(pic, origins, wsize, filt, size, bd, col, dctif)]


def rescale_plane_frames(backend, tmpdir, size, bd, col):
    """-> the `dctif` of frames(): vvdec::rescalePlane on its plain C++ path (tests/rescale_ref.py), one call for all crops"""
    def run(crops):
        cases = [(c[k], size[0] >> (1 if k else 0), size[1] >> (1 if k else 0), k, 1, bd, col[0], col[1]) for c in crops for k in range(3)]
        out = rescale_ref.rescale(cases, backend, False, tmpdir)
        return [out[3 * i:3 * i + 3] for i in range(len(crops))]
    return run


def setup_colour(L, ctx):
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    TH.set_transform(L, ctx, None)
    LH.set_lut(L, ctx, None)
    assert I.set_norm(L, ctx, None) == abi.VVR_OK
    N.set_filter(L, ctx, R.REFERENCE)


# ---- the cases

def check_straight(L, ctx, write, bd, home=Pageable):
    """no scaling: the source through the table of origins into k_output_rgb; rgb8, rgbf32 with the ImageNet normalisation, bgra8, and
    rgb10a2 at 10 bits"""
    wsize, _, origins = STRAIGHT
    pic = picture(bd, bd)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    assert I.set_norm(L, ctx, NORM) == abi.VVR_OK
    for fmt in ["rgb8", "rgbf32", "bgra8"] + (["rgb10a2"] if bd == 10 else []):
        want = expected(pic, origins, wsize, fmt, bd=bd, norm=NORM)
        batch(L, ctx, 0, origins, wsize, fmt, want, "no scaling, %s at %d bits" % (fmt, bd), home=home)
    assert I.set_norm(L, ctx, None) == abi.VVR_OK


def check_antialiased(L, ctx, write, bd, home=Pageable):
    """the second geometry under all three filters, rgb8 and rgbf16; all four chroma positions for the triangle filter"""
    wsize, size, origins = SECOND
    pic = picture(bd, 10 + bd)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    for filt in N.FILTERS:
        N.set_filter(L, ctx, filt)
        for col in (N.COLLOCATED if filt == R.TRIANGLE else [N.COLLOCATED[1]]):
            for fmt in ("rgb8", "rgbf16"):
                want = expected(pic, origins, wsize, fmt, filt, size, bd, col)
                batch(L, ctx, 0, origins, wsize, fmt, want, "filter %d, %s at %d bits, collocated %r" % (filt, fmt, bd, col), size=size, col=col, home=home)


def check_wide_and_two_launch(L, ctx, write, bd, home=Pageable):
    """more than one tile across with a narrow last one (cubic, rgb16); the two-launch form, whose horizontal results are per region (area, rgb8)"""
    pic = picture(bd, 20 + bd)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    for (wsize, size, origins), filt, fmt in ((WIDE, R.CUBIC, "rgb16"), (TWO_LAUNCH, R.AREA, "rgb8")):
        N.set_filter(L, ctx, filt)
        want = expected(pic, origins, wsize, fmt, filt, size, bd)
        batch(L, ctx, 0, origins, wsize, fmt, want, "%r -> %r under filter %d, %s at %d bits" % (wsize, size, filt, fmt, bd), size=size, home=home)


def check_dctif(L, ctx, write, bd, backend, tmpdir, home=Pageable):
    """no filter set: the reference's DCTIF, k_rescale with the region as its third grid dimension"""
    wsize, size, origins = DCTIF
    pic = picture(bd, 30 + bd)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    col = (True, False)
    want = expected(pic, origins, wsize, "rgb8", None, size, bd, col, dctif=rescale_plane_frames(backend, tmpdir, size, bd, col))
    batch(L, ctx, 0, origins, wsize, "rgb8", want, "DCTIF %r -> %r at %d bits" % (wsize, size, bd), size=size, col=col, home=home)


def offset_lut(n=17, offset=(300, -200, 1000)):
    """identity plus an offset per channel, clipped: node ( jb, jg, jr ) = min( j * S, 65535 ) + offset"""
    j = np.minimum(np.arange(n) * (1 << U.shift(n)), 65535)
    jb, jg, jr = np.meshgrid(j, j, j, indexing="ij")
    nodes = np.stack([jr + offset[0], jg + offset[1], jb + offset[2]], -1)
    return n, np.clip(nodes, 0, 65535).astype(np.uint16).reshape(-1)


def check_transform_and_lut(L, ctx, write, home=Pageable):
    """the second geometry under the triangle filter, rgb16 at 10 bits: the PQ-to-sRGB preset, then a 17-point identity-plus-offset LUT, then both"""
    bd = 10
    wsize, size, origins = SECOND
    pic = picture(bd, 40)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    N.set_filter(L, ctx, R.TRIANGLE)
    pq = X.preset(16, 9, 0, 1000., 100., bd)
    lut = offset_lut()
    for what, transform, l in (("the PQ-to-sRGB preset", pq, None), ("a 17-point LUT", None, lut), ("the preset and the LUT", pq, lut)):
        TH.set_transform(L, ctx, transform)
        LH.set_lut(L, ctx, l)
        want = expected(pic, origins, wsize, "rgb16", R.TRIANGLE, size, bd, transform=transform, lut=l)
        batch(L, ctx, 0, origins, wsize, "rgb16", want, "rgb16 under " + what, size=size, home=home)
    TH.set_transform(L, ctx, None)
    LH.set_lut(L, ctx, None)


def check_limit(L, ctx, write, bd=10, home=Pageable):
    """256 regions of 16 x 16 on a grid, wrapping with duplicates; 257 are refused"""
    wsize, _, origins = LIMIT
    pic = picture(bd, 50)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    assert len(origins) == abi.OUT_BATCH_MAX and len(set(origins)) == 65
    batch(L, ctx, 0, origins, wsize, "rgb8", expected(pic, origins, wsize, "rgb8", bd=bd), "256 regions", home=home)
    t, d = submit(L, ctx, 0, origins + [(0, 0)], wsize, "rgb8")
    assert t == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx).startswith(WHO), (t, L.vvr_last_error(ctx))
    d.untouched("a refused batch of 257")
    d.close()


def check_a_batch_of_one_is_the_single_request(L, ctx, write, bd=10):
    """a consistency check, not the oracle: count = 1 stores the bytes of vvr_output_submit for the same window, under a filter and without"""
    pic = picture(bd, 60)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    for filt, (wsize, size, origins) in ((R.REFERENCE, STRAIGHT), (R.CUBIC, SECOND)):
        N.set_filter(L, ctx, filt)
        o = origins[1]
        for fmt in ("rgb8", "rgba16f"):
            single = Q.queued(L, ctx, 0, o + wsize, fmt, 3, size=size)
            batch(L, ctx, 0, [o], wsize, fmt, [[np.ascontiguousarray(p) for p in single]], "a batch of one, %s under filter %d" % (fmt, filt), size=size)


def check_destinations(L, ctx, write, homes=HOMES, bd=10):
    """the second geometry with rgbf32: pageable memory; vvr_host_alloc memory with dst_stride_bytes = row + 6 and batch_stride_bytes = the
    plane's extent + 10; a device range with a contiguous ( N, 3, H, W ) layout, the direct store; a device range with batch_stride_bytes =
    extent + 6, not a multiple of 32.  The guard bytes of every one come back untouched (Dest.check compares the whole buffer)"""
    wsize, size, origins = SECOND
    pic = picture(bd, 70)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    N.set_filter(L, ctx, R.TRIANGLE)
    assert I.set_norm(L, ctx, NORM) == abi.VVR_OK
    want = expected(pic, origins, wsize, "rgbf32", R.TRIANGLE, size, bd, norm=NORM)
    pageable, pinned, device = homes
    for home, kw in ((pageable, dict(layout="packed")), (pageable, dict(layout="padded")), (pinned, dict(layout="padded", batch_pad=10)), (pinned, dict(layout="packed")),
                     (device, dict(layout="packed")), (device, dict(layout="padded", batch_pad=6)), (device, dict(layout="packed", mis=4))):
        if home is None:
            continue
        batch(L, ctx, 0, origins, wsize, "rgbf32", want, "rgbf32, %r" % (kw,), size=size, home=home, **kw)
    assert I.set_norm(L, ctx, None) == abi.VVR_OK


IN_FLIGHT = [(R.AREA, "rgb8"), (R.TRIANGLE, "rgb16"), (R.CUBIC, "rgbf16"), (R.AREA, "rgbf32"), (R.TRIANGLE, "rgba8"), (R.CUBIC, "bgr24"), (R.AREA, "rgb10a2"), (R.TRIANGLE, "rgba16f")]


def check_in_flight(L, ctx, write, bd=10):
    """eight batch requests of different filters and formats in flight, collected out of order; a ninth is VVR_ERR_BUSY"""
    wsize, size, origins = SECOND
    pic = picture(bd, 80)
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    flight = []
    for n, (filt, fmt) in enumerate(IN_FLIGHT):
        N.set_filter(L, ctx, filt)
        org = origins[n % 4:] + origins[:n % 4]
        t, d = submit(L, ctx, 0, org, wsize, fmt, size=size)
        assert t >= 2, (n, t, L.vvr_last_error(ctx))
        flight.append((t, d, expected(pic, org, wsize, fmt, filt, size, bd), "request %d: %s under filter %d" % (n, fmt, filt)))
    assert len(set(f[0] for f in flight)) == 8
    t, d = submit(L, ctx, 0, origins, wsize, "rgb8", size=size)
    assert t == abi.VVR_ERR_BUSY and L.vvr_last_error(ctx).startswith(WHO), (t, L.vvr_last_error(ctx))
    for n in (5, 0, 7, 2, 3, 6, 1, 4):
        collect(L, ctx, *flight[n])


def check_refusals(L, mk_ctx, write, bd=10):
    """every item of the refusal list: VVR_ERR_PARAMETER and a text that names vvr_output_submit_batch; then eight requests are still accepted
    (no ring entry leaked), and vvr_output_submit itself is as before"""
    wsize, size, origins = SECOND
    pic = picture(bd, 90)
    fresh = mk_ctx()
    write(fresh, 0, pic)

    def refused(ctx, text, origins=origins, wsize=wsize, fmt="rgb8", size=size, change=None, **kw):
        d = Dest(L, ctx, max(1, len(origins)), wsize, fmt, size, **kw)
        req, b, keep = d.request(0, wsize, fmt, size, (True, False), origins=origins)
        if change:
            change(req, b)
        t = L.vvr_output_submit_batch(ctx, C.byref(req), C.byref(b))
        err = L.vvr_last_error(ctx)
        assert t == abi.VVR_ERR_PARAMETER and err.startswith(WHO) and text in err, (text, t, err)
        d.untouched("refused: " + text.decode())
        d.close()

    # what vvr_output_submit refuses for the same request, with its text behind the new name: no colour description yet
    refused(fresh, b"RGB output with no colour description set (vvr_set_output_colour)")
    L.vvr_destroy(fresh)
    ctx = mk_ctx()
    write(ctx, 0, pic)
    setup_colour(L, ctx)
    N.set_filter(L, ctx, R.TRIANGLE)
    refused(ctx, b"struct_size is not sizeof( vvr_output_request )", change=lambda r, b: setattr(r, "struct_size", r.struct_size - 8))
    refused(ctx, b"struct_size is not sizeof( vvr_output_batch )", change=lambda r, b: setattr(b, "struct_size", b.struct_size + 8))
    refused(ctx, b"count must be 1 .. 256", change=lambda r, b: setattr(b, "count", 0))
    refused(ctx, b"count must be 1 .. 256", change=lambda r, b: setattr(b, "count", 257))
    refused(ctx, b"origin is NULL", change=lambda r, b: setattr(b, "origin", C.POINTER(C.c_int32)()))
    refused(ctx, b"x and y of the request must be 0", change=lambda r, b: setattr(r, "x", 2))
    refused(ctx, b"x and y of the request must be 0", change=lambda r, b: setattr(r, "y", 2))
    refused(ctx, b"region 2: window outside the picture, or odd in 4:2:0", origins=[(0, 0), (2, 2), (114, 32), (0, 0)])
    refused(ctx, b"region 1: window outside the picture, or odd in 4:2:0", origins=[(0, 0), (0, 34)])
    refused(ctx, b"region 3: window outside the picture, or odd in 4:2:0", origins=[(0, 0), (2, 2), (4, 4), (3, 2)])
    refused(ctx, b"region 0: window outside the picture, or odd in 4:2:0", origins=[(-2, 0)])
    refused(ctx, b"grain is not offered for a batch", change=lambda r, b: setattr(r, "grain", 1))
    for fmt in ("planar16", "nv12", "yuv444p8", "packed10"):
        refused(ctx, b"a batch takes the ten R'G'B' formats", change=lambda r, b, fmt=fmt: setattr(r, "format", abi.OUT_FORMATS[fmt]))
    refused(ctx, b"unknown format", change=lambda r, b: setattr(r, "format", 200))

    def short_stride(r, b):
        b.batch_stride_bytes[1] = 28 * 12 - 1
    refused(ctx, b"batch_stride_bytes below the plane's extent", change=short_stride)
    refused(ctx, b"batch_stride_bytes below the plane's extent", layout="padded", batch_pad=-1)

    def huge(r, b):      # 256 regions of 208 x 80 -> 1664 x 640 float32: 12.8 MB of outputs and 3.2 MB of resampled planes each
        r.w, r.h, r.out_w, r.out_h, r.format = 208, 80, 1664, 640, abi.OUT_FORMATS["rgbf32"]
        for k in range(3):
            r.dst_stride_bytes[k] = 1664 * 4
            b.batch_stride_bytes[k] = 3 * 1664 * 640 * 4
    refused(ctx, b"would exceed the limit of 512 MiB", origins=[(0, 0)] * 256, change=huge)
    # ... and more of what vvr_output_submit refuses for the same request
    refused(ctx, b"RGB output needs an even out_w and out_h", change=lambda r, b: setattr(r, "out_w", 27))
    refused(ctx, N.REFUSAL, change=lambda r, b: setattr(r, "out_h", 2 * 8194))
    refused(ctx, b"no such slot", change=lambda r, b: setattr(r, "slot", 7))
    refused(ctx, b"job must be a job id or -1", change=lambda r, b: setattr(r, "job", -2))
    refused(ctx, b"window outside the picture, or odd in 4:2:0", change=lambda r, b: setattr(r, "w", 210))
    refused(ctx, b"missing plane or stride below the output's row", change=lambda r, b: r.dst_stride_bytes.__setitem__(2, 27))
    assert L.vvr_output_submit_batch(ctx, None, None) == abi.VVR_ERR_PARAMETER
    # no ring entry leaked: eight requests are still accepted, the ninth is busy
    flight = [submit(L, ctx, 0, origins, wsize, "rgb8", size=size) for _ in range(8)]
    assert all(t >= 2 for t, _ in flight) and len(set(t for t, _ in flight)) == 8, [t for t, _ in flight]
    assert submit(L, ctx, 0, origins, wsize, "rgb8", size=size)[0] == abi.VVR_ERR_BUSY
    want = expected(pic, origins, wsize, "rgb8", R.TRIANGLE, size, bd)
    for t, d in flight:
        collect(L, ctx, t, d, want, "after the refusals")
    # vvr_output_submit itself: its bytes and its name
    N.same(Q.queued(L, ctx, 0, origins[1] + wsize, "rgb8", 3, size=size), want[1], "vvr_output_submit after the refusals")
    t, _ = Q.submit(L, ctx, 0, (0, 0, 210, 80), "rgb8", 3)
    assert t == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx) == b"vvr_output_submit: window outside the picture, or odd in 4:2:0"
    L.vvr_destroy(ctx)


# ---- the tests on the stand-in runtime

def _run(check, bd, *args, **kw):
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, W, H_, bd, 1)
    check(L, ctx, SUP.writer(L), *args, **kw)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_no_scaling(bd):
    _run(check_straight, bd, bd)


@pytest.mark.parametrize("bd", [10, 8])
def test_antialiased_one_launch_per_plane(bd):
    _run(check_antialiased, bd, bd)


@pytest.mark.parametrize("bd", [10, 8])
def test_more_than_one_tile_across_and_the_two_launch_form(bd):
    _run(check_wide_and_two_launch, bd, bd)


@need_ref
@pytest.mark.parametrize("bd", [10, 8])
def test_dctif_is_rescale_plane(tmp_path, bd):
    _run(check_dctif, bd, bd, T.build_stub(), str(tmp_path))


def test_transform_and_lut():
    _run(check_transform_and_lut, 10)


def test_count_at_the_limit():
    _run(check_limit, 10)


def test_a_batch_of_one_is_the_single_request():
    _run(check_a_batch_of_one_is_the_single_request, 10)


def test_destinations():
    _run(check_destinations, 10)


def test_eight_batches_in_flight():
    _run(check_in_flight, 10)


def test_refusals_leave_the_ring_alone():
    L = SUP.stub_lib()
    check_refusals(L, lambda: SUP.make_ctx(L, W, H_, 10, 1), SUP.writer(L))


def test_python_mirror():
    import vvdec_amd
    assert C.sizeof(abi.OutputBatch) == 40 and abi.OutputBatch.count.offset == 4 and abi.OutputBatch.origin.offset == 8 and abi.OutputBatch.batch_stride_bytes.offset == 16
    assert abi.OUT_BATCH_MAX == 256 and len(abi.OUT_BATCH_FORMATS) == 10 and all(f in abi.OUT_FORMATS for f in abi.OUT_BATCH_FORMATS)
    assert "vvr_output_submit_batch" in vvdec_amd.EXPORTED_SYMBOLS and hasattr(SUP.stub_lib(), "vvr_output_submit_batch")
    assert hasattr(vvdec_amd.Reconstructor, "output_submit_batch")
