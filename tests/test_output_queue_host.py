"""CPU: the output queue (vvr_output_submit / vvr_output_test / vvr_output_wait) on the stand-in runtime of tests/hoststub, whose launchers of the
output stage are plain loops (vvr_output.inc, host only; launch_output_window in the stub itself).  Planar requests must give the bytes of the
synchronous calls (vvr_read_output, _scaled, _grain: pinned to the reference by their own tests), packed requests the bytes of the application's
writer (_writeComponentToFile, vvdecHelper.h:106-145 and :201-248, restated in numpy here), grain with a size the reference's chain: vvdec::FilmGrain
(tests/film_grain_ref.py), then vvdec::rescalePlane (tests/rescale_ref.py).  The helpers take a library and a context, so tests/test_gpu_output_queue.py
runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import rescale_ref
import test_film_grain_host as H
import test_host_glue as T
from vvdec_amd import abi, stream, synth

pytestmark = T.pytestmark
need_ref = pytest.mark.skipif(not (film_grain_ref.available() and rescale_ref.available()), reason="oracle/_ref/libvvref.so / libvvdec.so not built (needs /root/reference at build time)")




def submit(L, ctx, slot, win, fmt, ncomp, size=None, col=(True, False), grain=False, job=None, pad=(3, 5, 7), blocking=True, alloc=None):
    """one vvr_output_submit into destinations whose rows are `pad` elements longer than the output's -> (ticket or error, the padded arrays);
    alloc( nbytes ) -> address: where the destinations live (default: numpy's, pageable)"""
    shapes, dt = abi.output_plane_shapes(win, fmt, size, ncomp)
    outs = []
    for c, (r, n) in enumerate(shapes):
        if alloc is None:
            a = np.empty((r, n + pad[c]), dt)
        else:
            nbytes = r * (n + pad[c]) * np.dtype(dt).itemsize
            a = np.frombuffer((C.c_char * nbytes).from_address(alloc(nbytes)), dt).reshape(r, n + pad[c])
        a.view(np.uint8)[...] = SUP.FILL
        outs.append(a)
    req = abi.output_request(slot, job, win, fmt, size, col, grain, blocking, outs)
    return L.vvr_output_submit(ctx, C.byref(req)), outs


def collect(L, ctx, ticket, outs, pad=(3, 5, 7)):
    """vvr_output_wait; nothing was written past a row -> the planes without their padding"""
    rc = L.vvr_output_wait(ctx, ticket)
    assert rc == abi.VVR_OK, (rc, L.vvr_last_error(ctx))
    return unpadded(outs, pad)


def unpadded(outs, pad=(3, 5, 7)):
    for c, a in enumerate(outs):
        assert pad[c] == 0 or (a[:, a.shape[1] - pad[c]:].view(np.uint8) == SUP.FILL).all(), "wrote beyond the row"
    return [a[:, :a.shape[1] - pad[c]] if pad[c] else a for c, a in enumerate(outs)]


def queued(L, ctx, slot, win, fmt, ncomp, **kw):
    pad = kw.get("pad", (3, 5, 7))
    t, outs = submit(L, ctx, slot, win, fmt, ncomp, **kw)
    assert t >= 0, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, outs, pad)


def sync_read(L, ctx, slot, win, bps, ncomp, size=None, col=(True, False), grain=False):
    """the same output by the synchronous calls (plane by plane, as Reconstructor.read_output drives them)"""
    x, y, w, h = win
    if grain:
        rc, got = H.read_grain(L, ctx, slot, win, bps, ncomp, call=L.vvr_read_output_grain)
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        return [np.ascontiguousarray(g) for g in got]
    out = []
    for c in range(ncomp):
        s = 1 if c else 0
        ow, oh = size or (w, h)
        a = np.zeros((oh >> s, ow >> s), np.uint8 if bps == 1 else np.uint16)
        if size is None:
            rc = L.vvr_read_output(ctx, slot, c, x >> s, y >> s, w >> s, h >> s, bps, a.ctypes.data, a.strides[0])
        else:
            rc = L.vvr_read_output_scaled(ctx, slot, c, x >> s, y >> s, w >> s, h >> s, ow >> s, oh >> s, int(col[0]) | int(col[1]) << 1, bps, a.ctypes.data, a.strides[0])
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        out.append(a)
    return out


def pack10(plane, bd):
    """_writeComponentToFile with writePYUV: four values into five bytes, low byte first; 8-bit planes (bytesPerSample 1) as p << 2"""
    p = plane.astype(np.int64) << (2 if bd == 8 else 0)
    assert p.shape[1] % 4 == 0
    t = p[:, 0::4] + (p[:, 1::4] << 10) + (p[:, 2::4] << 20) + (p[:, 3::4] << 30)
    return np.stack([(t >> (8 * k)) & 0xff for k in range(5)], axis=2).astype(np.uint8).reshape(p.shape[0], p.shape[1] // 4 * 5)


def grain_then_rescale_by_the_synchronous_calls(L, mk_ctx, ctx, slot, win, size, col, bps, ncomp, bd):
    """vvr_read_output_grain of the window, the grained frame written into the corner of a slot of a second context, vvr_read_output_scaled of it"""
    grained = sync_read(L, ctx, slot, win, 2, ncomp, grain=True)
    W, H_ = (win[2] + 7) & ~7, (win[3] + 7) & ~7
    ctx2 = mk_ctx(W, H_)
    for c, g in enumerate(grained):
        full = np.zeros((H_ >> (1 if c else 0), W >> (1 if c else 0)), np.uint16)
        full[:g.shape[0], :g.shape[1]] = g
        assert L.vvr_write_plane(ctx2, 0, c, full.ctypes.data, full.shape[1]) == abi.VVR_OK
    out = sync_read(L, ctx2, 0, (0, 0, win[2], win[3]), bps, ncomp, size=size, col=col)
    L.vvr_destroy(ctx2)
    return out


def matrix(bd, cf):
    """(slot, window, size, collocated, grain): slot 0 a 448 x 160 picture, slot 1 a 200 x 104 picture in a slot of that size; windows at odd
    offsets and of odd sizes in 4:0:0, widths that are no multiple of 16 (k_output_frame: rows that end inside a lane's piece), up and down"""
    odd = 0 if cf else 1
    return [(0, (0, 0, 448, 160), None, (True, False), False),
            (0, (2 + odd, 6 + odd, 200 + odd, 40 + odd), None, (True, False), False),
            (0, (10, 16 + odd, 146, 50), None, (True, False), False),
            (0, (4 + odd, 2, 384, 98), (576, 148), (True, False), False),
            (0, (10, 16, 146, 50), (100 + 2 * odd, 36), (False, True), False),
            (0, (0, 0, 448, 160), None, (True, False), True),
            (0, (2 + odd, 6 + odd, 200 + odd, 40 + odd), None, (True, False), True),
            (1, (4, 2, 160, 96), None, (True, False), False),
            (1, (0, 0, 200, 104), None, (True, False), True),
            (1, (0, 0, 200, 104), (400, 208), (True, True), False)]


def packed_matrix(bd, cf):
    """(slot, window, size, collocated, grain) with plane widths that are multiples of 4"""
    odd = 0 if cf else 1
    return [(0, (0, 0, 448, 160), None, (True, False), False),
            (0, (8 + odd, 4 + odd, 200, 40 + odd), None, (True, False), False),      # 25 groups per luma row: rows that end inside a lane's piece
            (0, (0, 0, 448, 160), (224, 80), (True, False), False),
            (0, (4 + odd, 2, 384, 98), (576, 148), (False, True), False),
            (0, (0, 0, 448, 160), None, (True, False), True),
            (0, (8, 4, 200, 40), (400, 80), (True, False), True),
            (0, (4, 2, 384, 96), (256, 64), (False, False), True),
            (1, (0, 0, 200, 104), None, (True, False), False)]


def setup(L, mk_ctx, write, rng, bd, cf):
    """a context with the two pictures of the matrices and a random bank -> ctx, the bank (kept alive by the caller)"""
    ctx = mk_ctx(448, 160)
    write(ctx, 0, film_grain_ref.grain_picture(rng, 448, 160, bd, cf))
    assert L.vvr_slot_picture_size(ctx, 1, 200, 104) == abi.VVR_OK
    small = film_grain_ref.grain_picture(rng, 200, 104, bd, cf)
    for c, p in enumerate(small):
        assert L.vvr_write_plane(ctx, 1, c, np.ascontiguousarray(p).ctypes.data, p.shape[1]) == abi.VVR_OK
    bank = abi.film_grain_bank(**H._bank(rng))
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    return ctx, bank


def check_planar(L, ctx, bd, cf):
    nc = 3 if cf else 1
    for n, (slot, win, size, col, grain) in enumerate(matrix(bd, cf)):
        for fmt, bps in [("planar16", 2)] + ([("planar8", 1)] if bd == 8 else []):
            assert L.vvr_set_film_grain_seed(ctx, 1000 + n) == abi.VVR_OK
            want = sync_read(L, ctx, slot, win, bps, nc, size=size, col=col, grain=grain)
            assert L.vvr_set_film_grain_seed(ctx, 1000 + n) == abi.VVR_OK
            got = queued(L, ctx, slot, win, fmt, nc, size=size, col=col, grain=grain)
            for c in range(nc):
                assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c]), "case %d %s component %d: %d samples differ" % (n, fmt, c, int((got[c] != want[c]).sum()))


def check_packed(L, mk_ctx, ctx, bd, cf):
    nc = 3 if cf else 1
    for n, (slot, win, size, col, grain) in enumerate(packed_matrix(bd, cf)):
        assert L.vvr_set_film_grain_seed(ctx, 2000 + n) == abi.VVR_OK
        if grain and size:
            want = grain_then_rescale_by_the_synchronous_calls(L, mk_ctx, ctx, slot, win, size, col, 2, nc, bd)
        else:
            want = sync_read(L, ctx, slot, win, 2, nc, size=size, col=col, grain=grain)
        assert L.vvr_set_film_grain_seed(ctx, 2000 + n) == abi.VVR_OK
        got = queued(L, ctx, slot, win, "packed10", nc, size=size, col=col, grain=grain)
        for c in range(nc):
            w_ = pack10(want[c], bd)
            assert got[c].shape == w_.shape and np.array_equal(got[c], w_), "case %d component %d: %d bytes differ" % (n, c, int((got[c] != w_).sum()))
        if grain and size:       # ... and the chain in the planar format
            assert L.vvr_set_film_grain_seed(ctx, 2000 + n) == abi.VVR_OK
            got = queued(L, ctx, slot, win, "planar16", nc, size=size, col=col, grain=True)
            assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), "case %d: grain, then rescale, planar" % n


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_planar_formats_match_the_synchronous_calls(bd, cf):
    L = SUP.stub_lib()
    ctx, bank = setup(L, lambda W, H_: SUP.make_ctx(L, W, H_, bd, cf), lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(bd + cf), bd, cf)
    check_planar(L, ctx, bd, cf)
    # a window beyond the picture in the slot (inside the slot) is refused
    t, _ = submit(L, ctx, 1, (8, 0, 200, 104), "planar16", 3 if cf else 1)
    assert t == abi.VVR_ERR_PARAMETER and b"outside the picture" in L.vvr_last_error(ctx)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_packed10_matches_the_applications_writer(bd, cf):
    L = SUP.stub_lib()
    mk = lambda W, H_: SUP.make_ctx(L, W, H_, bd, cf)
    ctx, bank = setup(L, mk, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(20 + bd + cf), bd, cf)
    check_packed(L, mk, ctx, bd, cf)
    L.vvr_destroy(ctx)


CHAIN_CASES = [((8, 4, 200, 64), (400, 128), (True, False)), ((4, 2, 384, 96), (256, 64), (False, True)), ((0, 0, 448, 160), (672, 240), (True, True))]


def reference_chain(picture, sei, cases, backend, tmpdir):
    """the frames of `cases` (window, size, collocated) grained by one vvdec::FilmGrain in order, each then rescaled plane by plane by
    vvdec::rescalePlane (plain C++ path) -> the bank, the list of frames"""
    banks, grained = film_grain_ref.expected(picture, [("fgc", sei)] + [("frame", win, 2) for win, _, _ in cases], 10, 1, tmpdir, "chain")
    rc = [(g[c], size[0] >> (1 if c else 0), size[1] >> (1 if c else 0), c, 1, 10, col[0], col[1]) for g, (_, size, col) in zip(grained, cases) for c in range(3)]
    out = rescale_ref.rescale(rc, backend, False, tmpdir)
    return banks[0], [out[3 * n:3 * n + 3] for n in range(len(cases))]


@need_ref
def test_grain_then_rescale_is_the_reference_chain(tmp_path):
    """10-bit 4:2:0, ratios 2, 2/3 and 3/2, three collocation settings, one seed chain over the three frames; scale factors below 128"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(31)
    picture = film_grain_ref.grain_picture(rng, 448, 160, 10, 1)
    bank, want = reference_chain(picture, film_grain_ref.random_sei(rng, 1, 3, 5), CHAIN_CASES, T.build_stub(), str(tmp_path))
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, picture)
    keep = abi.film_grain_bank(**bank)
    assert L.vvr_set_film_grain(ctx, C.addressof(keep)) == abi.VVR_OK
    for (win, size, col), w_ in zip(CHAIN_CASES, want):
        got = queued(L, ctx, 0, win, "planar16", 3, size=size, col=col, grain=True)
        for c in range(3):
            assert np.array_equal(got[c], w_[c]), "%r -> %r component %d: %d samples differ" % (win, size, c, int((got[c] != w_[c]).sum()))
    L.vvr_destroy(ctx)


@need_ref
def test_the_seed_chain_is_shared(tmp_path):
    """synchronous grained reads and queued grained requests interleaved on one context: the reference's sequence for the same frames; a refused
    request in between does not advance the chain; several requests in flight advance it in submission order"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(32)
    picture = film_grain_ref.grain_picture(rng, 448, 160, 10, 1)
    wins = [(0, 0, 136, 64), (2, 6, 200, 40), (4, 2, 384, 98), (10, 16, 146, 50), (0, 0, 448, 160), (40, 30, 256, 66)]
    banks, want = film_grain_ref.expected(picture, [("fgc", film_grain_ref.random_sei(rng, 0, 3, 4))] + [("frame", w, 2) for w in wins], 10, 1, str(tmp_path))
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, picture)
    keep = abi.film_grain_bank(**banks[0])
    assert L.vvr_set_film_grain(ctx, C.addressof(keep)) == abi.VVR_OK
    got = [sync_read(L, ctx, 0, wins[0], 2, 3, grain=True), queued(L, ctx, 0, wins[1], "planar16", 3, grain=True)]
    assert submit(L, ctx, 0, (0, 0, 128, 64), "planar16", 3, grain=True)[0] == abi.VVR_ERR_PARAMETER             # refused: the chain stays
    assert submit(L, ctx, 0, (0, 0, 204, 64), "packed10", 3, grain=True)[0] == abi.VVR_ERR_PARAMETER            # (chroma rows of 102 samples)
    got.append(sync_read(L, ctx, 0, wins[2], 2, 3, grain=True))
    flight = [submit(L, ctx, 0, w, "planar16", 3, grain=True) for w in wins[3:5]]                                  # two in flight, collected in reverse
    assert all(t >= 0 for t, _ in flight)
    late = [collect(L, ctx, t, outs) for t, outs in reversed(flight)][::-1]
    got += late
    got.append(sync_read(L, ctx, 0, wins[5], 2, 3, grain=True))
    for n, (g, w_) in enumerate(zip(got, want)):
        assert all(np.array_equal(a, b) for a, b in zip(g, w_)), "frame %d" % n
    L.vvr_destroy(ctx)


def test_refusals_tickets_and_the_ring():
    L = SUP.stub_lib()
    rng = np.random.default_rng(33)
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, film_grain_ref.grain_picture(rng, 448, 160, 10, 1))
    win = (8, 4, 200, 64)

    def refused(text, code=abi.VVR_ERR_PARAMETER, c=ctx, **kw):
        args = dict(slot=0, win=win, fmt="planar16", ncomp=3)
        args.update(kw)
        mutate = args.pop("mutate", None)
        shapes, dt = abi.output_plane_shapes(args["win"], args["fmt"], args.get("size"), args["ncomp"])
        outs = [np.zeros(s, dt) for s in shapes]
        req = abi.output_request(args["slot"], args.get("job"), args["win"], args["fmt"], args.get("size"), (True, False), args.get("grain", False), True, outs)
        if mutate:
            mutate(req)
        rc = L.vvr_output_submit(c, C.byref(req))
        assert rc == code and text in L.vvr_last_error(c), (kw, rc, L.vvr_last_error(c))

    refused(b"struct_size", mutate=lambda r: setattr(r, "struct_size", C.sizeof(abi.OutputRequest) - 8))
    for w_ in [(300, 0, 200, 64), (0, 120, 200, 64), (-2, 0, 200, 64), (0, 0, 200, 0), (1, 0, 200, 64), (0, 1, 200, 64), (0, 0, 201, 64), (0, 0, 200, 63)]:
        refused(b"outside the picture, or odd", win=w_)
    refused(b"8-bit output", fmt="planar8")
    refused(b"multiples of 4", fmt="packed10", win=(0, 0, 204, 64))          # chroma rows of 102
    refused(b"multiples of 4", fmt="packed10", size=(404, 128))              # the OUTPUT's width counts
    refused(b"no film grain bank", grain=True)
    refused(b"1/8", size=(8, 64))
    refused(b"no such slot", slot=7)
    refused(b"unknown format", mutate=lambda r: setattr(r, "format", 3))
    refused(b"missing plane or stride", mutate=lambda r: r.dst_stride_bytes.__setitem__(1, 199))
    refused(b"missing plane or stride", mutate=lambda r: r.dst.__setitem__(2, None))
    bank = abi.film_grain_bank(**H._bank(rng))
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    refused(b"wider than 128", grain=True, win=(0, 0, 128, 64))
    ctx9 = SUP.make_ctx(L, 448, 160, 9, 1)
    refused(b"bit depth of 8 or 10", c=ctx9, fmt="packed10")
    L.vvr_destroy(ctx9)
    # tickets: test leaves the ticket, wait retires it; unknown tickets
    t, outs = submit(L, ctx, 0, win, "planar16", 3)
    assert t >= 0 and L.vvr_output_test(ctx, t) == abi.VVR_OK and L.vvr_output_test(ctx, t) == abi.VVR_OK
    assert L.vvr_sync(ctx) == abi.VVR_OK and L.vvr_output_test(ctx, t) == abi.VVR_OK          # vvr_sync retires nothing
    first = collect(L, ctx, t, outs)
    assert L.vvr_output_wait(ctx, t) == abi.VVR_ERR_PARAMETER and b"ticket" in L.vvr_last_error(ctx)
    assert L.vvr_output_test(ctx, t) == abi.VVR_ERR_PARAMETER and L.vvr_output_wait(ctx, 12345) == abi.VVR_ERR_PARAMETER and L.vvr_output_wait(ctx, -1) == abi.VVR_ERR_PARAMETER
    # eight in flight, the ninth is refused and leaves the seed chain alone; every one of the eight is right
    assert L.vvr_set_film_grain_seed(ctx, 77) == abi.VVR_OK
    want = [sync_read(L, ctx, 0, win, 2, 3, grain=True) for _ in range(9)]
    assert L.vvr_set_film_grain_seed(ctx, 77) == abi.VVR_OK
    flight = [submit(L, ctx, 0, win, "planar16", 3, grain=True) for _ in range(8)]
    assert all(t >= 0 for t, _ in flight) and len(set(t for t, _ in flight)) == 8
    t9, _ = submit(L, ctx, 0, win, "planar16", 3, grain=True)
    assert t9 == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    got = [collect(L, ctx, t, outs) for t, outs in flight]
    got.append(queued(L, ctx, 0, win, "planar16", 3, grain=True))            # (the ninth frame of the chain, not the tenth)
    for n in range(9):
        assert all(np.array_equal(a, b) for a, b in zip(got[n], want[n])), n
    L.vvr_destroy(ctx)


def test_destinations_in_pinned_memory_are_written_by_the_copy():
    """every plane in memory of vvr_host_alloc: the rows are in place, at the padded stride, before vvr_output_wait is called (the stand-in's copies
    run at once) and the padding is untouched; pageable destinations: nothing arrives before vvr_output_wait"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(34)
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, film_grain_ref.grain_picture(rng, 448, 160, 10, 1))
    win = (8, 4, 200, 64)
    want = sync_read(L, ctx, 0, win, 2, 3)
    for fmt, w_ in (("planar16", want), ("packed10", [pack10(p, 10) for p in want])):
        t, outs = submit(L, ctx, 0, win, fmt, 3, alloc=lambda n: L.vvr_host_alloc(ctx, n))
        assert t >= 0
        for c in range(3):
            assert np.array_equal(outs[c][:, :w_[c].shape[1]], w_[c]), "the copy did not go straight to the caller's pinned memory"
        got = collect(L, ctx, t, outs)
        assert all(np.array_equal(a, b) for a, b in zip(got, w_))
    t, outs = submit(L, ctx, 0, win, "planar16", 3)
    assert t >= 0 and all((a.view(np.uint8) == SUP.FILL).all() for a in outs), "pageable destinations are written by vvr_output_wait"
    assert all(np.array_equal(a, b) for a, b in zip(collect(L, ctx, t, outs), want))
    L.vvr_destroy(ctx)


def _trace(L):
    scratch = (C.c_int * 60000)()
    n = L.vvt_take_trace(scratch, len(scratch))
    return [(scratch[3 * k], scratch[3 * k + 1], scratch[3 * k + 2]) for k in range(n // 3)]


def test_requests_are_ordered_on_the_device_not_on_the_host():
    """stream and event operations as the stand-in runtime records them: the output stream waits for the picture's completion event and the host
    never waits for the picture; the request's own event is recorded behind its kernels, and the picture that overwrites the slot later waits for
    exactly that event on its lane.  A job whose out_slot is another slot is refused; without `blocking` a picture still with the workers gives
    VVR_NOT_READY."""
    L = SUP.stub_lib()
    W, H_ = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = SUP.stream_ctx(L, W, H_, nslots)
    descs = [synth.picture_for_plan(pl, W, H_, seed=611, tool_flags=T.TOOLS) for pl in plans]
    pics = [d.c() for d in descs]
    win = (0, 0, W, H_)
    L.vvt_set_delay(20000)
    j0 = L.vvr_submit(ctx, C.byref(pics[0]))
    assert j0 >= 0
    t, outs = submit(L, ctx, plans[0].slot, win, "planar16", 3, job=j0, blocking=False)
    assert t == abi.VVR_NOT_READY or t >= 2        # (a ticket is never VVR_NOT_READY)
    L.vvt_set_delay(0)
    if t != abi.VVR_NOT_READY:
        collect(L, ctx, t, outs)
    other = (plans[0].slot + 1) % nslots
    bad, _ = submit(L, ctx, other, win, "planar16", 3, job=j0)
    assert bad == abi.VVR_ERR_PARAMETER and b"does not reconstruct into this slot" in L.vvr_last_error(ctx)
    _trace(L)
    L.vvt_events_pending(1)                     # (nothing the device was given has finished: events that are complete would be dropped, not waited for)
    t, outs = submit(L, ctx, plans[0].slot, win, "planar16", 3, job=j0)
    assert t >= 0 and L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY
    ops = _trace(L)
    waits, records = [(s, e) for op, s, e in ops if op == 0], [(s, e) for op, s, e in ops if op == 1]
    out_stream = records[-1][0]
    assert [s for s, _ in records if s == out_stream], "nothing recorded on the output stream"
    assert any(s == out_stream for s, _ in waits), "the output stream did not wait for the picture's event"
    read_event = [e for s, e in records if s == out_stream][0]      # the first record of the request: behind its kernels, before the copy
    # a second picture into the same slot: its lane waits for the request's read event
    again = synth.picture_for_plan(plans[0], W, H_, seed=612, tool_flags=T.TOOLS)
    pa = again.c()
    j1 = L.vvr_submit(ctx, C.byref(pa))
    assert j1 >= 0
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    assert L.vvr_stream_wait_job(ctx, j1, ext, 1) == abi.VVR_OK      # (handed to the device)
    ops = _trace(L)
    assert any(op == 0 and e == read_event and s != out_stream for op, s, e in ops), "the picture that overwrites the slot did not wait for the request's event"
    L.vvt_events_pending(0)
    collect(L, ctx, t, outs)
    # too late: the slot's next picture is with the device, the first picture's output can no longer be asked for
    late, _ = submit(L, ctx, plans[0].slot, win, "planar16", 3, job=j0)
    assert late == abi.VVR_ERR_PARAMETER and b"overwrites the slot" in L.vvr_last_error(ctx)
    t, outs = submit(L, ctx, plans[0].slot, win, "planar16", 3, job=j1)
    assert t >= 0
    collect(L, ctx, t, outs)
    assert L.vvr_sync(ctx) == abi.VVR_OK
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("out", SUP.stub_lib())


def ring_request(L, ctx, planes, win, part, ref, bd):
    def finish(t, keep, what):
        assert all(np.array_equal(a, b) for a, b in zip(collect(L, ctx, t, keep), part)), what
    return lambda: submit(L, ctx, 0, win, "planar16", 3), finish


SUP.register("out", b"vvr_output_submit", ring_request,
             failing=lambda L, ctx, slot, win, job, ref_slot: submit(L, ctx, slot, win, "planar16", 3, job=job),
             untouched=lambda outs: all((a.view(np.uint8) == SUP.FILL).all() for a in outs),
             delivered=unpadded)
