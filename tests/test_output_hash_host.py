"""CPU: decoded picture hashes as requests of the output queue (vvr_hash_submit, collected with vvr_output_test / vvr_output_wait) on the stand-in
runtime of tests/hoststub; the launchers of the two hash kernels are plain loops there (vvr_output.inc, host only).  Planes are uploaded with
vvr_write_plane, no stream is decoded.  Expected digests are those of tests/refdrv.py::picture_hash (pinned to the reference's PicYuvMD5.cpp by
tests/test_oracle_vs_ref.py), and every digest must also be what vvr_picture_hash gives for the slot.  The helpers take a library and a context,
so tests/test_gpu_output_hash.py runs the same cases on the device."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import refdrv
import test_film_grain_host as H
import test_host_glue as T
import test_output_queue_host as Q
from vvdec_amd import abi, stream, synth

pytestmark = T.pytestmark
METHODS = (abi.HASH_MD5, abi.HASH_CRC, abi.HASH_CHECKSUM)

# (W, H, chroma format, bit depth): the smallest shapes at which the kernels can go wrong - a lane of k_hash_rows takes 8 samples per pass, a wavefront 512
SHAPES = [(200, 72, 1, 10),       # luma rows: 25 chunks, chroma 100 x 36: 12 chunks and 4 samples left over, fewer rows than a wavefront has lanes
          (72, 136, 1, 8),        # one byte per sample; chroma rows of 36 samples; 136 and 68 rows: the combine has more rows than lanes and a tail
          (136, 8, 0, 10),        # one component, eight rows
          (200, 72, 1, 9),
          (7680, 16, 1, 10)]      # 122 880 bits per luma row: the CRC's exponent exceeds 2^16; rows of more than one pass (960 chunks)


def submit(L, ctx, slot, method, nc, job=None, expected=None, digest=True, blocking=True):
    """one vvr_hash_submit -> (ticket or error, what vvr_output_wait writes: the digest buffer or None, the mismatch word or None)"""
    n = abi.HASH_LEN[method]
    r = abi.HashRequest()
    r.struct_size, r.slot, r.job, r.method, r.blocking = C.sizeof(abi.HashRequest), slot, -1 if job is None else job, method, 1 if blocking else 0
    buf = (C.c_uint8 * (nc * n))(*([0xaa] * (nc * n))) if digest else None
    word = C.c_uint32(0xaaaaaaaa) if expected is not None else None
    want = None
    if buf is not None:
        r.digest = C.addressof(buf)
    if expected is not None:
        raw = b"".join(expected)
        want = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
        r.expected, r.mismatch = C.addressof(want), C.addressof(word)
    t = L.vvr_hash_submit(ctx, C.byref(r))
    if want is not None:
        C.memset(want, 0x55, len(raw))         # (the expected digests were copied inside the call)
    return t, (buf, word, nc, n)


def collect(L, ctx, ticket, keep):
    """vvr_output_wait -> (digests as a list of bytes or None, mismatch mask or None)"""
    buf, word, nc, n = keep
    rc = L.vvr_output_wait(ctx, ticket)
    assert rc == abi.VVR_OK, (rc, L.vvr_last_error(ctx))
    return None if buf is None else [bytes(buf[k * n:(k + 1) * n]) for k in range(nc)], None if word is None else word.value


def queued(L, ctx, slot, method, nc, **kw):
    t, keep = submit(L, ctx, slot, method, nc, **kw)
    assert t >= 2, (t, L.vvr_last_error(ctx))
    return collect(L, ctx, t, keep)


def sync_hash(L, ctx, slot, method, nc):
    buf, n = (C.c_uint8 * 48)(), C.c_int()
    assert L.vvr_picture_hash(ctx, slot, method, buf, C.byref(n)) == abi.VVR_OK, L.vvr_last_error(ctx)
    assert n.value == abi.HASH_LEN[method]
    return [bytes(buf[k * n.value:(k + 1) * n.value]) for k in range(nc)]


def flipped(digests, comp):
    """the digests with one byte of component `comp` changed"""
    out = list(digests)
    out[comp] = bytes([out[comp][0] ^ 0x40]) + out[comp][1:]
    return out


def check_slot(L, ctx, slot, planes, bd, what=""):
    """the three methods for the picture in `slot`: the queue's digests == refdrv.picture_hash == vvr_picture_hash; verification against equal and
    against changed digests, with and without a digest buffer"""
    nc = len(planes)
    for method in METHODS:
        want = refdrv.picture_hash(planes, bd, method)
        got, mask = queued(L, ctx, slot, method, nc)
        assert got == want and mask is None, "%s method %d: %r, expected %r" % (what, method, got, want)
        assert sync_hash(L, ctx, slot, method, nc) == want, "%s method %d: vvr_picture_hash" % (what, method)
        got, mask = queued(L, ctx, slot, method, nc, expected=want)
        assert got == want and mask == 0, "%s method %d: verified picture, mask %r" % (what, method, mask)
        comp = 1 if nc == 3 else 0
        got, mask = queued(L, ctx, slot, method, nc, expected=flipped(want, comp), digest=False)       # digest == NULL with expected is accepted
        assert got is None and mask == 1 << comp, "%s method %d: one byte of component %d changed, mask %r" % (what, method, comp, mask)


def crc_by_rows(plane, bit_depth):
    """refdrv.hash_crc restated so that numpy does the work (a 3840x2160 frame takes refdrv's byte loop six seconds): the register of every row
    from 0, all rows at once byte by byte with refdrv's table step, then the rows chained as polynomials mod x^16 + x^12 + x^5 + 1
    ( crc = crc * x^rowbits + piece ) from 0xffff, then the two zero bytes.  test_crc_by_rows_is_refdrvs_crc pins it to refdrv.hash_crc."""
    refdrv.hash_crc(np.zeros((1, 1), np.uint16), bit_depth)
    tbl = np.array(refdrv._CRC_T, np.uint32)
    a = np.ascontiguousarray(plane, dtype=np.uint16)
    data = a.astype("<u2").view(np.uint8).reshape(a.shape[0], -1) if bit_depth > 8 else a.astype(np.uint8)
    reg = np.zeros(a.shape[0], np.uint32)
    for x in range(data.shape[1]):
        reg = (((reg << 8) & 0xffff) | data[:, x]) ^ tbl[reg >> 8]

    def mul(p, q):
        r = 0
        for bit in range(15, -1, -1):
            r <<= 1
            if r & 0x10000:
                r ^= 0x11021
            if (q >> bit) & 1:
                r ^= p
        return r

    def xpow(n):
        r, base = 1, 2
        while n:
            if n & 1:
                r = mul(r, base)
            base = mul(base, base)
            n >>= 1
        return r
    x_row, crc = xpow(8 * data.shape[1]), 0xffff
    for piece in reg.tolist():
        crc = mul(crc, x_row) ^ piece
    crc = mul(crc, xpow(16))
    return bytes([crc >> 8, crc & 0xff])


def test_the_request_mirrors_the_header(tmp_path):
    """sizeof / offsetof of vvr_hash_request as gcc sees include/vvr.h == abi.HashRequest (vvr_abi_sizeof does not list the struct: it is guarded by
    its own struct_size)"""
    SUP.assert_mirrors(tmp_path, [("vvr_hash_request", abi.HashRequest)])


def test_lane_structure_of_the_kernels_replayed_on_the_cpu(tmp_path):
    """tests/hash_lanes_replay.cpp: what the plain-loop launchers of the stand-in runtime leave out - end-aligned chunks, the shuffle tree, the tail,
    the 256-thread combine, the host's powers of x - against the bit-serial CRC and the per-sample checksum; shapes incl. 7680-wide rows, rows of
    one chunk and rows shorter than a chunk, more rows than a workgroup has threads"""
    import os
    import subprocess
    exe = str(tmp_path / "replay")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(T.HERE, "hash_lanes_replay.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-2000:]


def test_crc_by_rows_is_refdrvs_crc():
    rng = np.random.default_rng(40)
    for W, H_, cf, bd in SHAPES:
        for p in SUP.random_planes(rng, W, H_, bd, cf):
            assert crc_by_rows(p, bd) == refdrv.hash_crc(p, bd), (W, H_, bd, p.shape)


@pytest.mark.parametrize("W,H_,cf,bd", SHAPES)
def test_digests_and_verification(W, H_, cf, bd):
    L = SUP.stub_lib()
    planes = SUP.random_planes(np.random.default_rng(W + H_ + bd), W, H_, bd, cf)
    ctx = SUP.make_ctx(L, W, H_, bd, cf)
    SUP.write_picture(L, ctx, 1, planes)
    check_slot(L, ctx, 1, planes, bd, "%dx%d" % (W, H_))
    L.vvr_destroy(ctx)


def small_picture_in_a_larger_slot(L, ctx, write, rng):
    """a 256x144 context, slot 1 declared to hold a 200x72 picture: the picture is hashed, not the slot"""
    full = SUP.random_planes(rng, 256, 144, 10, 1)
    write(ctx, 1, full)
    assert L.vvr_slot_picture_size(ctx, 1, 200, 72) == abi.VVR_OK
    check_slot(L, ctx, 1, [full[0][:72, :200], full[1][:36, :100], full[2][:36, :100]], 10, "200x72 in 256x144")


def test_the_picture_in_the_slot_is_hashed_not_the_slot():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, 256, 144, 10, 1)
    small_picture_in_a_larger_slot(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(41))
    L.vvr_destroy(ctx)


def test_refusals_tickets_and_the_ring():
    L = SUP.stub_lib()
    rng = np.random.default_rng(42)
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    picture = film_grain_ref.grain_picture(rng, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, picture)
    digest, word = (C.c_uint8 * 48)(), C.c_uint32()

    def refused(text, **kw):
        r = abi.HashRequest()
        r.struct_size, r.slot, r.job, r.method, r.blocking, r.digest = C.sizeof(abi.HashRequest), 0, -1, abi.HASH_CRC, 1, C.addressof(digest)
        for k, v in kw.items():
            setattr(r, k, v)
        rc = L.vvr_hash_submit(ctx, C.byref(r))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(ctx) and b"vvr_hash_submit" in L.vvr_last_error(ctx), (kw, rc, L.vvr_last_error(ctx))

    refused(b"struct_size", struct_size=C.sizeof(abi.HashRequest) - 8)
    refused(b"no such slot", slot=7)
    refused(b"no such slot", slot=-1)
    refused(b"unknown method", method=3)
    refused(b"job must be", job=-2)
    refused(b"neither digest nor expected", digest=None)
    refused(b"expected without mismatch", expected=C.addressof(digest))
    refused(b"expected without mismatch", digest=None, expected=C.addressof(digest))
    # the refusals took no ring entry: eight requests of both kinds in flight, the ninth of either kind is VVR_ERR_BUSY
    want = refdrv.picture_hash(picture, 10, abi.HASH_CRC)
    flight = []
    for n in range(8):
        if n % 3 == 2:
            flight.append(("out",) + Q.submit(L, ctx, 0, (8, 4, 200, 64), "planar16", 3))
        else:
            flight.append(("hash",) + submit(L, ctx, 0, METHODS[n % 3], 3))
    assert all(t >= 2 for _, t, _ in flight) and len(set(t for _, t, _ in flight)) == 8, [t for _, t, _ in flight]
    t9, _ = submit(L, ctx, 0, abi.HASH_CRC, 3)
    assert t9 == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    t9, _ = Q.submit(L, ctx, 0, (8, 4, 200, 64), "planar16", 3)
    assert t9 == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    # vvr_sync retires nothing; vvr_output_test leaves the ticket
    assert L.vvr_sync(ctx) == abi.VVR_OK
    assert all(L.vvr_output_test(ctx, t) == abi.VVR_OK for _, t, _ in flight)
    window = Q.sync_read(L, ctx, 0, (8, 4, 200, 64), 2, 3)
    for n, (kind, t, keep) in enumerate(flight):
        if kind == "out":
            assert all(np.array_equal(a, b) for a, b in zip(Q.collect(L, ctx, t, keep), window))
        else:
            assert collect(L, ctx, t, keep)[0] == refdrv.picture_hash(picture, 10, METHODS[n % 3])
    # an unknown or retired ticket
    t = flight[0][1]
    assert L.vvr_output_wait(ctx, t) == abi.VVR_ERR_PARAMETER and b"ticket" in L.vvr_last_error(ctx)
    assert L.vvr_output_test(ctx, t) == abi.VVR_ERR_PARAMETER and L.vvr_output_wait(ctx, 12345) == abi.VVR_ERR_PARAMETER
    assert queued(L, ctx, 0, abi.HASH_CRC, 3)[0] == want
    L.vvr_destroy(ctx)


def stats_case(L, ctx, planes, bd):
    """one launch of k_hash_rows and of k_hash_combine per CRC / checksum request, none for MD5; vvr_picture_hash counts its per-plane launches as
    k_plane_hash_rows (CRC, checksum) and gives the same digests with statistics on"""
    nc = len(planes)

    def request(method):
        def run():
            assert queued(L, ctx, 0, method, nc)[0] == refdrv.picture_hash(planes, bd, method)
        return run

    def synchronous(method):
        def run():
            assert sync_hash(L, ctx, 0, method, nc) == refdrv.picture_hash(planes, bd, method)
        return run

    def verify(stats):
        assert stats.get("k_hash_rows") == 4 and stats.get("k_hash_combine") == 4 and stats.get("k_plane_hash_rows") == 2 * nc, stats
    return ([request(m) for m in (abi.HASH_CRC, abi.HASH_CHECKSUM, abi.HASH_MD5, abi.HASH_CRC, abi.HASH_CRC)] + [synchronous(m) for m in METHODS],
            verify, synchronous(abi.HASH_CRC))


def test_statistics_name_the_kernels():
    L = SUP.stub_lib()
    planes = SUP.random_planes(np.random.default_rng(5), 200, 72, 10, 1)
    ctx = SUP.make_ctx(L, 200, 72, 10, 1)
    SUP.write_picture(L, ctx, 0, planes)
    SUP.statistics("hash", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_hash_requests_leave_the_seed_chain_alone():
    """a grained planar16 request gives the same bytes before and after a run of hash requests started from the same seed: neither the chain's state
    nor the bank moved"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(43)
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, film_grain_ref.grain_picture(rng, 448, 160, 10, 1))
    bank = abi.film_grain_bank(**H._bank(rng))
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    assert L.vvr_set_film_grain_seed(ctx, 77) == abi.VVR_OK
    first = Q.queued(L, ctx, 0, (0, 0, 448, 160), "planar16", 3, grain=True)
    second = Q.queued(L, ctx, 0, (0, 0, 448, 160), "planar16", 3, grain=True)
    assert any(not np.array_equal(a, b) for a, b in zip(first, second)), "the chain advances from frame to frame"
    assert L.vvr_set_film_grain_seed(ctx, 77) == abi.VVR_OK
    again = Q.queued(L, ctx, 0, (0, 0, 448, 160), "planar16", 3, grain=True)
    for method in METHODS * 2:
        queued(L, ctx, 0, method, 3)
    after = Q.queued(L, ctx, 0, (0, 0, 448, 160), "planar16", 3, grain=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, first)) and all(np.array_equal(a, b) for a, b in zip(after, second))
    L.vvr_destroy(ctx)


def test_requests_are_ordered_on_the_device_not_on_the_host():
    """the stand-in runtime's record of stream and event operations (waits and records; it does not record synchronising calls): between entry and
    return of vvr_hash_submit the output stream waits for the picture's completion event and records the request's two events, nothing else; the
    picture that overwrites the slot afterwards waits for the first of them on its lane.  Without `blocking`, a picture still with the workers
    gives VVR_NOT_READY and the same request is accepted later."""
    L = SUP.stub_lib()
    W, H_ = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = SUP.stream_ctx(L, W, H_, nslots)
    descs = [synth.picture_for_plan(pl, W, H_, seed=611, tool_flags=T.TOOLS) for pl in plans]      # (the records live in the descriptions)
    pics = [d.c() for d in descs]
    L.vvt_set_delay(20000)
    j0 = L.vvr_submit(ctx, C.byref(pics[0]))
    assert j0 >= 0
    t, keep = submit(L, ctx, plans[0].slot, abi.HASH_CRC, 3, job=j0, blocking=False)
    assert t == abi.VVR_NOT_READY or t >= 2        # (a ticket is never VVR_NOT_READY)
    L.vvt_set_delay(0)
    if t != abi.VVR_NOT_READY:
        collect(L, ctx, t, keep)
    other = (plans[0].slot + 1) % nslots
    bad, _ = submit(L, ctx, other, abi.HASH_CRC, 3, job=j0)
    assert bad == abi.VVR_ERR_PARAMETER and b"does not reconstruct into this slot" in L.vvr_last_error(ctx)
    Q._trace(L)
    L.vvt_events_pending(1)                     # (nothing the device was given has finished: events that are complete would be dropped, not waited for)
    t, keep = submit(L, ctx, plans[0].slot, abi.HASH_CRC, 3, job=j0)        # the same request, later: accepted
    assert t >= 2 and L.vvr_output_test(ctx, t) == abi.VVR_NOT_READY
    ops = Q._trace(L)
    waits, records = [(s, e) for op, s, e in ops if op == 0], [(s, e) for op, s, e in ops if op == 1]
    out_stream = records[-1][0]
    assert len([s for s, _ in waits if s == out_stream]) == 1, "the output stream waits for the picture's event and for nothing else"
    assert len([s for s, _ in records if s == out_stream]) == 2, "the request's read and done events, on the output stream"
    read_event = [e for s, e in records if s == out_stream][0]      # behind the kernels, before the copy
    again = synth.picture_for_plan(plans[0], W, H_, seed=612, tool_flags=T.TOOLS)
    pa = again.c()
    j1 = L.vvr_submit(ctx, C.byref(pa))         # a second picture into the same slot: its lane waits for the request's read event
    assert j1 >= 0
    ext = C.c_void_p()
    L.hipStreamCreateWithFlags(C.byref(ext), 0)
    assert L.vvr_stream_wait_job(ctx, j1, ext, 1) == abi.VVR_OK      # (handed to the device)
    ops = Q._trace(L)
    assert any(op == 0 and e == read_event and s != out_stream for op, s, e in ops), "the picture that overwrites the slot did not wait for the request's event"
    L.vvt_events_pending(0)
    collect(L, ctx, t, keep)
    late, _ = submit(L, ctx, plans[0].slot, abi.HASH_CRC, 3, job=j0)
    assert late == abi.VVR_ERR_PARAMETER and b"overwrites the slot" in L.vvr_last_error(ctx)
    assert L.vvr_sync(ctx) == abi.VVR_OK
    L.vvr_destroy(ctx)


def test_not_ready_while_the_picture_is_with_its_worker():
    """the host stage of a B picture is held for 0.3 s on its worker thread (the stand-in runtime's switch): a request without `blocking` made at
    once must come back VVR_NOT_READY, takes no ring entry, and the same request with `blocking` is accepted and delivers"""
    L = SUP.stub_lib()
    W, H_ = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = SUP.stream_ctx(L, W, H_, nslots)
    descs = [synth.picture_for_plan(pl, W, H_, seed=611, tool_flags=T.TOOLS) for pl in plans[:2]]
    pics = [d.c() for d in descs]
    assert plans[1].slice_type != abi.SLICE_I
    assert L.vvr_submit(ctx, C.byref(pics[0])) >= 0
    L.vvt_slow_b_pictures(300000)
    try:
        j1 = L.vvr_submit(ctx, C.byref(pics[1]))
        assert j1 >= 0
        for method in METHODS:
            t, _ = submit(L, ctx, plans[1].slot, method, 3, job=j1, blocking=False)
            assert t == abi.VVR_NOT_READY, (method, t, L.vvr_last_error(ctx))
        t, _ = submit(L, ctx, plans[1].slot, abi.HASH_CRC, 3, blocking=False)       # job -1: pictures are still with the workers
        assert t == abi.VVR_NOT_READY
        flight = [submit(L, ctx, plans[1].slot, abi.HASH_CRC, 3, job=j1) for _ in range(8)]       # (no entry was lost to the attempts above)
    finally:
        L.vvt_slow_b_pictures(0)
    assert all(t >= 2 for t, _ in flight), [t for t, _ in flight]
    got = [collect(L, ctx, t, keep)[0] for t, keep in flight]
    assert all(g == got[0] for g in got) and got[0] == sync_hash(L, ctx, plans[1].slot, abi.HASH_CRC, 3)
    L.vvr_destroy(ctx)


def test_a_failed_picture_fails_its_request():
    SUP.a_failed_picture_fails_its_request("hash", SUP.stub_lib())


def ring_request(L, ctx, planes, win, part, ref, bd):
    def finish(t, keep, what):
        assert collect(L, ctx, t, keep)[0] == refdrv.picture_hash(planes, bd, abi.HASH_CRC), what
    return lambda: submit(L, ctx, 0, abi.HASH_CRC, len(planes)), finish


def failing(L, ctx, slot, win, job, ref_slot):
    """the checksum with digests to verify against; asked again: MD5"""
    if ref_slot is not None:
        return submit(L, ctx, slot, abi.HASH_MD5, 3, job=job)
    return submit(L, ctx, slot, abi.HASH_CHECKSUM, 3, job=job, expected=[b"\0" * 4] * 3)


def untouched(keep):
    return (keep[1] is None or keep[1].value == 0xaaaaaaaa) and bytes(keep[0]) == b"\xaa" * len(keep[0])


def delivered(keep):
    assert bytes(keep[0]) != b"\xaa" * len(keep[0]) and keep[1].value != 0xaaaaaaaa, "neither digest nor mismatch"


SUP.register("hash", b"vvr_hash_submit", ring_request, stats=stats_case, failing=failing, untouched=untouched, delivered=delivered)
