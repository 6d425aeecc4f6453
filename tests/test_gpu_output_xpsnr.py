"""GPU: XPSNR of a picture against a reference frame through the output queue on the device (k_output_xpsnr).  The cases of
tests/test_output_xpsnr_host.py - windows x contents x block sizes x filters x temporal x forms of the planes, which between them hold tiles
that meet one block and many, blocks off the tile grid, partial last cells, blocks without positions, references of 16-bit words, unaligned
bases and odd strides - the anchor of the definition, planes in memory of vvr_host_alloc and in registered ranges, in torch tensors on the
device, a second slot as the reference, requests directly behind vvr_submit across the pictures of a small stream (ordered on the device:
nothing here depends on timing) and eight requests of mixed kinds in flight.  Expected values are tests/xpsnr_ref.py's; every comparison of
integers is exact."""
import numpy as np
import pytest

import compare_ref
import output_support as SUP
import xpsnr_ref
import test_gpu_output_compare as G
import test_output_xpsnr_host as X
from vvdec_amd import stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window_on_the_device(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1530 + bd + cf)
    X.check_contents(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_what_follows_from_the_definition(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1540)
    X.check_consequences(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


def test_the_anchor_on_the_device(built):
    L = SUP.product_lib()
    ctx, _ = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1541)
    X.check_anchor(L, ctx, SUP.writer(L))
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference_with_prev_planes_on_the_host(built, bd, cf):
    L = SUP.product_lib()
    ctx, a = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1550)
    SUP.check_ref_slot("xpsnr", L, ctx, SUP.writer(L), a, SUP.noisy(a, bd, 1551), bd)
    L.vvr_destroy(ctx)


def test_planes_in_memory_of_vvr_host_alloc(built):
    """reference and prev planes copied to the device straight from the caller's pinned planes, at their padded strides, on the output stream;
    and prev planes in pinned memory beside a ref_slot"""
    import ctypes as C
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1555)
    other = SUP.noisy(planes, 10, 1557)
    SUP.writer(L)(ctx, 1, other)
    rng = np.random.default_rng(1556)
    for win in X.WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps, dt in ((2, np.uint16), (1, np.uint8)):
            ref, prev = X.reference("random16", rng, part, 10, 8 * bps)
            given = []
            for c, p in enumerate(ref + prev):
                stride = p.shape[1] + (3, 5, 7, 9, 11)[c]
                base = L.vvr_host_alloc(ctx, p.shape[0] * stride * bps)
                assert base
                a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                a[...] = 0x44
                a[:, :p.shape[1]] = p
                given.append(a[:, :p.shape[1]])
            what = "vvr_host_alloc, window %r, %d bytes per sample" % (win, bps)
            X.same(X.queued(L, ctx, 0, win, given[:3], given[3:], block=44, filter_=2), xpsnr_ref.xpsnr_integers(part, ref, prev, 44, 2), win, 10, what)
            if bps == 2:
                want = xpsnr_ref.xpsnr_integers(part, compare_ref.window_planes(other, win), prev, 0, 1)
                X.same(X.queued(L, ctx, 0, win, 1, given[3:], filter_=1), want, win, 10, what + ", beside a ref_slot")
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1570)
    SUP.tickets_and_the_ring("xpsnr", L, ctx, planes, 10, None)      # (vvr_output_stream_wait on the null stream)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernel(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1571)
    SUP.statistics("xpsnr", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_planes_in_torch_tensors_are_read_in_place(built):
    """Reconstructor.xpsnr with tensors on the device (tests/xpsnr_on_the_device.py, a process of its own: torch brings its own HIP runtime,
    which has to be the first one the process initialises) - 16-bit and 8-bit, rows padded, planes starting at an even and at an odd column, so
    that both the wide and the sample-by-sample class read the caller's memory: registered for the call, exact, and with kernel statistics on
    k_output_xpsnr is all that ran - nothing was staged or copied by a kernel"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "xpsnr_on_the_device.py")], capture_output=True, text=True, timeout=120)
    assert "ok tensors" in r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def test_xpsnr_of_the_pictures_of_a_stream_in_flight(built):
    """the fixed-seed stream of five pictures, 256x128, of test_ssim_of_the_pictures_of_a_stream_in_flight.  Directly behind every vvr_submit,
    with `job` set and no wait in between: XPSNR of the picture against its "source" - the CPU oracle's planes plus fixed-seed noise, held in
    host arrays - with the sources of the one or two pictures before it as prev planes.  Expected: tests/xpsnr_ref.py on the CPU oracle's
    planes"""
    import refdrv
    import vvdec_amd
    Wd, Hd = 256, 128
    win = (0, 0, Wd, Hd)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **G.GEO)
    L = rec.L
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4714, tool_flags=G.TOOLS, alloc=rec.host_array, **G.GEO, **G.MIX) for pl in plans]
    cpu, sources, want = {}, [], []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        sources.append(SUP.noisy(cpu[pl.slot], 10, 1590 + n))
        prev = [s[0] for s in sources[-2::-1][:2]]
        want.append(xpsnr_ref.xpsnr_integers(cpu[pl.slot], sources[-1], prev))
        assert (want[-1]["block"], want[-1]["filter"], want[-1]["temporal"]) == (8, 1, min(n, 2)) and want[-1]["sse"][0] > 0
    pending = []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        job = rec.decompress_picture(d)
        t, keep = X.submit(L, rec.ctx, pl.slot, win, sources[n], [s[0] for s in sources[:n][::-1][:2]], job=job)
        assert t >= 2, L.vvr_last_error(rec.ctx)
        pending.append((t, keep))
    got = [X.collect(L, rec.ctx, t, keep) for t, keep in pending]
    rec.sync()
    assert len(got) == len(want) == 5
    for k, (g, w_) in enumerate(zip(got, want)):
        X.same(g, w_, win, 10, "request %d of the stream" % k)
        rc, db = X.c_xpsnr(L, *g)
        assert rc == 0
        X.close_enough(db, xpsnr_ref.xpsnr(w_, 10), "request %d of the stream" % k)
    rec.close()
