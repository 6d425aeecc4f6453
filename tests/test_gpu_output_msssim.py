"""GPU: MS-SSIM of a picture against a reference frame through the output queue on the device (k_output_msssim per scale, k_output_msssim_sum).
The cases of tests/test_output_msssim_host.py - windows x contents x forms of the reference, which between them hold a dropped odd column,
partial cells at two levels, levels smaller than one block, a halo across a block border of level 1, the never-read tail of consequence (b) and
the last covered sample of the last level - a reference in memory of vvr_host_alloc, in torch tensors on the device, a second slot as the
reference, requests directly behind vvr_submit across the pictures of a small stream (ordered on the device: nothing here depends on timing)
and eight requests of mixed kinds in flight.  Expected values are tests/msssim_ref.py's; every comparison is exact."""
import numpy as np
import pytest

import compare_ref
import msssim_ref
import output_support as SUP
import test_gpu_output_compare as G
import test_output_msssim_host as X
from vvdec_amd import stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window_on_the_device(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1530 + bd + cf)
    X.check_contents(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_slot_holding_words_above_the_bit_depth_is_clamped(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1540)
    X.check_words_above_the_bit_depth(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference(built, bd, cf):
    L = SUP.product_lib()
    ctx, a = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1550)
    SUP.check_ref_slot("msssim", L, ctx, SUP.writer(L), a, SUP.noisy(a, bd, 1551), bd)
    L.vvr_destroy(ctx)


def test_a_reference_in_memory_of_vvr_host_alloc(built):
    """copied to the device straight from the caller's pinned planes, at their padded stride, on the output stream"""
    import ctypes as C
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1555)
    rng = np.random.default_rng(1556)
    for win, scales in X.CASES:
        part = compare_ref.window_planes(planes, win)
        for bps, dt in ((2, np.uint16), (1, np.uint8)):
            ref = [rng.integers(0, 1 << (8 * bps), p.shape, dtype=np.int64) for p in part]
            given = []
            for c, p in enumerate(ref):
                stride = p.shape[1] + (3, 5, 7)[c]
                base = L.vvr_host_alloc(ctx, p.shape[0] * stride * bps)
                assert base
                a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                a[...] = 0x44
                a[:, :p.shape[1]] = p
                given.append(a[:, :p.shape[1]])
            X.same(X.queued(L, ctx, 0, win, given, scales), msssim_ref.msssim(part, ref, 10, scales), win, 10, "vvr_host_alloc, window %r, %d bytes per sample" % (win, bps))
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1560)
    SUP.tickets_and_the_ring("msssim", L, ctx, planes, 10, None)      # (vvr_output_stream_wait on the null stream)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernels(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1561)
    SUP.statistics("msssim", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_a_reference_in_torch_tensors_is_read_in_place(built):
    """Reconstructor.msssim with tensors on the device (tests/msssim_on_the_device.py, a process of its own: torch brings its own HIP runtime,
    which has to be the first one the process initialises) - 16-bit and 8-bit, rows padded, planes starting at an even and at an odd column, so
    that both the wide and the sample-by-sample class read the caller's memory at level 0: registered for the call, exact, and with kernel
    statistics on k_output_msssim and k_output_msssim_sum are all that ran - nothing was staged or copied by a kernel"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "msssim_on_the_device.py")], capture_output=True, text=True, timeout=120)
    assert "ok tensors" in r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def test_msssim_of_the_pictures_of_a_stream_in_flight(built):
    """the fixed-seed stream of five pictures, 256x128, of test_ssim_of_the_pictures_of_a_stream_in_flight, with the smallest DPB: the last
    picture overwrites the slot of the first.  Directly behind every vvr_submit from the second on, with `job` set and no wait in between:
    MS-SSIM over four scales (luma 256, 128, 64, 32 by 128, 64, 32, 16; chroma ends at 16 x 8) of the picture against the slot of the picture
    before it.  The picture that reuses a slot is ordered behind the request that reads it as `ref_slot` on the device.  Expected:
    tests/msssim_ref.py on the CPU oracle's planes"""
    import refdrv
    import vvdec_amd
    Wd, Hd, scales = 256, 128, 4
    win = (0, 0, Wd, Hd)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    assert plans[-1].slot == plans[0].slot, "a slot has to be reused"
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **G.GEO)
    L = rec.L
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4714, tool_flags=G.TOOLS, alloc=rec.host_array, **G.GEO, **G.MIX) for pl in plans]
    cpu, want = {}, []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        before = cpu.get(plans[n - 1].slot) if n else None
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        if n:
            want.append(msssim_ref.msssim(cpu[pl.slot], before, 10, scales))
            assert want[-1]["windows"][3] == [7 * 3, 3, 3] and want[-1]["width"][3] == [32, 16, 16] and want[-1]["sum_v"][0][0] < (63 * 31) << 24
    pending = []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        job = rec.decompress_picture(d)
        if n:
            t, keep = X.submit(L, rec.ctx, pl.slot, win, plans[n - 1].slot, scales, job=job)
            assert t >= 2, L.vvr_last_error(rec.ctx)
            pending.append((t, keep))
    got = [X.collect(L, rec.ctx, t, keep) for t, keep in pending]
    rec.sync()
    assert len(got) == len(want) == 4
    for k, (g, w_) in enumerate(zip(got, want)):
        X.same(g, w_, win, 10, "request %d of the stream" % k)
    rec.close()
