"""GPU: a picture compared with a reference frame through the output queue on the device (k_output_compare, k_output_compare_sum).  The cases of
tests/test_output_compare_host.py - windows x contents x forms of the reference - a reference in torch tensors on the device, a second slot as
the reference across two reconstructed pictures of a small stream, a request directly behind vvr_submit (ordered on the device: nothing here
depends on timing) and eight requests of mixed kinds in flight.  Expected values are tests/compare_ref.py's; every comparison is exact."""
import numpy as np
import pytest

import compare_ref
import output_support as SUP
import test_output_compare_host as X
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_window_on_the_device(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1200 + bd + cf)
    X.check_contents(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_sums_that_need_64_bits(built, bd, cf):
    L = SUP.product_lib()
    ctx, _ = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1210)
    X.check_all_ones_reference(L, ctx, SUP.writer(L), 3 if cf else 1, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_differences_just_outside_the_window_are_not_reported(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1220)
    X.check_outside(L, ctx, SUP.writer(L), planes, bd)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 0)])
def test_a_second_slot_as_the_reference(built, bd, cf):
    L = SUP.product_lib()
    ctx, a = SUP.ctx_with(L, X.picture_size(cf), bd, cf, 1230)
    b = [np.where(np.random.default_rng(1231 + c).random(p.shape) < 0.3, p ^ 5, p).astype(np.uint16) for c, p in enumerate(a)]
    SUP.check_ref_slot("compare", L, ctx, SUP.writer(L), a, b, bd)
    L.vvr_destroy(ctx)


def test_a_reference_in_memory_of_vvr_host_alloc(built):
    """copied to the device straight from the caller's pinned planes, at their stride, on the output stream"""
    import ctypes as C
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1250)
    rng = np.random.default_rng(1251)
    for win in X.WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps, dt in ((2, np.uint16), (1, np.uint8)):
            ref = X.reference("random", rng, part, 10, bps)
            given = []
            for c, p in enumerate(ref):
                stride = p.shape[1] + (3, 5, 7)[c]
                base = L.vvr_host_alloc(ctx, p.shape[0] * stride * bps)
                assert base
                a = np.frombuffer((C.c_char * (p.shape[0] * stride * bps)).from_address(base), dt).reshape(p.shape[0], stride)
                a[...] = 0x44
                a[:, :p.shape[1]] = p
                given.append(a[:, :p.shape[1]])
            X.same(X.queued(L, ctx, 0, win, given), compare_ref.compare(part, ref), win, 10, "vvr_host_alloc, window %r, %d bytes per sample" % (win, bps))
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_the_other_kinds_of_request(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1260)
    SUP.tickets_and_the_ring("compare", L, ctx, planes, 10, None)      # (vvr_output_stream_wait on the null stream)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernels(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, X.picture_size(1), 10, 1, 1261)
    SUP.statistics("compare", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_a_reference_in_torch_tensors_is_read_in_place(built):
    """Reconstructor.compare with tensors on the device (tests/compare_on_the_device.py, a process of its own: torch brings its own HIP runtime,
    which has to be the first one the process initialises) - 16-bit and 8-bit, rows padded, planes starting at an even and at an odd column, so
    that both the wide and the sample-by-sample class read the caller's memory: registered for the call, exact, and with kernel statistics on
    the two kernels are all that ran - nothing was staged or copied by a kernel.  psnr() of the result is the formula in numpy"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "compare_on_the_device.py")], capture_output=True, text=True, timeout=120)
    assert "ok tensors" in r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


GEO = dict(bit_depth=10, chroma_format=1, log2_ctu=6)
TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_PROF |
         abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE)
MIX = dict(p_intra=0.15, p_bi=0.6, p_affine=0.15, p_geo=0.05, p_sbtmvp=0.1, p_cclm=0.2, p_jccr=0.1)


def test_pictures_of_a_stream_in_flight_are_compared(built):
    """a fixed-seed stream of five pictures, 256x128, with the smallest DPB: the last picture overwrites the slot of the first.  Directly behind
    every vvr_submit, with `job` set and no wait in between: the picture against a reference of zeros (sad is then the sum of its samples) and,
    from the second picture on, against the slot of the picture before it.  At most eight requests outstanding; the picture that reuses a slot
    is ordered behind the requests that read it - as `slot` and as `ref_slot` - on the device.  Expected: numpy on the CPU oracle's planes"""
    import refdrv
    import vvdec_amd
    Wd, Hd = 256, 128
    win = (0, 0, Wd, Hd)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    assert plans[-1].slot == plans[0].slot, "a slot has to be reused"
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **GEO)
    L = rec.L
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4714, tool_flags=TOOLS, alloc=rec.host_array, **GEO, **MIX) for pl in plans]
    zeros = [np.zeros((Hd >> s, Wd >> s), np.uint16) for s in (0, 1, 1)]
    cpu, want = {}, []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        before = cpu.get(plans[n - 1].slot) if n else None
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        want.append(compare_ref.compare(cpu[pl.slot], zeros))
        if n:
            want.append(compare_ref.compare(cpu[pl.slot], before))
        assert all(w["differing"][0] > 0 for w in want[-2:])
    pending, got = [], []
    for n, (pl, d) in enumerate(zip(plans, descs)):
        job = rec.decompress_picture(d)
        for ref in [zeros] + ([plans[n - 1].slot] if n else []):
            t, keep = X.submit(L, rec.ctx, pl.slot, win, ref, job=job)
            assert t >= 2, L.vvr_last_error(rec.ctx)
            pending.append((t, keep))
            if len(pending) == 8:
                got.append(X.collect(L, rec.ctx, *pending.pop(0)))
    got += [X.collect(L, rec.ctx, t, keep) for t, keep in pending]
    rec.sync()
    assert len(got) == len(want) == 9
    for k, (g, w_) in enumerate(zip(got, want)):
        X.same(g, w_, win, 10, "request %d of the stream" % k)
    # ... and numpy on the planes read back, for the pairs of pictures that are both still in their slots (all but the first picture)
    back = {pl.slot: rec.read_picture(pl.slot) for pl in plans[1:]}
    for n in range(2, len(plans)):
        X.same(got[2 * n], compare_ref.compare(back[plans[n].slot], back[plans[n - 1].slot]), win, 10, "POC %d against the picture before it, read back" % plans[n].poc)
    rec.close()
