"""GPU: the four measures of the output queue against a reference of another size than the window (vvr_set_compare_scaling) on the device:
k_rescale into the request's ring entry, then the measure's kernels.  The cases of tests/test_output_scaled_compare_host.py; a reference in torch
tensors on the device; two picture sizes in one context against one reference (the RPR case); a scaled comparison directly behind vvr_submit
of a small stream (ordered on the device: nothing here depends on timing); eight requests in flight that mix scaled and unscaled kinds; one
comparison at 1080p to 4K and one 8x down.  The picture side is what vvr_read_output_scaled delivers (tests/test_gpu_output_rescale.py pins it
against vvdec::rescalePlane); every comparison is exact."""
import numpy as np
import pytest

import compare_ref
import output_support as SUP
import rescale_ref
import ssim_ref
import test_output_compare_host as XC
import test_output_queue_host as Q
import test_output_scaled_compare_host as S
import test_output_ssim_host as XS
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 1), (8, 0), (10, 0)])
def test_every_content_at_every_case_on_the_device(built, bd, cf):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(cf), bd, cf, 2000 + bd + cf)
    S.check_comparison(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_collocated_reaches_the_chroma_planes(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2010)
    S.check_collocated(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_ssim_msssim_and_xpsnr_of_the_rescaled_window(built, bd):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), bd, 1, 2020 + bd)
    S.check_windowed_measures(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_a_request_keeps_the_value_it_was_submitted_with(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2030)
    fresh, _ = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2030)
    S.check_capture_at_submit(L, ctx, fresh, planes, 10)
    L.vvr_destroy(ctx)
    L.vvr_destroy(fresh)


def test_the_homes_of_a_reference_of_the_scaled_size(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 8, 1, 2040)
    S.check_homes(L, ctx, planes, 8)
    L.vvr_destroy(ctx)


def test_the_setter_refuses_and_keeps_the_value_set_before(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2050)
    S.check_setter_refusals(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_refusals_at_submit_leave_the_ring_alone(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2060)
    S.check_submit_refusals(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_statistics_name_the_rescaling(built):
    L = SUP.product_lib()
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), 10, 1, 2070)
    S.check_statistics(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_a_reference_in_torch_tensors_is_read_in_place(built):
    """Reconstructor.set_compare_scaling, then compare / ssim / msssim / xpsnr with tensors on the device
    (tests/scaled_compare_on_the_device.py, a process of its own: torch brings its own HIP runtime, which has to be the first one the process
    initialises)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "scaled_compare_on_the_device.py")], capture_output=True, text=True, timeout=120)
    assert "ok tensors" in r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def test_two_picture_sizes_in_one_context_against_one_reference(built):
    """the RPR case: slot 0 holds a picture of 208 x 80, slot 1 one of 104 x 40 (vvr_slot_picture_size); both are measured against the same
    reference of 208 x 80 - comparison and SSIM"""
    L = SUP.product_lib()
    bd = 10
    ctx, full = SUP.ctx_with(L, S.picture_size(1), bd, 1, 2090)
    small = SUP.random_planes(np.random.default_rng(2091), 104, 40, bd, 1)
    assert L.vvr_slot_picture_size(ctx, 1, 104, 40) == abi.VVR_OK
    SUP.write_picture(L, ctx, 1, small)
    size = (208, 80)
    ref = [np.random.default_rng(2092 + c).integers(0, 1 << bd, p.shape, dtype=np.int64) for c, p in enumerate(full)]
    given = SUP.forms(ref)[0][1]
    S.scaling(L, ctx, size)
    for slot, win in ((0, (0, 0, 208, 80)), (1, (0, 0, 104, 40))):
        part = S.rescaled(L, ctx, slot, win, size, 1, 3)
        XC.same(S.queued(L, ctx, S.submit_compare(L, ctx, slot, win, size, given)), compare_ref.compare(part, ref), S.as_window(size), bd, "slot %d" % slot)
        XS.same(S.queued(L, ctx, S.submit_ssim(L, ctx, slot, win, size, given)), ssim_ref.ssim(part, ref, bd), S.as_window(size), bd, "SSIM, slot %d" % slot)
    # (beyond the small picture, inside the slot: the window is validated against the picture)
    rc = S.submit_compare(L, ctx, 1, (0, 0, 208, 80), size, given)[0]
    assert rc == abi.VVR_ERR_PARAMETER and b"outside the picture" in L.vvr_last_error(ctx)
    L.vvr_destroy(ctx)


GEO = dict(bit_depth=10, chroma_format=1, log2_ctu=6)
TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_PROF |
         abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE)
MIX = dict(p_intra=0.15, p_bi=0.6, p_affine=0.15, p_geo=0.05, p_sbtmvp=0.1, p_cclm=0.2, p_jccr=0.1)


def test_pictures_of_a_stream_in_flight_are_measured_at_another_size(built):
    """a fixed-seed stream of five pictures, 256 x 128, with the smallest DPB: the last picture overwrites the slot of the first.  Directly
    behind every vvr_submit, with `job` set and no wait in between: the picture, rescaled to 384 x 192, compared with a reference of zeros of
    that size (sad is then the sum of the rescaled samples).  The picture that reuses a slot is ordered behind the rescaling that reads it on
    the device.  Expected: the CPU oracle's planes written into a second context and read back rescaled"""
    import refdrv
    import vvdec_amd
    Wd, Hd = 256, 128
    win, size = (0, 0, Wd, Hd), (384, 192)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    assert plans[-1].slot == plans[0].slot, "a slot has to be reused"
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **GEO)
    L = rec.L
    aux = SUP.make_ctx(L, Wd, Hd, 10, 1)
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4715, tool_flags=TOOLS, alloc=rec.host_array, **GEO, **MIX) for pl in plans]
    zeros = [np.zeros((size[1] >> s, size[0] >> s), np.uint16) for s in (0, 1, 1)]
    cpu, want = {}, []
    for pl, d in zip(plans, descs):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        SUP.write_picture(L, aux, 0, cpu[pl.slot])
        want.append(compare_ref.compare(S.rescaled(L, aux, 0, win, size, 1, 3), zeros))
        assert want[-1]["differing"][0] > 0
    rec.set_compare_scaling(size)
    flight = []
    for pl, d in zip(plans, descs):
        job = rec.decompress_picture(d)
        sub = S.submit_compare(L, rec.ctx, pl.slot, win, size, zeros, job=job)
        assert sub[0] >= 2, L.vvr_last_error(rec.ctx)
        flight.append(sub)
    got = [S.queued(L, rec.ctx, sub) for sub in flight]
    rec.sync()
    for k, (g, w_) in enumerate(zip(got, want)):
        XC.same(g, w_, S.as_window(size), 10, "picture %d of the stream" % k)
    L.vvr_destroy(aux)
    rec.close()


def test_eight_requests_of_scaled_and_unscaled_kinds_in_flight(built):
    L = SUP.product_lib()
    bd = 10
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), bd, 1, 2100)
    name, win, size = S.LADDER
    rng = np.random.default_rng(2101)
    S.scaling(L, ctx, size)
    part = S.rescaled(L, ctx, 0, win, size, 1, 3)
    ref = XC.reference("random", rng, part, bd)
    given = SUP.forms(ref)[0][1]
    plain = compare_ref.window_planes(planes, win)
    plain_ref = XC.reference("random", rng, plain, bd)
    plain_given = SUP.forms(plain_ref)[0][1]
    flight = []
    for n in range(8):
        if n % 4 == 0:
            S.scaling(L, ctx, size)
            flight.append(("scaled compare", S.submit_compare(L, ctx, 0, win, size, given)))
        elif n % 4 == 1:
            S.off(L, ctx)
            flight.append(("compare", XC.submit(L, ctx, 0, win, plain_given)))
        elif n % 4 == 2:
            S.scaling(L, ctx, size)
            flight.append(("scaled ssim", S.submit_ssim(L, ctx, 0, win, size, given)))
        else:
            flight.append(("out", Q.submit(L, ctx, 0, win, "planar16", 3)))      # (an output request does not look at the scaling)
    assert all(sub[0] >= 2 for _, sub in flight) and len(set(sub[0] for _, sub in flight)) == 8
    assert S.submit_compare(L, ctx, 0, win, size, given)[0] == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx)
    for n, (kind, sub) in enumerate(flight):
        what = "request %d of eight, %s" % (n, kind)
        if kind == "scaled compare":
            XC.same(S.queued(L, ctx, sub), compare_ref.compare(part, ref), S.as_window(size), bd, what)
        elif kind == "compare":
            XC.same(S.queued(L, ctx, sub), compare_ref.compare(plain, plain_ref), win, bd, what)
        elif kind == "scaled ssim":
            XS.same(S.queued(L, ctx, sub), ssim_ref.ssim(part, ref, bd), S.as_window(size), bd, what)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(Q.collect(L, ctx, sub[0], sub[1]), plain)), what
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("what,pic,size", [("1080p to 4K", (1920, 1080), (3840, 2160)), ("8x down", (1024, 512), (128, 64))])
def test_one_comparison_at_a_large_size(built, what, pic, size):
    """the comparison alone: `random` content, with a map"""
    L = SUP.product_lib()
    bd = 10
    ctx, planes = SUP.ctx_with(L, pic, bd, 1, 2110)
    win = (0, 0, pic[0], pic[1])
    S.scaling(L, ctx, size)
    part = S.rescaled(L, ctx, 0, win, size, 1, 3)
    ref = XC.reference("random", np.random.default_rng(2111), part, bd)
    want = compare_ref.compare(part, ref)
    assert want["map"].shape == ((size[1] + 63) // 64, (size[0] + 63) // 64) and all(want["differing"])
    XC.same(S.queued(L, ctx, S.submit_compare(L, ctx, 0, win, size, S.words16(ref))), want, S.as_window(size), bd, what)
    L.vvr_destroy(ctx)


@pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs the reference at build time)")
def test_the_picture_side_is_rescale_plane(built, tmp_path):
    """the picture side straight from vvdec::rescalePlane: the comparison of every case against it reports nothing differing"""
    import vvdec_amd
    L = SUP.product_lib()
    bd = 10
    ctx, planes = SUP.ctx_with(L, S.picture_size(1), bd, 1, 2080)
    cases_ = []
    for name, win, size in S.CASES:
        for c in range(3):
            s = 1 if c else 0
            x, y, w, h = (v >> s for v in win)
            cases_.append((planes[c][y:y + h, x:x + w], size[0] >> s, size[1] >> s, c, 1, bd, 1, 0))
    want = rescale_ref.rescale(cases_, vvdec_amd._LIBPATH, False, str(tmp_path))
    for n, (name, win, size) in enumerate(S.CASES):
        part = [np.ascontiguousarray(p, np.uint16) for p in want[3 * n:3 * n + 3]]
        S.scaling(L, ctx, size, 1)
        XC.same(S.queued(L, ctx, S.submit_compare(L, ctx, 0, win, size, part)), compare_ref.compare(part, part), S.as_window(size), bd, name + ": rescalePlane's frame")
    L.vvr_destroy(ctx)
