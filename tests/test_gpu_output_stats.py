"""GPU: light-level statistics through the output queue on the device (k_output_stats, the statistics class of k_output_rgb, k_output_stats_sum).
The cases of tests/test_output_stats_host.py, one 3840x2160 frame in both modes, random and flat, and a random-access GOP whose pictures are
measured while the stream is in flight and its slots are reused (ordered on the device: nothing here depends on timing).  Expected values are
numpy's counts over tests/rgb_ref.py; every comparison is exact."""
import numpy as np
import pytest

import output_support as SUP
import refdrv
import test_output_stats_host as X
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu


def _random_ctx(L, seed, bd=10):
    planes = X.picture("random", np.random.default_rng(seed), X.W, X.H_, bd)
    ctx = SUP.make_ctx(L, X.W, X.H_, bd, 1)
    SUP.write_picture(L, ctx, 0, planes)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    return ctx, planes


@pytest.mark.parametrize("kind", X.CONTENTS)
@pytest.mark.parametrize("bd", [10, 8, 9])
def test_statistics_of_every_case_on_the_device(built, bd, kind):
    L = SUP.product_lib()
    planes = X.picture(kind, np.random.default_rng(900 + bd), X.W, X.H_, bd)
    ctx = SUP.make_ctx(L, X.W, X.H_, bd, 1)
    SUP.write_picture(L, ctx, 0, planes)
    X.check_content(L, ctx, planes, bd, kind)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_luma_mode_in_a_400_context(built, bd):
    L = SUP.product_lib()
    planes = X.picture("random", np.random.default_rng(910 + bd), X.W400, X.H400, bd, 0)
    ctx = SUP.make_ctx(L, X.W400, X.H400, bd, 0)
    SUP.write_picture(L, ctx, 0, planes)
    X.check_400(L, ctx, planes, bd)
    L.vvr_destroy(ctx)


def test_a_flat_512x256_frame_needs_32_bit_counts(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, 512, 256, 10, 1)
    X.check_flat_512x256(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p))
    L.vvr_destroy(ctx)


def test_the_picture_in_the_slot_not_the_slot(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, 256, 144, 10, 1)
    X.small_picture_in_a_larger_slot(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(920))
    L.vvr_destroy(ctx)


def test_tickets_are_shared_with_output_and_hash_requests(built):
    L = SUP.product_lib()
    ctx, planes = _random_ctx(L, 921)
    SUP.tickets_and_the_ring("stats", L, ctx, planes, 10, None)      # (vvr_output_stream_wait on the null stream)
    L.vvr_destroy(ctx)


def test_statistics_name_the_kernel(built):
    L = SUP.product_lib()
    ctx, planes = _random_ctx(L, 922)
    SUP.statistics("stats", L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_rgb_requests_around_a_statistics_request_store_the_same_bytes(built):
    L = SUP.product_lib()
    ctx, planes = _random_ctx(L, 923)
    X.rgb_requests_around_a_statistics_request(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_a_request_takes_the_colour_description_set_when_it_is_submitted(built):
    L = SUP.product_lib()
    ctx, planes = _random_ctx(L, 924)
    X.colour_snapshot(L, ctx, planes, 10)
    L.vvr_destroy(ctx)


def test_the_loop_from_statistics_to_the_lut(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, X.W, X.H_, 10, 1)
    X.loop_from_statistics_to_the_lut(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(930))
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("kind", ["random", "flat"])
def test_a_3840x2160_frame(built, kind):
    """uploaded, not decoded; both modes against numpy.  The flat frame puts 8 294 400 samples into one bin of each histogram"""
    L = SUP.product_lib()
    Wf, Hf, bd, win, col, colour = 3840, 2160, 10, (0, 0, 3840, 2160), (True, False), (9, 0)
    planes = X.picture(kind, np.random.default_rng(2160), Wf, Hf, bd)
    ctx = SUP.make_ctx(L, Wf, Hf, bd, 1, slots=1)
    SUP.write_picture(L, ctx, 0, planes)
    assert L.vvr_set_output_colour(ctx, *colour) == abi.VVR_OK
    want = X.expected(planes, bd, abi.STATS_RGB, colour, col)
    if kind == "flat":
        assert want["hist_y"].max() == Wf * Hf and want["hist_maxrgb"].max() == Wf * Hf
    X.same(X.queued(L, ctx, 0, win, abi.STATS_RGB, col=col), want, win, bd, abi.STATS_RGB, "3840x2160 %s, RGB mode" % kind)
    X.same(X.queued(L, ctx, 0, win, abi.STATS_LUMA), X.expected(planes, bd, abi.STATS_LUMA), win, bd, abi.STATS_LUMA, "3840x2160 %s, luma mode" % kind)
    L.vvr_destroy(ctx)


GEO = dict(bit_depth=10, chroma_format=1, log2_ctu=6)
TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_PROF |
         abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE)
MIX = dict(p_intra=0.15, p_bi=0.6, p_affine=0.15, p_geo=0.05, p_sbtmvp=0.1, p_cclm=0.2, p_jccr=0.1)


def test_every_picture_of_a_stream_in_flight_is_measured(built):
    """a random-access GOP of 17 pictures, 256x128, with the smallest DPB (slots are reused while requests are in flight): an RGB statistics
    request directly behind every vvr_submit, at most eight outstanding, no wait for a picture before the last has been submitted.  Every result
    is the statistics of the CPU oracle's planes for that picture; vvdec_amd.light_level of it gives the restatement's codes"""
    import vvdec_amd
    Wd, Hd, col, colour = 256, 128, (True, False), (9, 0)
    plans, nslots = stream.ra_plan(17, gop=8, seed_poc0_is_external=False)
    assert len({pl.slot for pl in plans}) < len(plans), "slots have to be reused"
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **GEO)
    rec.set_output_colour(*colour)
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4713, tool_flags=TOOLS, alloc=rec.host_array, **GEO, **MIX) for pl in plans]
    cpu, want = {}, []
    for pl, d in zip(plans, descs):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        want.append(X.expected(cpu[pl.slot], 10, abi.STATS_RGB, colour, col))
    assert len(set(w["hist_y"].tobytes() for w in want)) == len(want), "the pictures differ"
    pending, got = [], []
    for pl, d in zip(plans, descs):
        job = rec.decompress_picture(d)
        pending.append(rec.stats_submit(pl.slot, job=job, mode="rgb", collocated=col))
        if len(pending) == 8:
            got.append(rec.stats_wait(pending.pop(0)))
    got += [rec.stats_wait(t) for t in pending]
    rec.sync()
    for n, st in enumerate(got):
        X.same(st.raw, want[n], (0, 0, Wd, Hd), 10, abi.STATS_RGB, "POC %d" % plans[n].poc)
        assert np.array_equal(st.hist_maxrgb, want[n]["hist_maxrgb"]) and list(st.max_c) == want[n]["max_c"]
        ll = vvdec_amd.light_level(st, 16, 9995)
        ref = X.light_level(want[n]["hist_maxrgb"], want[n]["max_c"], 10, Wd * Hd, 16, 9995)
        X.same_light_level(ll, ref, "POC %d" % plans[n].poc)
    rec.close()
