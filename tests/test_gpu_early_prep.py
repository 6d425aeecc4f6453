"""The front half of a picture - k_prep and k_lf_init, which work from the picture's own uploaded records - is launched in front of the waits for the
picture's references and slot hazards (enqueuePicture, vvdec_amd/csrc/vvr_api.cpp).  It writes tables of the ring entry / the prepared picture and the
lane's cell maps; nothing it writes may be in use by a picture still in flight, whatever the pictures wait for."""
import numpy as np
import pytest

import refdrv
from vvdec_amd import abi, synth, stream

pytestmark = pytest.mark.gpu

TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_PROF |
         abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE)
MIX = dict(p_intra=0.15, p_bi=0.6, p_affine=0.15, p_geo=0.05, p_sbtmvp=0.1, p_cclm=0.2, p_jccr=0.1)


@pytest.mark.parametrize("W,H,l2", [(256, 128, 6), (384, 256, 7)])
def test_stream_in_flight_equals_one_picture_at_a_time(built, W, H, l2):
    """hierarchical-B stream of 17 pictures (GOP 8) on four lanes with the smallest DPB (a freed slot is reused at once: write-after-read waits), edge
    parameters and affine vectors left to the device, LMCS with chroma scaling, DMVR, 15 % intra CUs (k_intra_leaf and its cell maps): every plane of
    every picture, read through the output queue while the stream is in flight, equals the same stream submitted one picture at a time with a wait
    after each - and that one equals the CPU oracle"""
    import vvdec_amd
    plans, nslots = stream.ra_plan(17, gop=8, seed_poc0_is_external=False)              # pool = 0: the minimum number of slots
    assert len({pl.slot for pl in plans}) < len(plans), "slots have to be reused for write-after-read waits to occur"
    rec = vvdec_amd.Reconstructor(W, H, num_slots=nslots, num_streams=4, host_threads=3, log2_ctu=l2)
    descs = [synth.picture_for_plan(pl, W, H, seed=4711, tool_flags=TOOLS, alloc=rec.host_array, log2_ctu=l2, **MIX) for pl in plans]
    assert any(np.any(d.cu["pred_mode"] == abi.PRED_INTRA) and np.any(d.cu["pred_mode"] == abi.PRED_INTER) for d in descs[1:]), "B pictures with intra CUs wanted"
    assert any(getattr(d, "num_dmvr", 0) for d in descs), "DMVR CUs wanted"
    # ---- in flight: a picture's planes are asked for behind its job (the next writer of the slot waits for the request on the device)
    flight, pending = [], []
    for pl, d in zip(plans, descs):
        job = rec.decompress_picture(d)
        pending.append(rec.output_submit(pl.slot, job=job))
        if len(pending) == 6:
            flight.append([p.copy() for p in rec.output_wait(pending.pop(0))])
    while pending:
        flight.append([p.copy() for p in rec.output_wait(pending.pop(0))])
    rec.sync()
    # ---- one at a time, against the oracle (the records live in pinned memory of `rec`: it is closed at the end)
    rec2 = vvdec_amd.Reconstructor(W, H, num_slots=nslots, num_streams=4, log2_ctu=l2)
    cpu = {}
    for n, (pl, d) in enumerate(zip(plans, descs)):
        job = rec2.decompress_picture(d)
        rec2.wait(job)
        got = rec2.read_picture(pl.slot)
        for c in range(3):
            assert np.array_equal(flight[n][c], got[c]), "POC %d comp %d: in flight and alone differ in %d samples" % (pl.poc, c, int((flight[n][c] != got[c]).sum()))
        want = refdrv.oracle_reconstruct(d, cpu)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "POC %d comp %d: %d samples differ from the oracle" % (pl.poc, c, int((got[c] != want[c]).sum()))
        cpu[pl.slot] = want
        nd = getattr(d, "num_dmvr", 0)
        if nd:
            assert np.array_equal(rec2.read_dmvr(job, nd), refdrv.oracle_dmvr(nd)), "POC %d: DMVR delta MVs differ" % pl.poc
    rec2.close()
    rec.close()


def test_a_prepared_picture_submitted_again_while_in_flight(built):
    """vvr_submit_prepared twice back to back with the same handle, the second while the first is in flight (round-robin: on another lane): the front half
    of the second submission rewrites the handle's tables - it is ordered behind the first job.  Both leave what a single submission leaves, delta MVs
    included.  (A handle carries its output slot: both submissions write the same one.)"""
    import vvdec_amd
    W, H = 384, 256
    plans, nslots = stream.ra_plan(3, gop=2, seed_poc0_is_external=False)
    rec = vvdec_amd.Reconstructor(W, H, num_slots=nslots + 1, num_streams=4)
    descs = [synth.picture_for_plan(pl, W, H, seed=4712, tool_flags=TOOLS, **MIX) for pl in plans]
    for pl, d in zip(plans[:2], descs[:2]):            # the references: I picture and key picture
        rec.wait(rec.decompress_picture(d))
    pl, d = plans[2], descs[2]
    assert pl.slice_type != abi.SLICE_I and np.any(d.cu["pred_mode"] == abi.PRED_INTRA)
    nd = getattr(d, "num_dmvr", 0)
    assert nd
    h = rec.prepare(d)
    j = rec.submit_prepared(h)
    rec.wait(j)
    single = [p.copy() for p in rec.read_picture(pl.slot)]
    single_mv = rec.read_dmvr(j, nd).copy()
    for rnd in range(4):
        rec.write_picture(pl.slot, [np.zeros_like(p) for p in single])
        j1 = rec.submit_prepared(h)
        t1 = rec.output_submit(pl.slot, job=j1)          # (what the first submission leaves, before the second overwrites it)
        j2 = rec.submit_prepared(h)
        first = rec.output_wait(t1)
        rec.wait(j1)
        rec.wait(j2)
        second = rec.read_picture(pl.slot)
        for c in range(3):
            assert np.array_equal(first[c], single[c]), "round %d, first submission, comp %d" % (rnd, c)
            assert np.array_equal(second[c], single[c]), "round %d, second submission, comp %d" % (rnd, c)
        assert np.array_equal(rec.read_dmvr(j2, nd), single_mv)
    rec.free_prepared(h)
    rec.close()
