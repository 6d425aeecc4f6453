"""GPU: decoded picture hashes through the output queue on the device (k_hash_rows, k_hash_combine; MD5 through k_output_window).  The case matrix
of tests/test_output_hash_host.py, one 3840x2160 frame, a random-access GOP whose pictures are verified while the stream is in flight and its
slots are reused (ordered on the device: nothing here depends on timing), and the kernels' statistics."""
import ctypes as C

import numpy as np
import pytest

import output_support as SUP
import refdrv
import test_output_hash_host as X
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W,H_,cf,bd", X.SHAPES)
def test_matrix_on_the_device(built, W, H_, cf, bd):
    L = SUP.product_lib()
    planes = SUP.random_planes(np.random.default_rng(W + H_ + bd), W, H_, bd, cf)
    ctx = SUP.make_ctx(L, W, H_, bd, cf)
    SUP.write_picture(L, ctx, 1, planes)
    X.check_slot(L, ctx, 1, planes, bd, "%dx%d" % (W, H_))
    L.vvr_destroy(ctx)


def test_the_picture_in_the_slot_is_hashed_not_the_slot(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, 256, 144, 10, 1)
    X.small_picture_in_a_larger_slot(L, ctx, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(41))
    L.vvr_destroy(ctx)


def test_a_3840x2160_frame(built):
    """uploaded, not decoded; the three methods.  MD5 and checksum against refdrv.picture_hash; the CRC against refdrv's CRC as numpy computes it row
    by row (test_output_hash_host.crc_by_rows, pinned to refdrv.hash_crc there: refdrv's own byte loop takes six seconds for this frame) and
    against vvr_picture_hash"""
    L = SUP.product_lib()
    W, H_, bd = 3840, 2160, 10
    planes = SUP.random_planes(np.random.default_rng(2160), W, H_, bd, 1)
    ctx = SUP.make_ctx(L, W, H_, bd, 1, slots=1)
    SUP.write_picture(L, ctx, 0, planes)
    for method in X.METHODS:
        want = [X.crc_by_rows(p, bd) for p in planes] if method == abi.HASH_CRC else refdrv.picture_hash(planes, bd, method)
        got, mask = X.queued(L, ctx, 0, method, 3, expected=want)
        assert got == want and mask == 0, "method %d: %r, expected %r" % (method, got, want)
        assert X.sync_hash(L, ctx, 0, method, 3) == want, "method %d: vvr_picture_hash" % method
    L.vvr_destroy(ctx)


GEO = dict(bit_depth=10, chroma_format=1, log2_ctu=6)
TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_PROF |
         abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE)
MIX = dict(p_intra=0.15, p_bi=0.6, p_affine=0.15, p_geo=0.05, p_sbtmvp=0.1, p_cclm=0.2, p_jccr=0.1)


def test_every_picture_of_a_stream_in_flight_is_verified(built):
    """a random-access GOP of 17 pictures, 256x128, with the smallest DPB (slots are reused while requests are in flight): a CRC request directly
    behind every vvr_submit, at most eight outstanding, no vvr_wait / vvr_sync before the last picture has been submitted.  Every digest is
    refdrv.picture_hash of the CPU oracle's planes for that picture; once more with those digests as `expected`: every mask is 0"""
    import vvdec_amd
    W, H_ = 256, 128
    plans, nslots = stream.ra_plan(17, gop=8, seed_poc0_is_external=False)
    assert len({pl.slot for pl in plans}) < len(plans), "slots have to be reused"
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=nslots, num_streams=4, host_threads=3, **GEO)
    descs = [synth.picture_for_plan(pl, W, H_, seed=4713, tool_flags=TOOLS, alloc=rec.host_array, **GEO, **MIX) for pl in plans]
    cpu, want = {}, []
    for pl, d in zip(plans, descs):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        want.append(refdrv.picture_hash(cpu[pl.slot], 10, abi.HASH_CRC))
    assert len(set(b"".join(w) for w in want)) == len(want), "the pictures differ"
    for verify in (False, True):
        pending, got = [], []
        for n, (pl, d) in enumerate(zip(plans, descs)):
            job = rec.decompress_picture(d)
            pending.append(rec.hash_submit(pl.slot, job=job, method=abi.HASH_CRC, expected=want[n] if verify else None))
            if len(pending) == 8:
                got.append(rec.hash_wait(pending.pop(0)))
        got += [rec.hash_wait(t) for t in pending]
        rec.sync()
        for n, (digests, mask) in enumerate(got):
            assert digests == want[n], "POC %d: %r, the oracle's picture has %r" % (plans[n].poc, digests, want[n])
            assert mask == (0 if verify else None), "POC %d: mask %r" % (plans[n].poc, mask)
    rec.close()


def test_statistics_name_the_kernels(built):
    """vvr_get_stats: one launch of k_hash_rows and one of k_hash_combine per CRC / checksum request, an MD5 request launches neither; the per-plane
    launches of vvr_picture_hash are counted as k_plane_hash_rows"""
    L = SUP.product_lib()
    planes = SUP.random_planes(np.random.default_rng(5), 200, 72, 10, 1)
    ctx = SUP.make_ctx(L, 200, 72, 10, 1)
    SUP.write_picture(L, ctx, 0, planes)
    SUP.statistics("hash", L, ctx, planes, 10)
    L.vvr_destroy(ctx)
