"""CPU (the host glue against the stand-in runtime of tests/hoststub): k_itrans keeps the 32 x 32 corner of a block above 32 samples - the DCT-2 zero-out - so the
record checks of vvr_prepare refuse what carries levels everywhere in such a block: transform skip and BDPCM above 32 samples (VVC: MaxTsSize <= 32)."""
import numpy as np
import pytest

from vvdec_amd import abi, synth, stream
from test_host_glue import stub, Ctx, _expect_error, TOOLS, pytestmark      # noqa: F401  (the fixture and the skip without HIP headers)


def _picture_with_a_64_wide_block(plan, W, H):
    d = synth.picture_for_plan(plan, W, H, seed=971, tool_flags=TOOLS, p_split_scale=0.3, p_coded=1.0, p_ts=0.0, p_bdpcm=0.0, p_lfnst=0.0, p_isp=0.0, p_mip=0.0)
    coded = (d.tu["cbf"] & 1) != 0
    rooted = (d.cu["flags"][d.tu["cu"]] & abi.CU_ROOT_CBF) != 0
    wide = np.nonzero(coded & rooted & ((d.tu["w"] == 64) | (d.tu["h"] == 64)))[0]
    assert len(wide), "the generator left no coded 64-wide luma block"
    return d, int(wide[0])


def test_transform_skip_and_bdpcm_above_32_samples_are_refused(stub):
    W, H = 256, 128
    plans, nslots = stream.ra_plan(1, gop=1, seed_poc0_is_external=False)
    ctx = Ctx(stub, W, H, nslots)
    d, k = _picture_with_a_64_wide_block(plans[0], W, H)
    hnd = ctx.prepare(d)                                        # as generated: accepted
    stub.vvr_free_prepared(ctx.ctx, hnd)
    d.tu["mts_idx"][k][0] = abi.MTS_SKIP
    _expect_error(ctx, d, abi.VVR_ERR_PARAMETER, "larger than 32 samples")
    d, k = _picture_with_a_64_wide_block(plans[0], W, H)
    d.cu["bdpcm"][int(d.tu["cu"][k])] = (1, 0)
    _expect_error(ctx, d, abi.VVR_ERR_PARAMETER, "larger than 32 samples")
    # at 32 samples both stay accepted
    d = synth.picture_for_plan(plans[0], W, H, seed=972, tool_flags=TOOLS, p_split_scale=0.6, p_coded=1.0, p_ts=0.8, p_bdpcm=0.3)
    ts32 = ((d.tu["mts_idx"][:, 0] == abi.MTS_SKIP) & ((d.tu["cbf"] & 1) != 0) & (np.maximum(d.tu["w"], d.tu["h"]) == 32)).sum()
    assert ts32 > 0
    hnd = ctx.prepare(d)
    stub.vvr_free_prepared(ctx.ctx, hnd)
    ctx.close()
