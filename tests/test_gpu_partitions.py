"""GPU parity at the ends of the picture partitioning (run with -m gpu): the cases of tests/partition_cases.py - tiles of one CTU and a last column 8 samples
wide, 20 tile columns, raster-scan slices that start in the middle of a tile row (the ALF corner padding), rectangular slices inside tiles beside a slice of
several tiles, 256 slices with headers of their own, virtual boundaries at 8 and size - 8, on tile edges, beside a CTU's bottom edge and three at the smallest
spacing, sub-pictures of one CTU whose vectors leave them - through the C ABI, one small picture per case, bit-exact against the CPU oracle, once with the
description's edge tables and once with the edge parameters derived on the device.  tests/test_oracle_vs_ref_partitions.py pins the same inputs against the
reference classes on the CPU, so a mismatch here is a kernel's or the host glue's.  Every case asserts, from the description's records and the oracle's
stage outputs (never from what the GPU returned), that the picture holds what the case is about."""
import numpy as np
import pytest

import limits_cases as lc
import partition_cases as pc
from vvdec_amd import synth
from test_gpu_parity import _run_stream
from test_gpu_limits import _through_the_back_end

pytestmark = pytest.mark.gpu


def _equal(case, got, dmvr, st):
    want = st(0)
    for c in range(len(want)):
        g = got[c][:want[c].shape[0], :want[c].shape[1]]
        assert np.array_equal(g, want[c]), "%s comp %d: %d samples differ" % (case.id, c, int((g != want[c]).sum()))
    if st.dmvr is not None:
        assert np.array_equal(dmvr, st.dmvr), "%s: DMVR delta MVs differ" % case.id


@pytest.mark.parametrize("case", pc.PARTITION_CASES, ids=[c.id for c in pc.PARTITION_CASES])
def test_partitions_bit_exact(built, case):
    d, refs = case.make()
    st = lc.Stages(d, refs)
    st(0)
    case.present(case, d, refs, st)
    got, dmvr = _through_the_back_end(d, refs, case.l2)
    _equal(case, got, dmvr, st)


@pytest.mark.parametrize("case", pc.PARTITION_CASES, ids=[c.id for c in pc.PARTITION_CASES])
def test_partitions_edge_parameters_derived_on_the_device(built, case):
    """once more with VVR_TOOL_LFP_ON_DEVICE: k_lf_maps / k_lf_init derive the edge parameters from the CU records and these slice / tile / sub-picture maps and
    boundary positions themselves"""
    d, refs = case.make()
    st = lc.Stages(d, refs)
    st(0)
    got, dmvr = _through_the_back_end(d, refs, case.l2, lfp_on_device=True)
    _equal(case, got, dmvr, st)


@pytest.mark.parametrize("name,W,H,l2,seed,tools,kw,vary", pc.STREAMS, ids=[s[0] for s in pc.STREAMS])
def test_partition_streams_in_flight(built, name, W, H, l2, seed, tools, kw, vary):
    """five pictures through the path a decoder uses - worker threads that build the work lists in bands, three streams, everything submitted before the first
    wait, the intra stage ordering blocks across tile edges - then picture by picture against the oracle, and pipelined against serial (_run_stream)"""
    post = (lambda d: synth.vary_slices(d, seed + d.hdr.poc)) if vary else None
    _run_stream(W, H, 5, 4, seed, tools, streams=3, log2_ctu=l2, intra=True, post=post, **dict(pc.STREAM_MIX, **kw))
