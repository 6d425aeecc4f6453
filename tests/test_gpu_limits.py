"""GPU parity at the ends of the value ranges (run with -m gpu): the cases of tests/limits_cases.py - QPs from -QpBdOffset to 63, reference pictures that
alternate between 0 and the largest sample value, prediction weights, ALF / CC-ALF taps and deblocking offsets at the limits of their syntax, reference lists
of 16 entries, motion vectors over the 18-bit range - through the
C ABI, one small picture per case, bit-exact against the CPU oracle.  tests/test_oracle_vs_ref_limits.py pins the same inputs against the reference classes on
the CPU, so a mismatch here is a kernel's.  Every case asserts, from the description's records and the oracle's stage outputs (never from what the GPU
returned), that the picture holds what the case is about."""
import numpy as np
import pytest

import refdrv
import limits_cases as lc
from vvdec_amd import abi, synth
from test_gpu_parity import _run_stream, TOOLS_B, TOOLS_DB

pytestmark = pytest.mark.gpu


def _through_the_back_end(d, refs, l2, lfp_on_device=False):
    """the picture of a description, its reference pictures uploaded at their own sizes -> (planes, DMVR delta MVs or None)"""
    import vvdec_amd
    bd, cf = int(d.hdr.bit_depth), int(d.hdr.chroma_format)
    W, H = int(d.hdr.width), int(d.hdr.height)
    MW = max([W] + [r[0].shape[1] for r in refs.values()])
    MH = max([H] + [r[0].shape[0] for r in refs.values()])
    rec = vvdec_amd.Reconstructor(MW, MH, num_slots=max(list(refs) + [int(d.hdr.out_slot)]) + 1, num_streams=1, log2_ctu=l2, bit_depth=bd, chroma_format=cf)
    try:
        for slot, planes in refs.items():
            full = []
            for c, p in enumerate(planes):
                a = np.zeros(rec.plane_shape(c), np.uint16)
                a[:p.shape[0], :p.shape[1]] = p
                full.append(a)
            rec.write_picture(slot, full)
        if lfp_on_device:
            d.hdr.tool_flags |= abi.TOOL_LFP_ON_DEVICE
        job = rec.decompress_picture(d)
        rec.wait(job)
        got = rec.read_picture(int(d.hdr.out_slot))
        nd = getattr(d, "num_dmvr", 0)
        dmvr = rec.read_dmvr(job, nd) if nd else None
    finally:
        if lfp_on_device:
            d.hdr.tool_flags &= ~abi.TOOL_LFP_ON_DEVICE
        rec.close()
    return got, dmvr


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_limits_bit_exact(built, case):
    d, refs = case.make()
    st = lc.Stages(d, refs)
    want = st(0)
    case.present(case, d, refs, st)
    got, dmvr = _through_the_back_end(d, refs, case.l2)
    for c in range(len(want)):
        g = got[c][:want[c].shape[0], :want[c].shape[1]]
        assert np.array_equal(g, want[c]), "%s comp %d: %d samples differ" % (case.id, c, int((g != want[c]).sum()))
    if st.dmvr is not None:
        assert np.array_equal(dmvr, st.dmvr), "%s: DMVR delta MVs differ" % case.id


@pytest.mark.parametrize("case", [c for c in lc.CASES if c.derive_lfp], ids=[c.id for c in lc.CASES if c.derive_lfp])
def test_limits_edge_parameters_derived_on_the_device(built, case):
    """the cases whose subject is the deblocking - QPs at both ends, offsets at +-6, hard edges - once more with VVR_TOOL_LFP_ON_DEVICE: k_lf_maps / k_lf_init
    derive the edge QPs from these CU records themselves"""
    d, refs = case.make()
    want = refdrv.oracle_reconstruct(d, refs)
    got, _ = _through_the_back_end(d, refs, case.l2, lfp_on_device=True)
    for c in range(len(want)):
        assert np.array_equal(got[c], want[c]), "%s comp %d: %d samples differ" % (case.id, c, int((got[c] != want[c]).sum()))


@pytest.mark.parametrize("name,kind,tools,seed", lc.STREAMS, ids=[x[0] for x in lc.STREAMS])
def test_limits_streams_from_an_extreme_picture(built, name, kind, tools, seed):
    """three pictures from an uploaded extreme picture (_run_stream's seed_picture), everything in flight and then picture by picture: BDOF / DMVR CUs between
    the extreme picture and its own reconstructions, the loop filters on"""
    modes = set()
    g = lc.STREAM_GEO

    def post(d):
        modes.update(int(m) for m in np.array(d.cu["mc_mode"], copy=True)[np.array(d.cu["pred_mode"], copy=True) == abi.PRED_INTER])
    _run_stream(g["W"], g["H"], g["frames"], g["gop"], seed, tools, log2_ctu=g["log2_ctu"], seed_picture=synth.extreme_picture(g["W"], g["H"], seed, kind=kind), post=post, **lc.STREAM_MIX)
    assert (abi.MC_BDOF in modes) if tools == TOOLS_B else (abi.MC_DMVR_BDOF in modes), sorted(modes)


def test_limits_collocated_motion_at_the_limit(built):
    """VVR_TOOL_COL_MOTION on the DMVR case whose start vectors lie beside an end of the 18-bit range: what the back-end hands out is the reference's final motion
    field (DecCu::TaskFinishMotionInfo), sub-sampled as in test_gpu_parity.py::test_collocated_motion_on_the_device.  From the reference's field alone: vectors
    that arrive on the limit from a start vector beside it, and vectors beyond it - the reference clamps the refined vector it predicts with and stores the
    unclamped sum, so the hand-out does the same.  tests/test_oracle_vs_ref_limits.py pins the oracle's planes and delta MVs for this input"""
    if not refdrv.available():
        pytest.skip("reference build not present")
    d, refs = lc.col_motion_at_the_limit()
    planes, motion = refdrv.reconstruct_with_motion(d, refs, flags=0)
    assert lc.handed_out_on_the_limit(d, motion) > 0 and lc.handed_out_beyond_the_limit(motion) > 0
    want = motion.reshape(d.h4, d.w4)[::2, ::2].reshape(-1)
    assert lc.handed_out_beyond_the_limit(want) > 0, "none of the cells that are handed out"
    import vvdec_amd
    rec = vvdec_amd.Reconstructor(int(d.hdr.width), int(d.hdr.height), num_slots=3, num_streams=1, log2_ctu=7)
    try:
        for slot, p in refs.items():
            rec.write_picture(slot, p)
        d.hdr.tool_flags |= abi.TOOL_COL_MOTION
        job = rec.decompress_picture(d)
        got = rec.read_col_motion(job)
        assert len(got) == len(want)
        assert np.array_equal(got["mv"], want["mv"]) and np.array_equal(got["ref_idx"], want["ref_idx"]), "%d records differ" % int((got["mv"] != want["mv"]).any(axis=(1, 2)).sum())
        assert all(np.array_equal(g, w) for g, w in zip(rec.read_picture(0), planes))
        st = lc.Stages(d, refs)
        st(0)
        assert np.array_equal(rec.read_dmvr(job, d.num_dmvr), st.dmvr)
    finally:
        rec.close()


def test_limits_long_lists_in_flight(built):
    """lists of 16 entries through the path a decoder uses - worker threads, several streams, everything submitted before the first wait: 24 pictures of a low-delay
    stream, each listing the 16 before it, in 18 slots taken round-robin, so a slot is written again while up to 16 pictures in flight still read it; then
    picture by picture against the oracle, and pipelined against serial (_run_stream)"""
    plans, nslots = lc.long_lists_plan()
    used = [set(), set()]

    def post(d):
        for cu in np.array(d.cu, copy=True)[np.array(d.cu["pred_mode"], copy=True) == abi.PRED_INTER]:
            for l, i in lc.cu_indices(d, cu):
                used[l].add(i)
    _run_stream(128, 64, len(plans), 0, 3601, TOOLS_DB | abi.TOOL_PROF, streams=3, log2_ctu=6, plan=(plans, nslots), post=post, p_affine=0.15, p_sbtmvp=0.1, p_geo=0.1, p_ciip=0.1, p_bi=0.6, p_coded=0.3, p_split_scale=1.3)
    assert max(len(pl.ref_slots[0]) for pl in plans) == abi.VVR_MAX_REFS and used[0] >= set(range(abi.VVR_MAX_REFS)) and used[1] >= set(range(abi.VVR_MAX_REFS)), used
