"""CPU: the plain-C oracle against the real reference classes at the ends of the value ranges - QPs from -QpBdOffset to 63, reference pictures that alternate
between 0 and the largest sample value, prediction weights, ALF / CC-ALF taps and deblocking offsets at the limits of their syntax, reference lists of 16 entries,
motion vectors over the 18-bit range, LMCS models at the ends of lmcs_data(), chroma QPs from mapping tables and offsets (installed into the reference's parameter
sets, so that its own QpParam derives them), min_qp_ts above 4 (tests/limits_cases.py).
Every input of tests/test_gpu_limits.py is pinned here first, so a GPU failure there says that the kernel is wrong, not the oracle.  Skipped where oracle/_ref
is not built, like tests/test_oracle_vs_ref.py."""
import numpy as np
import pytest

import refdrv
import limits_cases as lc
from vvdec_amd import abi, synth
from test_oracle_vs_ref import STAGES

pytestmark = pytest.mark.skipif(not refdrv.available(), reason="oracle/_ref not built")


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_oracle_equals_reference_at_the_limits(built, case):
    d, refs = case.make()
    n = lc.plane_count(case)
    st = lc.Stages(d, refs)
    nd = getattr(d, "num_dmvr", 0)
    for fl in STAGES:
        r = refdrv.reconstruct(d, refs, flags=fl, want_dmvr=nd)
        got = st(fl)
        for c in range(n):
            assert np.array_equal(got[c], r["planes"][c]), "flags %d comp %d: %d differ" % (fl, c, int((got[c] != r["planes"][c]).sum()))
        if nd and fl == 0:
            assert np.array_equal(st.dmvr, r["dmvr"][:nd]), "DMVR delta MVs differ"
    if case.derive_lfp:       # the description's edge table against the reference's own derivation, at these QPs and offsets
        for fl in (refdrv.STOP_AFTER_DBK, 0):
            b = refdrv.reconstruct(d, refs, flags=fl | refdrv.DERIVE_LFP)["planes"]
            assert all(np.array_equal(x, y) for x, y in zip(st(fl), b)), "flags %d: the reference derives other edge parameters" % fl
    # the reference's SIMD path: the scalar path above is the expected value; a disagreement here is a finding about the reference (range coverage)
    simd = refdrv.reconstruct(d, refs, flags=refdrv.SIMD)["planes"]
    assert all(np.array_equal(x, y) for x, y in zip(st(0), simd)), "the reference's SIMD path differs from its scalar path"
    case.present(case, d, refs, st)


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_the_limits_matter(built, case):
    """every case can fail: with its subject moved back to the middle of the range - reference pictures clamped to the middle half, the table as the generator
    drew it, QP 32, levels as drawn, reference indices folded to 0 and 1, vectors inside the encoder's clip window - the oracle reconstructs another picture.
    Where the decoder clips the vectors the clip is idempotent and the picture need not change (Case.middle == "vectors"): there the stored vectors differ and
    every other record is the same byte for byte - the case exercises the clip, not another picture"""
    d, refs = case.make()
    d2, refs2 = case.make(extreme=False)
    if case.middle == "vectors":
        lc.only_the_vectors_differ(d, d2)
        return
    final = refdrv.oracle_reconstruct(d, refs)
    other = refdrv.oracle_reconstruct(d2, refs2)
    assert lc.differ(final, other), "the picture does not depend on its extreme"


LMCS_CASES = [c for c in lc.CASES if c.family == "lmcs_model"]
CQP_CASES = [c for c in lc.CASES if c.family == "chroma_qp"]


@pytest.mark.parametrize("case", LMCS_CASES, ids=[c.id for c in LMCS_CASES])
def test_lmcs_tables_of_the_shapes_are_the_references(built, case):
    """the tables the generator builds from each named model are the ones the reference's Reshape builds from the same model (integration/vvr_extract.h reads
    them out of the Reshape object): forward and inverse map, chroma scale factors, pivots, the two bin indices"""
    d, refs = case.make()
    got, want, n = refdrv.extract(d, refs)["lmcs"], d.lmcs, 1 << case.bd
    for name, count in (("fwd_lut", n), ("inv_lut", n), ("chroma_scale", 16), ("pivot", 17)):
        a, b = np.ctypeslib.as_array(getattr(got, name))[:count], np.ctypeslib.as_array(getattr(want, name))[:count]
        assert np.array_equal(a, b), "%s: %d entries differ, the first at %d" % (name, int((a != b).sum()), int(np.flatnonzero(a != b)[0]))
    assert (int(got.min_bin), int(got.max_bin)) == (int(want.min_bin), int(want.max_bin))


@pytest.mark.parametrize("case", CQP_CASES, ids=[c.id for c in CQP_CASES])
def test_chroma_qps_of_the_model_are_qp_params(built, case):
    """with the model installed the harness asks the reference's QpParam for every TransformUnit::chromaQp and refuses a description that holds another value:
    the generator's restatement of QpParam is pinned TU by TU, and the QPs the reference dequantises with are the description's.  The glue hands them back."""
    d, refs = case.make()
    e = refdrv.extract(d, refs)
    ch = (d.tu["comp_mask"] & 6) != 0
    assert len(e["tu"]) == len(d.tu) and np.array_equal(e["tu"]["qp"][ch], d.tu["qp"][ch])
    t = int(np.flatnonzero(ch)[len(np.flatnonzero(ch)) // 2])
    for comp, delta in ((1, 1), (2, -1)):
        keep = int(d.tu["qp"][t, comp])
        d.tu["qp"][t, comp] = keep + delta if 0 <= keep + delta <= 63 + 6 * (case.bd - 8) else keep - delta
        with pytest.raises(RuntimeError, match="chroma QP model: QpParam gives %d" % keep):
            refdrv.reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
        d.tu["qp"][t, comp] = keep
    # and without the model the reference sees the identity mapping: another picture
    model, d.chroma_qp_model = d.chroma_qp_model, None
    try:
        other = refdrv.reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)["planes"]
    finally:
        d.chroma_qp_model = model
    assert lc.differ(other[1:], refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)[1:]), "the reference's dequantisation does not see the chroma QPs"


def test_collocated_motion_at_the_limit_on_the_cpu(built):
    """the input of tests/test_gpu_limits.py::test_limits_collocated_motion_at_the_limit: the oracle's planes and DMVR delta MVs are the reference's, and the
    reference's final motion field alone holds refined vectors that arrive on an end of the 18-bit range from a start vector beside it - and vectors beyond it:
    the reference clamps the refined vector it predicts with, not the one it stores (limits_cases.handed_out_beyond_the_limit)"""
    d, refs = lc.col_motion_at_the_limit()
    nd = d.num_dmvr
    planes, motion = refdrv.reconstruct_with_motion(d, refs, flags=0)
    got = refdrv.oracle_reconstruct(d, refs)
    assert not lc.differ(got, planes)
    assert np.array_equal(refdrv.oracle_dmvr(nd), refdrv.reconstruct(d, refs, want_dmvr=nd)["dmvr"][:nd])
    n = lc.handed_out_on_the_limit(d, motion)
    beyond = lc.handed_out_beyond_the_limit(motion)
    print("cells of the final motion field on the limit whose start vector was not: %d; beyond the limit (stored unclamped by the reference): %d" % (n, beyond))
    assert n > 0 and beyond > 0


@pytest.mark.parametrize("name,kind,tools,seed", lc.STREAMS, ids=[x[0] for x in lc.STREAMS])
def test_oracle_equals_reference_on_the_streams_from_an_extreme_picture(built, name, kind, tools, seed):
    """the streams tests/test_gpu_limits.py sends through _run_stream: the same descriptions, the oracle consuming its own pictures as references"""
    from vvdec_amd import stream
    g = lc.STREAM_GEO
    plans, _ = stream.ra_plan(g["frames"], gop=g["gop"], seed_poc0_is_external=True)
    dpb = {0: synth.extreme_picture(g["W"], g["H"], seed, kind=kind)}
    flat = lc.middle_half(dpb[0], 10)
    modes, moved = set(), False
    for pl in plans:
        d = synth.picture_for_plan(pl, g["W"], g["H"], seed=seed, tool_flags=tools, log2_ctu=g["log2_ctu"], **lc.STREAM_MIX)
        modes.update(int(m) for m in d.cu["mc_mode"][d.cu["pred_mode"] == abi.PRED_INTER])
        nd = d.num_dmvr
        for fl in STAGES:
            r = refdrv.reconstruct(d, dpb, flags=fl, want_dmvr=nd)
            got = refdrv.oracle_reconstruct(d, dpb, flags=fl)
            assert not lc.differ(got, r["planes"]), "POC %d flags %d" % (pl.poc, fl)
            if nd:
                assert np.array_equal(refdrv.oracle_dmvr(nd), r["dmvr"][:nd]), "POC %d: DMVR delta MVs differ" % pl.poc
        if pl is plans[0]:       # the extreme picture matters
            assert lc.differ(got, refdrv.oracle_reconstruct(d, {0: flat}))
        dpb[pl.slot] = got
    assert (abi.MC_BDOF in modes) if tools == lc.TOOLS_B else (abi.MC_DMVR_BDOF in modes), sorted(modes)


@pytest.mark.parametrize("kind", synth.EXTREME_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_extreme_pictures(kind, bd):
    """the pictures themselves: only 0 and max (noise: the whole range with both ends), every plane drawn on its own, both orientations and phases of the
    checker, step edges on and off the 8-sample grid"""
    mx = (1 << bd) - 1
    y, cb, cr = synth.extreme_picture(256, 128, 7, bit_depth=bd, kind=kind)
    assert y.shape == (128, 256) and cb.shape == cr.shape == (64, 128) and y.dtype == np.uint16
    for p in (y, cb, cr):
        if kind == "flat_max":
            assert (p == mx).all()
        elif kind == "flat_zero":
            assert (p == 0).all()
        else:
            assert p.min() == 0 and p.max() == mx
            if kind != "noise":
                assert set(np.unique(p)) == {0, mx}
    if kind in ("checker", "steps", "noise", "taps"):
        assert not np.array_equal(cb, cr) and not np.array_equal(cb, y[::2, ::2]) and not np.array_equal(cb, y[:64, :128])
    if kind == "checker":
        b = (y[:, :] > 0).astype(int)
        hor, ver = (b[:, 1:] != b[:, :-1]), (b[1:, :] != b[:-1, :])
        blocks = [(hor[j:j + 16, i:i + 15].all(), ver[j:j + 15, i:i + 16].all()) for j in range(0, 128, 16) for i in range(0, 256, 16)]
        assert {(True, True), (True, False), (False, True)} == set(blocks)       # per sample, per column, per row
        assert len({int(y[j, i]) for j in range(0, 128, 16) for i in range(0, 256, 16)}) == 2      # both phases
    if kind == "taps":      # the half-sample filter along a row of a block: the largest overshoot a row of samples can produce
        f = np.array([-1, 4, -11, 40, 40, -11, 4, -1])
        best = max(int((y[j, i:i + 8].astype(int) * f).sum()) for j in range(0, 128, 5) for i in range(0, 248))
        assert best == 88 * mx
    if kind == "steps":
        edges = np.nonzero((y[:, 1:] != y[:, :-1]).any(axis=0))[0] + 1
        assert (edges % 8 == 0).any() and (edges % 8 == 4).any()
        runs = np.diff(np.concatenate([[0], np.nonzero(y[0, 1:] != y[0, :-1])[0] + 1, [256]]))
        assert runs.min() >= 4
