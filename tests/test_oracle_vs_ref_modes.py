"""CPU: the pictures of tests/mode_cases.py - every index of a mode table on every block shape it is legal on: the 67 luma intra modes and the reference lines
on the 25 CU shapes in I pictures and in intra CUs of B pictures, the chroma modes and the three CCLM modes on every chroma shape, the MIP modes with and
without transposition, both ISP directions, the 64 GPM splits on the 14 shapes that allow them, the interpolation phases of plain motion compensation.
The plain-C oracle against the real reference classes at every stage, scalar and SIMD, so that a mismatch of tests/test_gpu_modes.py is a kernel's; the
census of every case against its legal set, each counted instance shown to matter by one oracle run with the subject moved to the adjacent entry; and every
picture through the product's record checks on the stand-in runtime (tests/hoststub), so that a refusal of a legal, rarely drawn combination shows here.
The comparison with the reference is skipped where oracle/_ref is not built, like tests/test_oracle_vs_ref.py; the census and the record checks need the
oracle and the generator only."""
import ctypes as C

import numpy as np
import pytest

import refdrv
import limits_cases as lc
import mode_cases as mc
from vvdec_amd import abi
from test_oracle_vs_ref import STAGES
from test_host_glue import stub, Ctx       # noqa: F401 (stub is a fixture)

needs_ref = pytest.mark.skipif(not refdrv.available(), reason="oracle/_ref not built")
IDS = [c.id for c in mc.CASES]


@needs_ref
@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_oracle_equals_reference_on_the_modes(built, case):
    for n, (d, refs, l2) in enumerate(case.pictures()):
        st = lc.Stages(d, refs)
        nd = getattr(d, "num_dmvr", 0)
        for fl in STAGES:
            r = refdrv.reconstruct(d, refs, flags=fl, want_dmvr=nd)
            got = st(fl)
            for c in range(mc.plane_count(case)):
                assert np.array_equal(got[c], r["planes"][c]), "picture %d flags %d comp %d: %d differ" % (n, fl, c, int((got[c] != r["planes"][c]).sum()))
            if nd and fl == 0:
                assert np.array_equal(st.dmvr, r["dmvr"][:nd]), "picture %d: DMVR delta MVs differ" % n
        simd = refdrv.reconstruct(d, refs, flags=refdrv.SIMD)["planes"]
        assert all(np.array_equal(x, y) for x, y in zip(st(0), simd)), "picture %d: the reference's SIMD path differs from its scalar path" % n


@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_the_census_is_complete(built, case):
    """every entry of the case's legal set (less mode_cases.IMPOSSIBLE) has an instance with both neighbours inside the picture whose own samples change when
    its subject field is moved to the adjacent entry of the table - the analogue of test_the_limits_matter, one oracle run per checked instance"""
    mc.present(case, case.pictures())
    print("%s: %r" % (case.id, case.found))


@pytest.mark.parametrize("case", mc.CASES, ids=IDS)
def test_the_record_checks_accept_every_picture(stub, case):
    """vvr_prepare on the stand-in runtime: validation and work lists of every census picture"""
    for n, (d, refs, l2) in enumerate(case.pictures()):
        ctx = Ctx(stub, int(d.hdr.width), int(d.hdr.height), 3, log2_ctu=l2, bit_depth=case.bd, chroma_format=case.cf, leaf=True)
        try:
            p, h = d.c(), C.c_void_p()
            rc = stub.vvr_prepare(ctx.ctx, C.byref(p), C.byref(h))
            assert rc == abi.VVR_OK, "picture %d (seed %d) is refused: %s" % (n, case.specs[n][3], stub.vvr_last_error(ctx.ctx).decode())
            stub.vvr_free_prepared(ctx.ctx, h)
        finally:
            ctx.close()


def test_the_shares_of_the_shapes_hold_every_mode_with_both_lines():
    """the (mode, line) pairs are dealt out over the shapes: together the I-picture cases hold all 132, so do the B-picture cases, and every shape has both lines"""
    for name in ("intra_angular_i_", "intra_angular_b_"):
        cases = [c for c in mc.CASES if c.id.startswith(name) and any(e[0] == "line" for e in c.legal)]
        assert sorted(c.shape for c in cases) == sorted(mc.SHAPES)
        pairs = set()
        for c in cases:
            pairs |= {e[1:] for e in c.legal if e[0] == "mode_line"}
            assert {e[3] for e in c.legal if e[0] == "line"} == {1, 2} and {e[2] for e in c.legal if e[0] == "mode_line"} == {1, 2}, c.id
            assert {e[3] for e in c.legal if e[0] == "mode"} == set(range(67)), c.id
        assert pairs == {(m, r) for m in range(1, 67) for r in (1, 2)}


def test_the_legal_sets_are_the_rules():
    """the sizes of the legal sets, from the rules alone: 25 shapes x 67 modes; MIP 16 / 8 / 6 modes per size class, each transposed or not; 64 splits on the 14
    shapes with both sides in 8 .. 64 and neither side 8 times the other; the chroma shapes of a 4:2:0 single tree; ISP on every shape but 4 x 4; all pairs of
    both interpolation filter banks"""
    by = {}
    for c in mc.CASES:
        by.setdefault(c.id.rsplit("_", 1)[0], set()).update(c.legal)
    assert len({e for e in by["intra_angular_i"] if e[0] == "mode"}) == 25 * 67 == len({e for e in by["intra_angular_b"] if e[0] == "mode"})
    mip = by["intra_mip_i"] | by["intra_mip_b"]
    assert len(mip) == 2 * (16 + 9 * 8 + 15 * 6) and {e[1:3] for e in mip} == set(mc.SHAPES)
    assert len(mc.GPM_SHAPES) == 14 and (8, 64) not in mc.GPM_SHAPES and (64, 8) not in mc.GPM_SHAPES and len(by["gpm_splits"]) == 14 * 64
    fam = {}
    for c in mc.CASES:
        fam.setdefault(c.family, set()).update(c.legal)
    # chroma blocks of a 4:2:0 single tree: 4 .. 32 wide, 2 .. 32 high, at least 16 samples; every mode on each, the three CCLM modes with the flag off or on
    shapes = {(w, h) for w in (4, 8, 16, 32) for h in (2, 4, 8, 16, 32) if w * h >= 16}
    assert {e[1:] for e in fam["intra_chroma"] if e[0] == "chroma"} == {s + (m,) for s in shapes for m in range(67)}
    assert {e[1:4] for e in fam["intra_chroma"] if e[0] == "cclm"} == {s + (m,) for s in shapes for m in (67, 68, 69)}
    # a missing template: above or left outside the picture or in another tile, above in another slice (bands of CTU rows), each mode, the flag off and on
    assert {e for e in fam["intra_chroma"] if e[0].startswith("cclm_no_")} == {(n, m, f, why) for n, why in (("cclm_no_above", "picture"), ("cclm_no_left", "picture"),
            ("cclm_no_above", "tile"), ("cclm_no_left", "tile"), ("cclm_no_above", "slice")) for m in (67, 68, 69) for f in (0, 1)}
    # the chroma trees of dual-tree pictures: 4 .. 32 x 4 .. 32; CCLM not where the 64 x 64 luma node is split in two first
    dual = {(w, h) for w in (4, 8, 16, 32) for h in (4, 8, 16, 32)}
    assert {e[1:] for e in fam["intra_chroma"] if e[0] == "chroma_dual"} == {s + (m,) for s in dual for m in range(67)}
    assert {e[1:3] for e in fam["intra_chroma"] if e[0] == "cclm_dual"} == {s for s in dual if 32 not in s or s == (32, 32)}
    # LFNST: both indices with every mode on shapes of all four classes; the three transform families
    assert {mc.lfnst_class(*e[1:3]) for e in fam["lfnst_sets"] if e[0] == "lfnst"} == {"4x4", "8x8", "4xN", "8xN"}
    for s in mc.LFNST_SHAPES:
        assert {e[3:] for e in fam["lfnst_sets"] if e[:3] == ("lfnst",) + s} == {(i, m) for i in (1, 2) for m in range(67)}
    assert {e[1:] for e in fam["transform_types"] if e[0] == "mts"} == {(w, h, i) for w in (4, 8, 16, 32) for h in (4, 8, 16, 32) for i in (2, 3, 4, 5)}
    assert {e[1:] for e in fam["transform_types"] if e[0] == "dct2_last"} == set(mc.SHAPES)
    assert {e[1:] for e in fam["transform_types"] if e[0] == "sbt"} == {(w, h, i, p) for w, h in mc.SHAPES for i, ok in ((1, w >= 8), (2, h >= 8), (3, w >= 16), (4, h >= 16)) if ok for p in (0, 1)}
    # ISP: both directions on the 24 shapes of more than 16 samples
    assert {e[1:4] for e in fam["intra_isp"] if e[4] == 0} == {s + (dr,) for s in mc.SHAPES if s != (4, 4) for dr in (1, 2)}
    # the phases: all pairs of both filter banks, every phase per axis in every size class, the half-sample filter in the classes the cases hold
    assert {e[1:] for e in fam["mc_phases"] if e[0] == "luma"} == {(x, y) for x in range(16) for y in range(16)}
    assert {e[1:] for e in fam["mc_phases"] if e[0] == "chroma"} == {(x, y) for x in range(32) for y in range(32)}
    assert {e for e in fam["mc_phases"] if e[0] in "xy"} == {(a, c, p) for a in "xy" for c in (4, 8, 16) for p in range(16)}


@pytest.mark.parametrize("slice_type", [abi.SLICE_I, abi.SLICE_B])
def test_the_grid_cuts_every_ctu_into_cus_of_one_shape(slice_type):
    """the generator switch by itself: the luma area of a picture is covered by CUs of grid_w x grid_h and nothing else (a grid with a side of 4: luma-tree or
    inter-only CUs of that shape, and chroma-tree CUs over their parents); a grid the picture cannot hold is refused"""
    from vvdec_amd import synth
    for w, h in mc.SHAPES:
        p = synth.default_params(width=256, height=128, seed=9, slice_type=slice_type, log2_ctu=7 if (w + h) & 8 else 6, min_cu_log2=2, grid_w=w, grid_h=h, p_intra=0.5)
        if slice_type == abi.SLICE_B:
            synth.set_refs(p, [(1, 0)], [(2, 8)])
        d = synth.generate(p)
        luma = d.cu[d.cu["tree"] != abi.TREE_CHROMA]
        assert set(zip(luma["w"].tolist(), luma["h"].tolist())) == {(w, h)} and len(luma) == (256 // w) * (128 // h), (w, h)
        chroma = d.cu[d.cu["tree"] == abi.TREE_CHROMA]
        assert set(zip(chroma["w"].tolist(), chroma["h"].tolist())) <= {(max(w, 8), max(h, 8))}, (w, h)
    for kw in (dict(grid_w=4, grid_h=8, min_cu_log2=3), dict(grid_w=12, grid_h=8), dict(grid_w=128, grid_h=64), dict(grid_w=64, grid_h=32, log2_ctu=5), dict(grid_w=8, grid_h=0)):
        with pytest.raises(RuntimeError, match="vvs_generate failed"):
            synth.generate(synth.default_params(width=256, height=128, seed=9, slice_type=abi.SLICE_I, **kw))


def test_the_list_of_impossible_entries_does_not_grow():
    """no entry of any legal set is excused today; a name in the list is "family:entry", carries the reference line that forbids the entry, and excuses exactly that
    entry from the census - shown on a case with one MIP mode taken away"""
    assert len(mc.IMPOSSIBLE) <= 0
    case = [c for c in mc.CASES if c.id == "intra_mip_i_4x4"][0]
    pics = case.pictures()
    for d, refs, l2 in pics:
        for k, (e,) in case.instances(d):
            if e[3] == 5:
                mc.set_mip_mode(d, k, 4, e[4])
    try:
        mc.IMPOSSIBLE["intra_mip:%r" % (("mip", 4, 4, 5, 0),)] = "(a test: no such line)"
        with pytest.raises(AssertionError, match="1 of 32 entries without a counting instance"):
            mc.present(case, pics)
        with pytest.raises(AssertionError, match="1 of 32 entries are not in the pictures"):
            mc.held(case, pics)
    finally:
        mc.IMPOSSIBLE.clear()


def test_the_census_notices_a_missing_entry(built):
    """the check can fail: with MIP mode 5 of the 4 x 4 matrices rewritten to mode 4 everywhere, both entries of mode 5 are reported"""
    case = [c for c in mc.CASES if c.id == "intra_mip_i_4x4"][0]
    pics = case.pictures()
    for d, refs, l2 in pics:
        for k, (e,) in case.instances(d):
            if e[3] == 5:
                mc.set_mip_mode(d, k, 4, e[4])
    with pytest.raises(AssertionError, match="2 of 32 entries without a counting instance"):
        mc.present(case, pics)
