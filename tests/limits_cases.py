"""The cases of the range-limit tests: pictures whose QPs, samples, weights, filter taps, reference indices, motion vectors and side tables (LMCS model,
chroma QP mapping and offsets, min_qp_ts) sit at the ends of what the syntax allows.

One table, two users: tests/test_oracle_vs_ref_limits.py pins every input on the CPU (oracle against the reference classes), tests/test_gpu_limits.py
then runs the same inputs through the back-end against the oracle.  Nothing here touches a GPU or the reference build: a case is a builder
`make(extreme=True) -> (description, reference pictures)` plus a check `present(case, d, refs, stage)` of what the picture must hold, computed from the
description's records and the oracle's stage outputs.  `make(extreme=False)` is the same picture with the subject of the case moved back to the middle
of the range (reference pictures clamped to the middle half, the table as the generator drew it, QP 32): the CPU leg asserts that the oracle's picture
changes, i.e. that the case depends on its extreme."""
import numpy as np

import refdrv
from vvdec_amd import abi, synth
from test_gpu_parity import TOOLS, TOOLS_I, TOOLS_B, TOOLS_DB, TOOLS_A
from test_gpu_itrans_packed import _saturate, _blocks

FILTERS = abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_CCALF
B, P, I = abi.SLICE_B, abi.SLICE_P, abi.SLICE_I


def no_filters(tools):
    """prediction only: what the MC kernels write is what the picture holds"""
    return (tools & ~FILTERS) | abi.TOOL_DEBLOCK_OFF


def middle_half(planes, bd):
    mx = (1 << bd) - 1
    return [np.clip(p, mx // 4, mx - mx // 4).astype(np.uint16) for p in planes]


def one_picture(W, H, l2, seed, tools, kinds=(), slice_type=B, bd=10, cf=1, extreme=True, **kw):
    """one picture at POC 4 in slot 0; its reference pictures are extreme pictures of `kinds`: slot 1 (POC 0) and slot 2 (POC 8), list 0 = [1, 2],
    list 1 = [2, 1] - CUs with the same index in both lists predict from opposite directions at the same distance (BDOF / DMVR)"""
    p = synth.default_params(width=W, height=H, seed=seed, tool_flags=tools, slice_type=slice_type, log2_ctu=l2, bit_depth=bd, chroma_format=cf, **kw)
    p.poc, p.out_slot = 4, 0
    refs = {}
    if slice_type != I:
        synth.set_refs(p, [(1, 0), (2, 8)], [] if slice_type == P else [(2, 8), (1, 0)])
        for k, slot in enumerate((1, 2)):
            pic = synth.extreme_picture(W, H, seed * 10 + k, bit_depth=bd, kind=kinds[k % len(kinds)])
            refs[slot] = (pic if extreme else middle_half(pic, bd))[:3 if cf else 1]
    return synth.generate(p), refs


class Stages:
    """the oracle's stage outputs of one case, computed once"""

    def __init__(self, d, refs):
        self.d, self.refs, self._out, self.dmvr = d, refs, {}, None

    def __call__(self, flag):
        if flag not in self._out:
            self._out[flag] = refdrv.oracle_reconstruct(self.d, self.refs, flags=flag)
            if flag == 0:
                nd = getattr(self.d, "num_dmvr", 0)
                self.dmvr = refdrv.oracle_dmvr(nd).copy() if nd else None
        return self._out[flag]


def differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def holds_both_ends(planes, bd):
    mx = (1 << bd) - 1
    return all(int(p.min()) == 0 and int(p.max()) == mx for p in planes)


class Case:
    """middle: what make(extreme=False) is asserted to change - "picture": the oracle reconstructs another picture; "vectors": the stored motion vectors differ
    and every other record is byte-identical (the decoder's clip is idempotent: the picture need not change, the case exercises the clip and nothing else).
    found: the numbers `present` counted, for the record (a later change to the generator that empties a case shows there first)"""

    def __init__(self, id, family, make, present, derive_lfp=False, bd=10, cf=1, l2=7, middle="picture"):
        self.id, self.family, self.make, self.present, self.derive_lfp, self.bd, self.cf, self.l2 = id, family, make, present, derive_lfp, bd, cf, l2
        self.middle, self.found = middle, {}


CASES = []


def case(id, family, present, derive_lfp=False, bd=10, cf=1, l2=7, middle="picture"):
    def reg(make):
        CASES.append(Case(id, family, make, present, derive_lfp, bd, cf, l2, middle))
        return make
    return reg


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# QP at the low end
# ----------------------------------------------------------------------------------------------------------------------------------------------------
RESI = dict(p_coded=0.9, p_coded_chroma=0.8, p_ts=0.3, p_bdpcm=0.3, p_mts=0.4, p_lfnst=0.4, p_intra=0.3, p_small_corner=0.5)


def _qp_low_present(c, d, refs, st):
    qpbd = 6 * (c.bd - 8)
    b = _blocks(d)
    sums = {int(np.log2(w)) + int(np.log2(h)) for w, h, comp, tu, cu in b}
    assert sums >= set(range(4, 13)), sorted(sums)
    assert {int(cu["pred_mode"]) for w, h, comp, tu, cu in b} >= {abi.PRED_INTRA, abi.PRED_INTER}
    ts = [int(tu["qp"][comp]) for w, h, comp, tu, cu in b if int(tu["mts_idx"][comp]) == abi.MTS_SKIP]
    assert len(ts) > 0
    if int(d.cu["qp"].min()) + qpbd < int(d.hdr.min_qp_ts):         # (QP 2 at 10 bit is TU.qp 11 .. 17: above the bound by arithmetic, not by seed)
        assert sum(1 for q in ts if q < int(d.hdr.min_qp_ts)) > 0
    # tc = 0 and beta = 0 at these QPs: edges are there (strength > 0), and deblocking leaves the picture alone
    assert int(((d.lfp[0]["bs"] & 3) > 0).sum()) > 0 and int(d.cu["qp"].max()) <= 8
    assert not differ(st(refdrv.STOP_AFTER_DBK), st(refdrv.STOP_AFTER_RECO))


def _qp_case(id, family, present, qp, bd, tools, seed, W=256, H=128, l2=7, post=None, keep_qp=False, kinds=("noise", "noise"), derive_lfp=False, **kw):
    @case(id, family, present, bd=bd, l2=l2, derive_lfp=derive_lfp)
    def make(extreme=True):
        d, refs = one_picture(W, H, l2, seed, tools, kinds, bd=bd, base_qp=qp if extreme or keep_qp else 32, **kw)
        if post:
            post(d, extreme)
        return d, refs


LOW = dict(RESI, min_cu_log2=2, p_split_scale=0.75)
_qp_case("qp_low_2_10bit", "qp_low", _qp_low_present, 2, 10, TOOLS_I, 3200, **LOW)
_qp_case("qp_low_minus_10_10bit", "qp_low", _qp_low_present, -10, 10, TOOLS_I, 3202, derive_lfp=True, **LOW)
_qp_case("qp_low_minus_10_10bit_no_dep_quant_scaling_lists", "qp_low", _qp_low_present, -10, 10, (TOOLS_I & ~abi.TOOL_DEP_QUANT) | abi.TOOL_SCALING_LIST, 3204, l2=6, **LOW)
_qp_case("qp_low_2_8bit_scaling_lists", "qp_low", _qp_low_present, 2, 8, TOOLS_I | abi.TOOL_SCALING_LIST, 3206, **LOW)
_qp_case("qp_low_2_8bit_no_dep_quant", "qp_low", _qp_low_present, 2, 8, TOOLS_I & ~abi.TOOL_DEP_QUANT, 3202, l2=6, **LOW)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# QP at the high end, deblocking offsets at the ends of their range
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _qp_high_present(c, d, refs, st):
    assert int(d.cu["qp"].min()) >= 58 and int(d.cu["qp"].max()) == 63
    assert abs(int(d.hdr.deblock_tc_offset_div2[0])) == 6 and abs(int(d.hdr.deblock_beta_offset_div2[1])) == 6
    assert differ(st(refdrv.STOP_AFTER_DBK), st(refdrv.STOP_AFTER_RECO)), "deblocking changes nothing"
    keep = [(list(d.hdr.deblock_beta_offset_div2), list(d.hdr.deblock_tc_offset_div2))]
    for k in range(3):
        d.hdr.deblock_beta_offset_div2[k] = d.hdr.deblock_tc_offset_div2[k] = 0
    zero = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_DBK)
    for k in range(3):
        d.hdr.deblock_beta_offset_div2[k], d.hdr.deblock_tc_offset_div2[k] = keep[0][0][k], keep[0][1][k]
    assert differ(zero, st(refdrv.STOP_AFTER_DBK)), "the offsets change nothing"


def _offsets(sign):
    def post(d, extreme):
        if extreme:
            synth.deblock_offsets_to_limits(d, sign)
        else:
            for k in range(3):
                d.hdr.deblock_beta_offset_div2[k] = d.hdr.deblock_tc_offset_div2[k] = 0
    return post


HIGH = dict(RESI, p_split_scale=0.8)
_qp_case("qp_high_61_10bit_offsets_plus_6", "qp_high", _qp_high_present, 61, 10, TOOLS_I, 3011, post=_offsets(+1), keep_qp=True, derive_lfp=True, **HIGH)
_qp_case("qp_high_61_10bit_offsets_minus_6", "qp_high", _qp_high_present, 61, 10, TOOLS_I, 3012, l2=6, post=_offsets(-1), keep_qp=True, derive_lfp=True, **HIGH)
_qp_case("qp_high_61_8bit_offsets_plus_6", "qp_high", _qp_high_present, 61, 8, TOOLS_I, 3013, W=200, H=136, l2=5, post=_offsets(+1), keep_qp=True, derive_lfp=True, **HIGH)
_qp_case("qp_high_61_8bit_offsets_minus_6_ladf", "qp_high", _qp_high_present, 61, 8, TOOLS_I | abi.TOOL_LADF, 3014, post=_offsets(-1), keep_qp=True, derive_lfp=True, **HIGH)
_qp_case("qp_high_61_10bit_offsets_plus_6_ladf", "qp_high", _qp_high_present, 61, 10, TOOLS_I | abi.TOOL_LADF, 3015, l2=6, post=_offsets(+1), keep_qp=True, derive_lfp=True, **HIGH)


def _saturated(then=None):
    def post(d, extreme):
        if then:
            then(d, extreme)
        if extreme:
            _saturate(d)
    return post


def _qp_saturated_present(c, d, refs, st):
    """levels of +-32767 through the dequantisation at per 0 (a right shift with rounding) and at per 12 (a left shift into the 16-bit clip)"""
    b = _blocks(d)
    assert len(b) > 0 and int(np.abs(d.coef).max()) == 32767
    per = {(int(tu["qp"][comp]) + (1 if int(d.hdr.tool_flags) & abi.TOOL_DEP_QUANT and int(tu["mts_idx"][comp]) != abi.MTS_SKIP else 0)) // 6 for w, h, comp, tu, cu in b}
    assert (0 in per) if int(d.cu["qp"].max()) < 32 else (max(per) == (12 if c.bd == 10 else 10)), sorted(per)
    assert holds_both_ends(st(refdrv.STOP_AFTER_RECO), c.bd)


_qp_case("qp_low_minus_10_10bit_saturated_levels", "qp_low", _qp_saturated_present, -10, 10, TOOLS_I, 3231, post=_saturated(), **LOW)
_qp_case("qp_low_2_8bit_saturated_levels_no_dep_quant", "qp_low", _qp_saturated_present, 2, 8, (TOOLS_I & ~abi.TOOL_DEP_QUANT) | abi.TOOL_SCALING_LIST, 3232, l2=6, post=_saturated(), **LOW)
_qp_case("qp_high_61_10bit_saturated_levels", "qp_high", _qp_saturated_present, 61, 10, TOOLS_I, 3233, post=_saturated(), derive_lfp=True, **dict(HIGH, min_cu_log2=2))
_qp_case("qp_high_61_8bit_saturated_levels_scaling_lists", "qp_high", _qp_saturated_present, 61, 8, (TOOLS_I & ~abi.TOOL_DEP_QUANT) | abi.TOOL_SCALING_LIST, 3234, l2=6, post=_saturated(), derive_lfp=True, **dict(HIGH, min_cu_log2=2))


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# both ends in one picture
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _spread(d, extreme):
    qpbd = 6 * (int(d.hdr.bit_depth) - 8)
    n = len(d.cu)
    synth.rewrite_qp(d, np.where(np.arange(n) & 1, 63, -qpbd) if extreme else np.full(n, 32))


def _qp_spread_present(c, d, refs, st):
    n = 0
    for dr in range(2):
        q4 = np.zeros((d.h4, d.w4), np.int32)
        for cu in d.cu:
            q4[int(cu["y"]) >> 2:(int(cu["y"]) + int(cu["h"])) >> 2, int(cu["x"]) >> 2:(int(cu["x"]) + int(cu["w"])) >> 2] = int(cu["qp"])
        far = np.abs(q4 - np.roll(q4, 1, axis=1 - dr)) > 50
        far[:, 0] &= dr == 1
        far[0, :] &= dr == 0
        bs = d.lfp[dr]["bs"].reshape(d.h4, d.w4)
        n += int((far & ((bs & 3) > 0)).sum())
    assert n > 0, "no filtered edge between the two ends"
    assert differ(st(refdrv.STOP_AFTER_DBK), st(refdrv.STOP_AFTER_RECO))


_qp_case("qp_spread_10bit", "qp_spread", _qp_spread_present, 32, 10, TOOLS_I, 3021, post=_spread, keep_qp=True, derive_lfp=True, **HIGH)
_qp_case("qp_spread_8bit_ctu64", "qp_spread", _qp_spread_present, 32, 8, TOOLS_I, 3022, l2=6, post=_spread, keep_qp=True, derive_lfp=True, **HIGH)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# motion compensation on extreme reference pictures (prediction only: no residual, no filters)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _inter(d):
    return d.cu[d.cu["pred_mode"] == abi.PRED_INTER]


def _mc_present(c, d, refs, st):
    cu = _inter(d)
    plain = cu[(cu["mc_mode"] == abi.MC_UNI) | (cu["mc_mode"] == abi.MC_BI)]
    assert {abi.MC_UNI, abi.MC_BI} <= set(int(m) for m in plain["mc_mode"])
    for comp in range(2):       # every fractional phase (1/16 luma sample) in x and in y
        ph = set()
        for l in range(2):
            ph |= set(int(v) & 15 for v in plain["mv"][:, l, 0, comp][plain["ref_idx"][:, l] >= 0])
        assert ph == set(range(16)), (comp, sorted(ph))
    assert int((cu["imv"] == 3).sum()) > 0
    if c.family != "mono_8bit":
        assert int((cu["w"] == 4).sum()) > 0 and int((cu["h"] == 4).sum()) > 0
    assert holds_both_ends(st(0), c.bd), "the prediction is clipped from one side only"


def _mc_case(id, family, present, tools, seed, kinds, W=256, H=128, l2=7, bd=10, cf=1, slice_type=B, post=None, clamp_refs=True, **kw):
    @case(id, family, present, bd=bd, cf=cf, l2=l2)
    def make(extreme=True):
        d, refs = one_picture(W, H, l2, seed, tools, kinds, slice_type=slice_type, bd=bd, cf=cf, extreme=extreme or not clamp_refs, **kw)
        if post:
            post(d, extreme)
        return d, refs


MC = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_imv_hpel=0.3, min_cu_log2=2, p_split_scale=1.3)
_mc_case("mc_checker_noise", "regular_mc", _mc_present, no_filters(TOOLS_I), 3031, ("checker", "noise"), **MC)
_mc_case("mc_noise_checker_ctu32", "regular_mc", _mc_present, no_filters(TOOLS_I), 3032, ("noise", "checker"), W=200, H=136, l2=5, **MC)


_mc_case("mc_taps", "regular_mc", _mc_present, no_filters(TOOLS_I), 3033, ("taps",), l2=6, **MC)


def _bcw_present(c, d, refs, st):
    cu = _inter(d)
    bi = cu[cu["mc_mode"] == abi.MC_BI]
    assert {0, 4} <= set(int(v) for v in bi["bcw_idx"]), sorted(set(int(v) for v in bi["bcw_idx"]))
    assert int(((cu["flags"] & abi.CU_GEO) != 0).sum()) > 0 and int(((cu["flags"] & abi.CU_CIIP) != 0).sum()) > 0
    assert int((d.cu["pred_mode"] == abi.PRED_INTRA).sum()) > 0
    if d.lmcs is None:
        assert holds_both_ends(st(0), c.bd)
    else:       # (forward and inverse luma map in a row need not return the ends; the predictions that go in still hold them)
        assert holds_both_ends([r[0] for r in refs.values()], c.bd) and int(st(0)[0].max()) - int(st(0)[0].min()) > 3 << (c.bd - 2)


BCW = dict(MC, p_bcw=1.0, p_geo=0.4, p_ciip=0.4, p_intra=0.2, p_bi=0.8)
_mc_case("bcw_gpm_ciip_checker_noise", "bcw_gpm_ciip", _bcw_present, no_filters(TOOLS_A), 3041, ("checker", "noise"), **BCW)
_mc_case("bcw_gpm_ciip_noise_checker_ctu64", "bcw_gpm_ciip", _bcw_present, no_filters(TOOLS_A), 3042, ("noise", "checker"), l2=6, **BCW)


_mc_case("bcw_gpm_ciip_checker_noise_lmcs", "bcw_gpm_ciip", _bcw_present, no_filters(TOOLS_A) | abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE, 3243, ("checker", "noise"), **BCW)


def _bdof_present(c, d, refs, st):
    assert int((_inter(d)["mc_mode"] == abi.MC_BDOF).sum()) > 0
    assert holds_both_ends(st(0)[:1], c.bd)


BI = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_bi=1.0, mv_sigma=3.0)
_mc_case("bdof_checker", "bdof", _bdof_present, no_filters(TOOLS_B), 3051, ("checker",), **BI)
_mc_case("bdof_steps_ctu64", "bdof", _bdof_present, no_filters(TOOLS_B), 3052, ("steps",), l2=6, **BI)


_mc_case("bdof_taps", "bdof", _bdof_present, no_filters(TOOLS_B), 3254, ("taps",), **BI)
_mc_case("bdof_checker_8bit", "bdof", _bdof_present, no_filters(TOOLS_B), 3253, ("checker", "steps"), bd=8, **BI)


def _dmvr_present(c, d, refs, st):
    cu = _inter(d)
    assert d.num_dmvr > 0 and int((cu["mc_mode"] == abi.MC_DMVR_BDOF).sum()) > 0
    st(0)
    assert st.dmvr is not None and len(st.dmvr) == d.num_dmvr


def _dmvr_moves(c, d, refs, st):
    _dmvr_present(c, d, refs, st)
    assert int((st.dmvr != 0).any(axis=1).sum()) > 0, "no sub-block was refined"


def _dmvr_tie(c, d, refs, st):
    """flat_max against flat_zero: every candidate of the search costs the same, so the delta MVs are the tie-break - no refinement at all"""
    _dmvr_present(c, d, refs, st)
    assert not st.dmvr.any()


_mc_case("dmvr_checker", "dmvr", _dmvr_moves, no_filters(TOOLS_DB), 3061, ("checker",), **BI)
_mc_case("dmvr_steps_ctu64", "dmvr", _dmvr_moves, no_filters(TOOLS_DB), 3062, ("steps",), l2=6, **BI)
_mc_case("dmvr_flat_max_against_flat_zero", "dmvr", _dmvr_tie, no_filters(TOOLS_DB), 3063, ("flat_max", "flat_zero"), **BI)


_mc_case("dmvr_taps_ctu32", "dmvr", _dmvr_moves, no_filters(TOOLS_DB), 3265, ("taps",), W=200, H=136, l2=5, **BI)
_mc_case("dmvr_checker_steps_8bit", "dmvr", _dmvr_moves, no_filters(TOOLS_DB), 3264, ("checker", "steps"), bd=8, **BI)


def _affine_present(c, d, refs, st):
    f = _inter(d)["flags"]
    assert int((((f & abi.CU_AFFINE) != 0) & ((f & abi.CU_AFFINE_6P) != 0)).sum()) > 0 and int((((f & abi.CU_AFFINE) != 0) & ((f & abi.CU_AFFINE_6P) == 0)).sum()) > 0
    assert holds_both_ends(st(0)[:1], c.bd)


AFF = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_affine=0.7)
_mc_case("affine_prof_checker_mv_sigma_2", "affine_prof", _affine_present, no_filters(TOOLS_A), 3071, ("checker",), mv_sigma=2.0, **AFF)
_mc_case("affine_prof_checker_mv_sigma_60_ctu64", "affine_prof", _affine_present, no_filters(TOOLS_A), 3072, ("checker",), l2=6, mv_sigma=60.0, **AFF)


_mc_case("affine_prof_taps", "affine_prof", _affine_present, no_filters(TOOLS_A), 3274, ("taps",), mv_sigma=4.0, **AFF)
_mc_case("affine_prof_checker_noise_8bit_ctu32", "affine_prof", _affine_present, no_filters(TOOLS_A), 3273, ("checker", "noise"), W=200, H=136, l2=5, bd=8, mv_sigma=8.0, **AFF)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# explicit weighted prediction at the limits of the weight table
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _wp_post(d, extreme):
    if extreme:
        synth.wp_to_limits(d, len(d.cu))       # (a seed of its own per picture)


def _wp_present(c, d, refs, st):
    w = d.wp
    assert {int(w.log2_denom[0]), int(w.log2_denom[1])} == {0, 7}
    cu = _inter(d)
    used = {(l, int(r)) for l in range(2) for r in cu["ref_idx"][:, l] if r >= 0}
    dw, off = set(), set()
    for (l, r) in used:
        for comp in range(3):
            e = w.e[l][r][comp]
            if e.present:
                dw.add((int(w.log2_denom[1 if comp else 0]), int(e.weight) - (1 << int(w.log2_denom[1 if comp else 0]))))
                off.add(int(e.offset))
    assert {dn for dn, _ in dw} == {0, 7} and {x for _, x in dw} == {-128, 127} and off == {-128, 127}, (sorted(dw), sorted(off))


WP = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.1, p_affine=0.2, p_sbtmvp=0.15, p_ciip=0.1, p_geo=0.1, p_bcw=0.2)
_mc_case("wp_limits_b_noise_flat_max", "weighted_prediction", _wp_present, no_filters(TOOLS_A | abi.TOOL_WP), 3201, ("noise", "flat_max"), post=_wp_post, clamp_refs=False, **WP)
_mc_case("wp_limits_p_flat_max_noise", "weighted_prediction", _wp_present, no_filters(TOOLS_A | abi.TOOL_WP), 3203, ("flat_max", "noise"), slice_type=P, l2=6, post=_wp_post, clamp_refs=False, **WP)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# scaled reference pictures
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _rpr_present(c, d, refs, st):
    assert len(_inter(d)) > 10 and d.rpr is not None
    assert holds_both_ends(st(0)[:1], c.bd)


def _rpr(k, name):
    from test_oracle_vs_ref import RPR_CASES, rpr_case, ALL
    W, H, l2, idx, seed, specs, win, colloc, kw = RPR_CASES[k]

    @case("rpr_%s_checker" % name, "rpr", _rpr_present, l2=l2)
    def make(extreme=True):
        d, refs = rpr_case(W, H, l2, idx, seed, specs, win=win, colloc=colloc, tools=no_filters(ALL), p_coded=0.0, p_coded_chroma=0.0, **kw)
        for slot in refs:
            h, w = refs[slot][0].shape
            pic = synth.extreme_picture(w, h, seed * 10 + slot, kind="checker")
            refs[slot] = pic if extreme else middle_half(pic, 10)
        return d, refs


_rpr(0, "1_5x")
_rpr(1, "2x")
_rpr(2, "0_5x")


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# SAO + ALF + CC-ALF on an extreme reconstruction with the filter tables at their limits
# ----------------------------------------------------------------------------------------------------------------------------------------------------
COPY = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_bi=0.0, mv_sigma=0.0, p_imv_hpel=0.0)       # every CU copies a reference picture at MV 0
LOOP = dict(COPY, p_sao=0.8, p_alf_luma=1.0, p_alf_chroma=1.0, p_ccalf=0.8)


def _alf_present(c, d, refs, st):
    reco = st(refdrv.STOP_AFTER_RECO)
    assert all(set(np.unique(p)) <= {0, (1 << c.bd) - 1} for p in reco), "the reconstruction is not the extreme picture"
    assert differ(st(0), st(refdrv.STOP_AFTER_SAO)), "ALF changes nothing"
    assert holds_both_ends(st(0), c.bd)
    lc = np.ctypeslib.as_array(d.alf_params.luma_coeff)[..., :12]
    assert set(np.unique(lc)) == {-128, 127} and set(np.unique(np.ctypeslib.as_array(d.alf_params.ccalf_coeff)[..., :7])) == {-64, 64}


def _alf_case(id, family, seed, kinds, clip, tools=TOOLS, W=256, H=128, l2=7, bd=10, cf=1, **kw):
    @case(id, family, _alf_present, bd=bd, cf=cf, l2=l2)
    def make(extreme=True):
        d, refs = one_picture(W, H, l2, seed, tools | abi.TOOL_DEBLOCK_OFF, kinds, bd=bd, cf=cf, **dict(LOOP, **kw))
        if extreme:
            synth.alf_to_limits(d, seed, clip=clip)
        return d, refs


_alf_case("sao_alf_fused_ctu128_checker_no_clipping", "sao_alf_ccalf", 3101, ("checker",), 0)
_alf_case("sao_alf_fused_ctu64_steps_tightest_clipping_virtual_boundary", "sao_alf_ccalf", 3102, ("steps",), 3, l2=6, virtual_boundaries=1 | (1 << 2))
_alf_case("sao_alf_fused_ctu64_checker_tightest_clipping", "sao_alf_ccalf", 3103, ("checker", "steps"), 3, l2=6)
_alf_case("sao_alf_separate_ctu32_checker_clipping_by_class", "sao_alf_ccalf", 3104, ("checker", "steps"), None, W=200, H=136, l2=5)
_alf_case("sao_alf_separate_ctu32_steps_no_clipping", "sao_alf_ccalf", 3105, ("steps", "checker"), 0, l2=5)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# deblocking on hard edges
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _dbk_present(c, d, refs, st):
    a, b = st(refdrv.STOP_AFTER_RECO), st(refdrv.STOP_AFTER_DBK)
    assert 42 <= int(d.cu["qp"].min()) and int(d.cu["qp"].max()) <= 63
    ch = a[0] != b[0]
    gy, gx = np.mgrid[0:ch.shape[0], 0:ch.shape[1]]
    # luma edges lie on the 8-sample grid here; the short filters reach three samples into a side, so a changed sample four or more away from the edges of
    # both directions was written by a long (7 / 5 / 3 with a 32-sample side) filter
    inner = ((gx & 7) >= 3) & ((gx & 7) <= 4) & ((gy & 7) >= 3) & ((gy & 7) <= 4)
    assert int((ch & inner).sum()) > 0, "no long luma filter"
    if c.cf:
        # chroma edges lie on the 8-sample chroma grid; the weak filter writes one sample per side, the strong one three
        for k in (1, 2):
            chc = a[k] != b[k]
            gy, gx = np.mgrid[0:chc.shape[0], 0:chc.shape[1]]
            one_dir = (((gx & 7) == 1) | ((gx & 7) == 2) | ((gx & 7) == 5) | ((gx & 7) == 6)) & ((gy & 7) >= 3) & ((gy & 7) <= 4)
            assert int((chc & one_dir).sum()) > 0, "no strong chroma filter in component %d" % k


def _dbk_case(id, seed, qp, bd, tools, W=256, H=128, l2=7, **kw):
    @case(id, "deblock_hard_edges", _dbk_present, bd=bd, l2=l2, derive_lfp=True)
    def make(extreme=True):
        kk = dict(COPY, p_coded=0.5, p_coded_chroma=0.4, p_split_scale=0.45, p_small_corner=1.0, **kw)
        return one_picture(W, H, l2, seed, tools, ("steps",), bd=bd, extreme=extreme, base_qp=qp, **kk)


_dbk_case("deblock_steps_qp48_10bit", 3111, 48, 10, TOOLS)
_dbk_case("deblock_steps_qp60_8bit_ctu64", 3201, 60, 8, TOOLS, l2=6)
_dbk_case("deblock_steps_qp56_10bit_lmcs", 3113, 56, 10, TOOLS | abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE)
_dbk_case("deblock_steps_qp52_8bit_ctu32", 3114, 52, 8, TOOLS, W=200, H=136, l2=5)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# intra prediction from saturated neighbours
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _intra_present(c, d, refs, st):
    reco = st(refdrv.STOP_AFTER_RECO)[0].astype(np.int32)
    mx = (1 << c.bd) - 1
    cclm = d.cu[(d.cu["pred_mode"] == abi.PRED_INTRA) & (d.cu["intra_dir"][:, 1] >= 67) & (d.cu["tree"] != abi.TREE_LUMA)]
    full = 0
    for cu in cclm:
        x, y, w, h = int(cu["x"]), int(cu["y"]), int(cu["w"]), int(cu["h"])
        nb = np.concatenate([reco[max(0, y - 2):y, x:x + w].ravel(), reco[y:y + h, max(0, x - 3):x].ravel()])
        if len(nb) and nb.max() - nb.min() >= mx - 3:       # (the templates are 2:1 down-sampled luma: a span this wide outlasts the [1 2 1] taps in at least one phase)
            full += 1
    assert full > 0, "no CCLM CU whose neighbouring luma spans the range (%d CCLM CUs)" % len(cclm)
    assert int(((d.cu["flags"] & abi.CU_MIP) != 0).sum()) > 0
    assert int((d.cu["isp_mode"] != 0).sum()) > 0 and int((d.cu["multi_ref_idx"] != 0).sum()) > 0
    assert holds_both_ends(st(refdrv.STOP_AFTER_RECO), c.bd)


def _intra_case(id, seed, slice_type, l2=7, bd=10, W=256, H=128, **kw):
    @case(id, "intra_extreme_neighbours", _intra_present, bd=bd, l2=l2)
    def make(extreme=True):
        kk = dict(p_cclm=0.5, p_mip=0.3, p_isp=0.3, p_mrl=0.3, p_coded=0.8, p_coded_chroma=0.6, p_lfnst=0.3, **kw)
        d, refs = one_picture(W, H, l2, seed, TOOLS_A, ("noise", "checker"), slice_type=slice_type, bd=bd, **kk)
        if extreme:
            _saturate(d)
        return d, refs


_intra_case("intra_saturated_i_picture", 3121, I)
_intra_case("intra_saturated_cus_of_a_b_picture_ctu64", 3122, B, l2=6, p_intra=0.5)
_intra_case("intra_saturated_i_picture_8bit_ctu32", 3123, I, l2=5, bd=8, W=200, H=136)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# the other sample formats: one regular-MC case and one filter case at 4:0:0 and at 8 bit
# ----------------------------------------------------------------------------------------------------------------------------------------------------
MC8 = dict(MC, min_cu_log2=3)
_mc_case("mc_checker_noise_400", "mono_8bit", _mc_present, no_filters(TOOLS_I), 3200, ("checker", "noise"), cf=0, **MC8)
_mc_case("mc_checker_noise_8bit", "mono_8bit", _mc_present, no_filters(TOOLS_I), 3132, ("checker", "noise"), bd=8, **MC)
_mc_case("mc_taps_8bit", "mono_8bit", _mc_present, no_filters(TOOLS_I), 3137, ("taps",), bd=8, l2=6, **MC)
_alf_case("sao_alf_fused_ctu128_checker_400", "mono_8bit", 3133, ("checker",), None, cf=0)
_alf_case("sao_alf_fused_ctu64_steps_8bit", "mono_8bit", 3134, ("steps", "checker"), None, l2=6, bd=8)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# reference picture lists of up to 16 entries (VVR_MAX_REFS): indices of 2 and more, a picture at several indices of one list
# ----------------------------------------------------------------------------------------------------------------------------------------------------
LIST_POC = 16
LIST_DISTS = (2, 8, 4)
POOL_KINDS = {2: "checker", 4: "noise", 6: "steps"}      # the pool: slots 1 .. 6, the odd ones natural pictures, the even ones extreme pictures of these kinds


def paired_lists(seed, n0, n1):
    """two lists over six pictures, drawn with repetition: slots 1 .. 3 lie 2, 8 and 4 pictures before the current one, slots 4 .. 6 as many after it.  At every
    index the two lists hold the two pictures of one distance, one before and one after: CUs with the same index in both lists are BDOF / DMVR candidates at
    every index, not only at 0 and 1"""
    rng = np.random.default_rng(seed)
    past = {dist: (1 + k, LIST_POC - dist) for k, dist in enumerate(LIST_DISTS)}
    future = {dist: (4 + k, LIST_POC + dist) for k, dist in enumerate(LIST_DISTS)}
    l0, l1 = [], []
    for i in range(abi.VVR_MAX_REFS):
        dist = LIST_DISTS[i] if i < 3 else LIST_DISTS[int(rng.integers(3))]
        a, b = past[dist], future[dist]
        if i >= 3 and rng.random() < 0.4:
            a, b = b, a
        l0.append(a)
        l1.append(b)
    return l0[:n0], l1[:n1]


def list_picture(W, H, l2, seed, tools, n0, n1, slice_type=B, bd=10, cf=1, scaled=None, **kw):
    """one picture at POC 16 in slot 0 with the lists of paired_lists; scaled: {slot: dict(ratio=, size=)} - the pictures of the pool that have another size
    (tests/test_oracle_vs_ref.py::rpr_case's way of attaching the table, for lists of any length)"""
    import ctypes as C
    l0, l1 = paired_lists(seed, n0, 0 if slice_type == P else n1)
    scaled = scaled or {}
    if scaled:
        kw["scaled_refs"] = (C.c_uint16 * 2)(*[sum(1 << i for i, (slot, _) in enumerate(lst) if slot in scaled) for lst in (l0, l1)])
    p = synth.default_params(width=W, height=H, seed=seed, tool_flags=tools, slice_type=slice_type, log2_ctu=l2, bit_depth=bd, chroma_format=cf, **kw)
    p.poc, p.out_slot = LIST_POC, 0
    synth.set_refs(p, l0, l1)
    d = synth.generate(p)
    if scaled:
        synth.attach_rpr(d, {(l, i): scaled[slot] for l, lst in enumerate((l0, l1)) for i, (slot, _) in enumerate(lst) if slot in scaled})
    refs = {}
    for slot in range(1, 7):
        w, h = scaled.get(slot, {}).get("size", (W, H))
        pic = synth.extreme_picture(w, h, seed * 10 + slot, bit_depth=bd, kind=POOL_KINDS[slot]) if slot in POOL_KINDS else synth.natural_picture(w, h, seed * 10 + slot, bit_depth=bd)
        refs[slot] = pic[:3 if cf else 1]
    return d, refs


def fold_indices(d):
    """every reference index to index & 1 over the same lists - CU records, GPM partitions, motion field - and the loop filters off (the edge tables were drawn
    for the other indices)"""
    r = d.cu["ref_idx"]
    d.cu["ref_idx"] = np.where(r >= 0, r & 1, r)
    g = d.cu["geo_dir_ref"]
    d.cu["geo_dir_ref"] = (g & 0xF0) | (g & 1)
    m = d.motion["ref_idx"]
    d.motion["ref_idx"] = np.where(m >= 0, m & 1, m)
    d.hdr.tool_flags = no_filters(int(d.hdr.tool_flags))
    return d


def cu_cells(d, cu):
    x4, y4, w4, h4 = int(cu["x"]) >> 2, int(cu["y"]) >> 2, int(cu["w"]) >> 2, int(cu["h"]) >> 2
    return d.motion.reshape(d.h4, d.w4)[y4:y4 + h4, x4:x4 + w4]


def cu_indices(d, cu):
    """the (list, reference index) pairs the prediction of a CU reads: its own, those of its GPM partitions, those of its SbTMVP sub-blocks in the motion field"""
    m = int(cu["mc_mode"])
    if m == abi.MC_GEO:
        return [((int(g) >> 4) - 1, int(g) & 15) for g in cu["geo_dir_ref"]]
    if m == abi.MC_SBTMVP:
        cells = cu_cells(d, cu)["ref_idx"].reshape(-1, 2)
        return sorted({(l, int(v)) for l in range(2) for v in cells[:, l] if v >= 0})
    return [(l, int(cu["ref_idx"][l])) for l in range(2) if cu["ref_idx"][l] >= 0]


def same_picture_other_index(d):
    """pairs of neighbouring 4x4 cells across a CU edge that refer, in one list, to the same picture through different indices: the deblocking compares pictures,
    so these are the edges an index comparison would filter (or not) wrongly"""
    owner = np.full((d.h4, d.w4), -1, np.int32)
    for k, cu in enumerate(d.cu):
        if cu["tree"] != abi.TREE_CHROMA:
            owner[int(cu["y"]) >> 2:(int(cu["y"]) + int(cu["h"])) >> 2, int(cu["x"]) >> 2:(int(cu["x"]) + int(cu["w"])) >> 2] = k
    idx = d.motion.reshape(d.h4, d.w4)["ref_idx"].astype(np.int32)
    n = 0
    for l in range(2):
        il = idx[:, :, l]
        poc = np.array(list(d.hdr.ref_poc[l]), np.int64)[np.maximum(il, 0)]
        for a, b in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[1:, :], np.s_[:-1, :])):
            n += int(((owner[a] != owner[b]) & (il[a] >= 0) & (il[b] >= 0) & (il[a] != il[b]) & (poc[a] == poc[b])).sum())
    return n


MODE_NAMES = {abi.MC_UNI: "uni", abi.MC_BI: "bi", abi.MC_BDOF: "bdof", abi.MC_DMVR: "dmvr", abi.MC_DMVR_BDOF: "dmvr_bdof", abi.MC_AFFINE: "affine", abi.MC_SBTMVP: "sbtmvp", abi.MC_GEO: "gpm"}


def _lists_present(c, d, refs, st):
    cu = _inter(d)
    used, high = set(), {}
    for u in cu:
        ix = cu_indices(d, u)
        used.update(ix)
        m = int(u["mc_mode"])
        high[m] = high.get(m, 0) + (1 if max(i for _, i in ix) >= 2 else 0)
    for l in range(2):
        if int(d.hdr.num_ref[l]) == abi.VVR_MAX_REFS:
            assert (l, abi.VVR_MAX_REFS - 1) in used, "index 15 of list %d is not used" % l
    assert set(c.modes) <= set(high), (sorted(c.modes), sorted(high))
    assert all(n > 0 for n in high.values()), "a mode without an index of 2 or more: %r" % high
    edges = same_picture_other_index(d)
    assert edges > 0, "no CU edge between cells that reach one picture through different indices"
    c.found = dict(inter_cus=len(cu), cus_with_index_2_or_more=sum(1 for u in cu if max(i for _, i in cu_indices(d, u)) >= 2), highest_index=max(i for _, i in used),
                   high_index_cus_by_mode={MODE_NAMES[m]: n for m, n in sorted(high.items())}, edges_same_picture_other_index=edges)
    if d.wp is not None:       # one picture at two indices of a list, both used, with different weights
        n = 0
        for l in range(2):
            for i in range(int(d.hdr.num_ref[l])):
                for j in range(i):
                    if d.hdr.ref_poc[l][i] == d.hdr.ref_poc[l][j] and (l, i) in used and (l, j) in used:
                        n += any((int(d.wp.e[l][i][k].present), int(d.wp.e[l][i][k].weight), int(d.wp.e[l][i][k].offset)) != (int(d.wp.e[l][j][k].present), int(d.wp.e[l][j][k].weight), int(d.wp.e[l][j][k].offset)) for k in range(3))
        assert n > 0, "no picture with two sets of weights"
        c.found["index_pairs_one_picture_two_weights"] = n
    if d.rpr is not None:
        n = sum(1 for u in cu if any(i >= 2 and d.rpr.ref[l][i].scaled for l, i in cu_indices(d, u)))
        ratios = {int(d.rpr.ref[l][i].ratio[0]) for l, i in used if i >= 2 and d.rpr.ref[l][i].scaled}
        assert n > 0 and ratios == {1 << 13, 1 << 15}, (n, sorted(ratios))
        c.found["cus_with_a_scaled_picture_at_index_2_or_more"] = n
    # the high indices decide the prediction itself (before any filter): the same records with every index folded to index & 1
    d2, refs2 = c.make(extreme=False)
    assert differ(st(refdrv.STOP_AFTER_RECO), refdrv.oracle_reconstruct(d2, refs2, flags=refdrv.STOP_AFTER_RECO)), "the prediction does not depend on the high indices"


def _list_case(id, tools, seed, n0, n1, modes, W=256, H=128, l2=7, bd=10, cf=1, slice_type=B, derive_lfp=False, post=None, **kw):
    @case(id, "reference_lists", _lists_present, derive_lfp=derive_lfp, bd=bd, cf=cf, l2=l2)
    def make(extreme=True):
        d, refs = list_picture(W, H, l2, seed, tools, n0, n1, slice_type=slice_type, bd=bd, cf=cf, **kw)
        if post:
            post(d, extreme)
        return (d if extreme else fold_indices(d)), refs
    CASES[-1].modes = modes


EVERY_MODE = (abi.MC_UNI, abi.MC_BI, abi.MC_BDOF, abi.MC_DMVR_BDOF, abi.MC_AFFINE, abi.MC_SBTMVP, abi.MC_GEO)
LISTS = dict(p_intra=0.1, p_affine=0.2, p_sbtmvp=0.15, p_ciip=0.1, p_geo=0.15, p_bcw=0.2, p_bi=0.7, p_coded=0.3, p_coded_chroma=0.2, p_split_scale=1.2)
_list_case("lists_16_16_every_inter_tool", TOOLS_A, 3401, 16, 16, EVERY_MODE, derive_lfp=True, **LISTS)
_list_case("lists_16_9_wp_lmcs", TOOLS_A | abi.TOOL_WP | abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE, 3402, 16, 9, (abi.MC_UNI, abi.MC_BI, abi.MC_AFFINE, abi.MC_SBTMVP, abi.MC_GEO), l2=6, **LISTS)
_list_case("lists_16_p_wp", TOOLS_A | abi.TOOL_WP, 3403, 16, 0, (abi.MC_UNI, abi.MC_AFFINE, abi.MC_SBTMVP), slice_type=P, l2=6, **LISTS)
_list_case("lists_5_16_bdof_dmvr_small_cus", no_filters(TOOLS_DB), 3404, 5, 16, (abi.MC_BDOF, abi.MC_DMVR_BDOF), p_intra=0.0, p_bi=1.0, mv_sigma=3.0, min_cu_log2=2, p_split_scale=1.3, p_coded=0.0, p_coded_chroma=0.0)
_list_case("lists_16_16_8bit_ctu32", TOOLS_A, 3603, 16, 16, EVERY_MODE, W=200, H=136, l2=5, bd=8, derive_lfp=True, **LISTS)
_list_case("lists_16_16_400", TOOLS_A, 3613, 16, 16, EVERY_MODE, l2=6, cf=0, **LISTS)
_list_case("lists_16_16_scaled_pictures_at_high_indices", no_filters(TOOLS_A), 3407, 16, 16, (abi.MC_UNI, abi.MC_BI, abi.MC_AFFINE, abi.MC_SBTMVP, abi.MC_GEO), l2=6,
           scaled={3: dict(ratio=(1 << 13, 1 << 13), size=(128, 64)), 6: dict(ratio=(1 << 15, 1 << 15), size=(512, 256))}, **dict(LISTS, p_coded=0.0, p_coded_chroma=0.0))


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# motion vectors over the 18-bit range: beyond the window an encoder's clip leaves them in (Mv.cpp:64), up to the ends of the storage range.
# What this family can show: for a plain block the decoder's clip and a clamped read give the same samples wherever the vector points.  The vector's size and
# the clip's position change the result where DMVR start vectors are clipped against the CU, SbTMVP vectors against the sub-block, affine vectors per
# sub-block and chroma at the halved vector; with scaled reference pictures (no clip at all); in the refined vectors handed back as collocated motion; in the
# edge parameters derived on the device; and in every integer that holds position * 16 + vector on the way.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
MV_MIN, MV_MAX = -(1 << 17), (1 << 17) - 1


def cu_vectors(d, cu):
    """(x, y, mvx, mvy) of the vectors the prediction of a CU starts from, with the position the clip window is taken at: the CU's own (affine: its first control
    point), its GPM partitions', its SbTMVP sub-blocks' in the motion field"""
    x, y, m = int(cu["x"]), int(cu["y"]), int(cu["mc_mode"])
    if m == abi.MC_GEO:
        return [(x, y, int(v[0]), int(v[1])) for v in cu["geo_mv"]]
    if m == abi.MC_SBTMVP:
        cells = cu_cells(d, cu)
        return [(x + 4 * i, y + 4 * j, int(cells["mv"][j, i, l, 0]), int(cells["mv"][j, i, l, 1])) for j in range(0, cells.shape[0], 2) for i in range(0, cells.shape[1], 2)
                for l in range(2) if cells["ref_idx"][j, i, l] >= 0]
    return [(x, y, int(cu["mv"][l, 0, 0]), int(cu["mv"][l, 0, 1])) for l in range(2) if cu["ref_idx"][l] >= 0]


def window_sides(d, x, y, mvx, mvy):
    """through which sides a vector leaves the window of clipMvInPic (Mv.cpp:64): (left, right, top, bottom)"""
    W, H, ctu, off = int(d.hdr.width), int(d.hdr.height), 1 << int(d.hdr.log2_ctu), 8
    return (mvx < (-ctu - off - x + 1) * 16, mvx > (W + off - x - 1) * 16, mvy < (-ctu - off - y + 1) * 16, mvy > (H + off - y - 1) * 16)


def _tally(d, keys):
    """per key of `keys(cu)`: [vectors inside the window, vectors outside], and the vectors leaving per side"""
    sides, by = [0, 0, 0, 0], {}
    for cu in _inter(d):
        for v in cu_vectors(d, cu):
            s = window_sides(d, *v)
            for k in range(4):
                sides[k] += int(s[k])
            for key in keys(cu):
                by.setdefault(key, [0, 0])[1 if any(s) else 0] += 1
    return sides, by


def _mode_keys(cu):
    keys = [MODE_NAMES[int(cu["mc_mode"])]]
    if cu["flags"] & abi.CU_CIIP:
        keys.append("ciip")
    if cu["flags"] & abi.CU_AFFINE:
        keys.append("affine_6p" if cu["flags"] & abi.CU_AFFINE_6P else "affine_4p")
    return keys


def _mv_mix_present(c, d, refs, st):
    sides, by = _tally(d, _mode_keys)
    assert all(n > 0 for n in sides), "no vector leaves through one of the sides (left, right, top, bottom): %r" % sides
    for key in c.modes:
        assert key in by and by[key][0] > 0 and by[key][1] > 0, "%s: [inside, outside] = %r" % (key, by.get(key))
    if d.wp is not None:
        assert any(d.wp.e[l][i][k].present for l in range(2) for i in range(2) for k in range(3))
    if d.hdr.wrap_offset:
        assert sides[2] > 0 and sides[3] > 0
    c.found = dict(vectors_leaving_left_right_top_bottom=sides, inside_outside_by_mode={k: by[k] for k in sorted(by)})


def _mv_limits_present(c, d, refs, st):
    """each of -2^17, -2^17 + k, 2^17 - 1 - k, 2^17 - 1 (0 < k < 32) among the used vectors, horizontally and vertically"""
    n = np.zeros((2, 4), np.int64)
    for cu in _inter(d):
        for v in cu_vectors(d, cu):
            for comp in range(2):
                m = v[2 + comp]
                for k, hit in enumerate((m == MV_MIN, MV_MIN < m < MV_MIN + 32, MV_MAX - 32 < m < MV_MAX, m == MV_MAX)):
                    n[comp, k] += int(hit)
    assert (n > 0).all(), n.tolist()
    c.found = dict(x_at_min_nearmin_nearmax_max=n[0].tolist(), y_at_min_nearmin_nearmax_max=n[1].tolist())


def near_limit(v):
    return v <= MV_MIN + 32 or v >= MV_MAX - 32


def _mv_dmvr_present(c, d, refs, st):
    """a refined vector that the clamp to the storage range can reach: a sub-block with a non-zero delta in a direction in which one of its lists starts within
    32 units of the limit"""
    st(0)
    assert st.dmvr is not None and len(st.dmvr) == d.num_dmvr
    n = moved = 0
    for cu in _inter(d):
        if int(cu["mc_mode"]) not in (abi.MC_DMVR, abi.MC_DMVR_BDOF):
            continue
        nsb = ((int(cu["w"]) + 15) // 16) * ((int(cu["h"]) + 15) // 16)
        for dm in st.dmvr[int(cu["dmvr_off"]):int(cu["dmvr_off"]) + nsb]:
            moved += int(dm.any())
            n += sum(1 for comp in range(2) if dm[comp] != 0 and any(near_limit(int(cu["mv"][l, 0, comp])) for l in range(2)))
    assert n > 0, "no refined sub-block next to the limit (%d refined at all)" % moved
    c.found = dict(dmvr_sub_blocks=int(d.num_dmvr), refined=moved, refined_in_a_direction_next_to_the_limit=n)


def dmvr_to_the_limit(d):
    """one component of one list of every DMVR CU to within 32 units of an end of the range (a whole sample, the step of the integer search, more often than not), in the CU record and in its cells of the motion field; the other list
    stays inside the picture, so the search has something to match and the refined vector can run into the clamp"""
    k = 0
    for i in np.nonzero((d.cu["pred_mode"] == abi.PRED_INTER) & ((d.cu["mc_mode"] == abi.MC_DMVR) | (d.cu["mc_mode"] == abi.MC_DMVR_BDOF)))[0]:
        l, comp, neg, r = k & 1, (k >> 1) & 1, (k >> 2) & 1, (16, 1, 16, 2, 16, 4, 16, 8, 16, 32)[(k >> 3) % 10]
        v = MV_MIN + r if neg else MV_MAX - r
        d.cu["mv"][i, l, 0, comp] = v
        cu_cells(d, d.cu[i])["mv"][:, :, l, comp] = v
        k += 1
    return d


def _mv_rpr_present(c, d, refs, st):
    n = out = at_end = 0
    for cu in _inter(d):
        if not any(d.rpr.ref[l][i].scaled for l, i in cu_indices(d, cu)):
            continue
        n += 1
        vs = cu_vectors(d, cu)
        out += int(any(any(window_sides(d, *v)) for v in vs))
        at_end += int(any(m in (MV_MIN, MV_MAX) for v in vs for m in v[2:]))
    assert out > 0 and at_end > 0, (n, out, at_end)
    c.found = dict(cus_with_a_scaled_picture=n, of_those_outside_the_window=out, of_those_at_an_end_of_the_range=at_end)


def only_the_vectors_differ(d, d2):
    """two descriptions whose stored vectors differ and whose other records are the same bytes.  (The edge tables are left out: the generator derives the
    boundary strengths from the stored vectors.)"""
    def but(a, *fields):
        b = a.copy()
        for f in fields:
            b[f] = 0
        return b.tobytes()
    assert d.cu["mv"].tobytes() != d2.cu["mv"].tobytes() or d.motion["mv"].tobytes() != d2.motion["mv"].tobytes(), "the stored vectors are the same"
    assert but(d.cu, "mv", "geo_mv") == but(d2.cu, "mv", "geo_mv"), "CU records differ in more than their vectors"
    assert but(d.motion, "mv") == but(d2.motion, "mv"), "the motion field differs in more than its vectors"
    for name in ("tu", "coef", "sao", "alf", "ctu_first_cu"):
        assert getattr(d, name).tobytes() == getattr(d2, name).tobytes(), name
    for name in ("hdr", "alf_params", "lmcs", "wp"):
        a, b = getattr(d, name, None), getattr(d2, name, None)
        assert (a is None) == (b is None) and (a is None or bytes(a) == bytes(b)), name


def _mv_case(id, present, tools, seed, modes=(), kinds=("noise", "checker"), W=256, H=128, l2=7, bd=10, cf=1, middle="vectors", derive_lfp=False, post=None, far=None, **kw):
    far = dict(mv_sigma=300.0, mv_window=500, mv_window_ver=500) if far is None else far

    @case(id, "motion_vectors", present, derive_lfp=derive_lfp, bd=bd, cf=cf, l2=l2, middle=middle)
    def make(extreme=True):
        k2 = dict(kw, **far)
        if not extreme:
            k2.update(mv_window=0, mv_window_ver=0, p_mv_limit=0.0)
        d, refs = one_picture(W, H, l2, seed, tools, kinds, bd=bd, cf=cf, **k2)
        if post and extreme:
            post(d)
        return d, refs
    CASES[-1].modes = modes


PLAIN = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_bi=0.7, p_split_scale=1.2)
MIXED = dict(PLAIN, p_intra=0.1, p_affine=0.25, p_sbtmvp=0.15, p_ciip=0.15, p_geo=0.15, p_bi=0.6)
MIXED_MODES = ("affine_4p", "affine_6p", "gpm", "ciip", "sbtmvp")
_mv_case("mv_in_and_out_uni_bi_bdof_dmvr", _mv_mix_present, TOOLS_DB, 3604, ("uni", "bi", "bdof", "dmvr_bdof"), derive_lfp=True, **dict(PLAIN, p_coded=0.3, p_coded_chroma=0.2))
_mv_case("mv_in_and_out_affine_gpm_ciip_sbtmvp_wp_ctu32", _mv_mix_present, TOOLS_A | abi.TOOL_WP, 3502, MIXED_MODES, W=200, H=136, l2=5, derive_lfp=True, **dict(MIXED, p_coded=0.3, p_coded_chroma=0.2))
_mv_case("mv_in_and_out_affine_gpm_ciip_sbtmvp_wp_8bit", _mv_mix_present, no_filters(TOOLS_A | abi.TOOL_WP), 3503, MIXED_MODES, bd=8, l2=6, **MIXED)
_mv_case("mv_in_and_out_affine_gpm_ciip_sbtmvp_400", _mv_mix_present, no_filters(TOOLS_A), 3602, MIXED_MODES, cf=0, l2=6, **MIXED)
_mv_case("mv_components_at_the_limits", _mv_limits_present, no_filters(TOOLS_A), 3505, far=dict(mv_sigma=300.0, mv_window=500, mv_window_ver=500, p_mv_limit=0.2), l2=6, p_imv_hpel=0.0, **MIXED)
_mv_case("mv_dmvr_refined_into_the_limit", _mv_dmvr_present, no_filters(TOOLS_DB), 3627, kinds=("noise", "noise"), far=dict(mv_sigma=3.0), post=dmvr_to_the_limit, p_imv_hpel=0.0,
         **dict(PLAIN, p_bi=1.0))
_mv_case("mv_wrap_around_vertical_lift", _mv_mix_present, no_filters(TOOLS_A), 3507, ("uni", "bi", "bdof", "dmvr_bdof"), far=dict(mv_sigma=300.0, mv_window=500, mv_window_ver=500), l2=6, wrap_offset=256,
         **dict(PLAIN, p_affine=0.15, p_sbtmvp=0.1, p_geo=0.1))


def _mv_rpr(name, seed, spec):
    @case("mv_scaled_picture_%s" % name, "motion_vectors", _mv_rpr_present, l2=6)
    def make(extreme=True):
        from test_oracle_vs_ref import rpr_case, ALL
        far = dict(mv_window=8200, mv_window_ver=8200) if extreme else {}
        return rpr_case(256, 128, 6, 2, seed, [spec], tools=no_filters(ALL), p_coded=0.0, p_coded_chroma=0.0, p_intra=0.1, p_affine=0.25, p_geo=0.1, p_sbtmvp=0.15, mv_sigma=4000.0, **far)
    CASES[-1].modes = ()


_mv_rpr("0_5x", 3511, dict(ratio=(1 << 13, 1 << 13), size=(128, 64)))
_mv_rpr("2x", 3512, dict(ratio=(1 << 15, 1 << 15), size=(512, 256)))

def col_motion_at_the_limit():
    """the DMVR case as a picture that stays a reference (the reference finishes the motion of such pictures only): (description, reference pictures)"""
    d, refs = [c for c in CASES if c.id == "mv_dmvr_refined_into_the_limit"][0].make()
    d.hdr.tool_flags |= abi.TOOL_STILL_REF
    return d, refs


def handed_out_on_the_limit(d, final):
    """cells of a final motion field (4x4 raster, abi.Motion) with a component on an end of the range whose start vector in the description was not there: refined
    vectors the clamp to the storage range caught"""
    start = d.motion["mv"]
    return int((np.isin(final["mv"], (MV_MIN, MV_MAX)) & ~np.isin(start, (MV_MIN, MV_MAX))).any(axis=(1, 2)).sum())


def handed_out_beyond_the_limit(final):
    """cells of a final motion field with a component outside the 18-bit range.  The reference clamps the refined vector it predicts with (InterPrediction.cpp:1956)
    and not the one DecCu::TaskFinishMotionInfo stores (DecCu.cpp:191): what is handed out as collocated motion is the unclamped sum, and the back-end's is the same"""
    return int(((final["mv"] < MV_MIN) | (final["mv"] > MV_MAX)).any(axis=(1, 2)).sum())


def long_lists_plan(pictures=24, slots=18):
    """a low-delay stream after an uploaded POC 0: picture k lists pictures k - 1 .. k - 16 in list 0 and the same in reverse in list 1; slots are taken round-robin,
    so a slot is written again while up to 16 pictures in flight still read it -> (plans, number of slots)"""
    from vvdec_amd import stream
    plans = []
    for k in range(1, pictures + 1):
        past = [(j % slots, j) for j in range(k - 1, max(-1, k - 1 - abi.VVR_MAX_REFS), -1)]
        plans.append(stream.PicPlan(poc=k, layer=0, slice_type=B, l0=[poc for _, poc in past], l1=[poc for _, poc in past[::-1]], slot=k % slots, ref_slots=(past, past[::-1])))
    return plans, slots


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# LMCS models at the ends of lmcs_data(): one bin, few bins, slopes of 1 / 8 next to 8, lmcsDeltaCrs at -7 and +7 (vvdec_amd.synth.LMCS_SHAPES)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
LM = abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE


def cscale_indices(d, mapped):
    """Reshape::calculateChromaAdjVpduNei / getPWLIdxInv (Reshape.cpp:192-280) restated for a picture of one slice and one tile: per transform unit whose chroma
    residual is scaled, the index of the search BEFORE the clamp to 15 (min_bin .. max_bin + 1), from the luma plane `mapped` (the oracle's, before the inverse
    map) -> {TU index: search index}"""
    L, W, H = d.lmcs, int(d.hdr.width), int(d.hdr.height)
    l2 = int(d.hdr.log2_ctu)
    n = min(1 << l2, 64)
    nlog = n.bit_length() - 1
    cu_at = np.full((d.h4, d.w4), -1, np.int64)
    for k, cu in enumerate(d.cu):
        if cu["tree"] != abi.TREE_CHROMA:
            cu_at[int(cu["y"]) >> 2:(int(cu["y"]) + int(cu["h"]) + 3) >> 2, int(cu["x"]) >> 2:(int(cu["x"]) + int(cu["w"]) + 3) >> 2] = k
    Y = mapped.astype(np.int64)
    pivot = [int(v) for v in L.pivot]
    out, memo = {}, {}
    for t, tu in enumerate(d.tu):
        cu = d.cu[int(tu["cu"])]
        if not (int(tu["comp_mask"]) & 6) or not (int(cu["flags"]) & abi.CU_ROOT_CBF) or not ((int(tu["cbf"]) & 6) or int(tu["joint_cbcr"])):
            continue
        w, h = (int(cu["w"]), int(cu["h"])) if int(cu["isp_mode"]) else (int(tu["w"]), int(tu["h"]))
        if (w >> 1) * (h >> 1) <= 4:
            continue
        key = (int(tu["x"]) & ~(n - 1), int(tu["y"]) & ~(n - 1))
        if key not in memo:
            tl = int(cu_at[key[1] >> 2, key[0] >> 2])
            x, y = int(d.cu["x"][tl]), int(d.cu["y"][tl])
            left = x > 0 and not (((x - 1) >> l2) == (x >> l2) and cu_at[y >> 2, (x - 1) >> 2] > tl)
            above = y > 0 and not (((y - 1) >> l2) == (y >> l2) and cu_at[(y - 1) >> 2, x >> 2] > tl)
            s = 0
            if left:
                s += int(Y[np.minimum(y + np.arange(n), H - 1), x - 1].sum())
            if above:
                s += int(Y[y - 1, np.minimum(x + np.arange(n), W - 1)].sum())
            v = (s + (1 << nlog)) >> (nlog + 1) if left and above else (s + (1 << (nlog - 1))) >> nlog if left or above else 1 << (int(d.hdr.bit_depth) - 1)
            idx = int(L.min_bin)
            while idx <= int(L.max_bin) and v >= pivot[idx + 1]:
                idx += 1
            memo[key] = idx
        out[t] = memo[key]
    return out


def longest_flat_run(a):
    a = np.asarray(a, np.int64)
    edges = np.flatnonzero(np.diff(a) != 0)
    return int(np.diff(np.concatenate([[-1], edges, [len(a) - 1]])).max())


def _lmcs_present(c, d, refs, st):
    L, bd = d.lmcs, c.bd
    lo, hi = int(L.min_bin), int(L.max_bin)
    org = (1 << bd) // 16
    cw = [int(L.pivot[i + 1]) - int(L.pivot[i]) for i in range(16)]
    assert d.hdr.tool_flags & LM == LM
    mapped = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO | refdrv.ORACLE_MAPPED_LUMA)
    idx = cscale_indices(d, mapped[0])
    n_fall, n_min, n_15 = (sum(1 for v in idx.values() if cond(v)) for cond in (lambda v: v == hi + 1, lambda v: v == lo, lambda v: min(v, 15) == 15))
    factors = {int(L.chroma_scale[min(v, 15)]) for v in idx.values()}
    fwd, inv = np.ctypeslib.as_array(L.fwd_lut)[:1 << bd], np.ctypeslib.as_array(L.inv_lut)[:1 << bd]
    c.found = dict(scaled_tus=len(idx), index_max_bin_plus_1=n_fall, index_min_bin=n_min, index_15=n_15, factors=sorted(factors),
                   fwd_flat_run=longest_flat_run(fwd), fwd_step=int(np.diff(fwd.astype(int)).max()), inv_flat_run=longest_flat_run(inv), inv_step=int(np.diff(inv.astype(int)).max()))
    shape = c.shape
    assert len(idx) > 20
    if shape in ("single_bin_low", "single_bin_high", "late_early"):      # few bins: the search starts above 0, and falls through to the zero bin
        assert lo > 0 and hi < 15 and n_fall > 0 and n_min > 0, c.found
        assert 1 << 11 in factors and int(L.chroma_scale[hi + 1]) == 1 << 11, "the zero-code-word bin's entry is not used"
    if shape in ("single_bin_low", "single_bin_high"):
        assert lo == hi and cw[lo] == 8 * org - 1
    if shape in ("single_bin_low", "single_bin_high"):      # forward slope 8 inside the bin and 0 outside, inverse slope 1 / 8
        assert c.found["fwd_step"] >= 8 and c.found["fwd_flat_run"] >= 8 and c.found["inv_flat_run"] >= 8, c.found
    if shape == "sawtooth":      # slopes of 8 and of 1 / 8 next to each other: steps and flat stretches in both tables
        assert c.found["fwd_step"] >= 8 and c.found["inv_step"] >= 8 and c.found["fwd_flat_run"] >= 8 and c.found["inv_flat_run"] >= 8, c.found
    if shape == "sawtooth":
        assert hi == 15 and n_15 > 0 and min(cw) == org >> 3 and max(cw) >= 7 * org, c.found
        assert any(cw[i] == org >> 3 and cw[i + 1] >= 7 * org for i in range(15))
    if shape == "crs_low":       # lmcsCW + lmcsDeltaCrs at OrgCW >> 3: the largest factor there is
        assert int(L.model_delta_crs) == -7 and 16384 in factors and max(int(v) for v in L.chroma_scale) == 16384, c.found
        # |residual| is clipped to 1 << bd before the factor (AreaBuf::scaleSignal, Buffer.cpp:412): 8 << bd at most comes out, which the +-32768 clip
        # behind it never sees; what saturated levels at this factor do reach is the sample clip on both sides, in both chroma planes
        assert int(np.abs(d.coef).max()) == 32767 and holds_both_ends(st(refdrv.STOP_AFTER_RECO)[1:], bd)
    if shape == "crs_high":      # lmcsCW + lmcsDeltaCrs at ( OrgCW << 3 ) - 1: the smallest
        assert int(L.model_delta_crs) == 7 and min(int(v) for v in L.chroma_scale) == 256 and 256 in factors, c.found
        assert int(np.abs(d.coef).max()) == 32767
    if shape == "nearly_identity_full":
        assert (lo, hi) == (0, 15) and int(L.pivot[16]) == (1 << bd) - 1 and cw == [org] * 15 + [org - 1]
    if c.slice_type == B:
        assert int(((d.cu["flags"] & abi.CU_CIIP) != 0).sum()) > 0 and int((d.cu["pred_mode"] == abi.PRED_INTRA).sum()) > 0
        assert min(int(r[0].min()) for r in refs.values()) == 0 and max(int(r[0].max()) for r in refs.values()) == (1 << bd) - 1
    if not (int(d.hdr.tool_flags) & abi.TOOL_DEBLOCK_OFF):
        assert differ(st(refdrv.STOP_AFTER_DBK), st(refdrv.STOP_AFTER_RECO)), "deblocking changes nothing"


LMCS_MIX = dict(RESI, p_jccr=0.2, p_cclm=0.2)
LMCS_MIX_B = dict(LMCS_MIX, p_ciip=0.3, p_intra=0.3, p_bi=0.6)


def _lmcs_case(id, shape, seed, slice_type, tools, W=256, H=128, l2=7, bd=10, saturate=False, kinds=("noise", "checker"), **kw):
    @case(id, "lmcs_model", _lmcs_present, bd=bd, l2=l2)
    def make(extreme=True):
        d, refs = one_picture(W, H, l2, seed, tools | LM, kinds, slice_type=slice_type, bd=bd, lmcs_shape=synth.LMCS_SHAPES[shape] if extreme else 0,
                              **dict(LMCS_MIX if slice_type == I else LMCS_MIX_B, **kw))
        if saturate and extreme:
            _saturate(d)
        return d, refs
    CASES[-1].shape, CASES[-1].slice_type = shape, slice_type


_lmcs_case("lmcs_single_bin_low_i", "single_bin_low", 3701, I, TOOLS_I)
_lmcs_case("lmcs_single_bin_high_b_ctu64", "single_bin_high", 3702, B, TOOLS_A, l2=6)
_lmcs_case("lmcs_late_early_b_ctu64", "late_early", 3704, B, TOOLS_A, l2=6, kinds=("flat_max", "flat_zero"), p_bi=0.2)    # (flat pictures: the mean of 128 neighbouring samples reaches both ends)
_lmcs_case("lmcs_sawtooth_i", "sawtooth", 3704, I, TOOLS_I)
_lmcs_case("lmcs_sawtooth_b_8bit_ctu64", "sawtooth", 3705, B, no_filters(TOOLS_A), l2=6, bd=8)
_lmcs_case("lmcs_crs_low_i_saturated_levels", "crs_low", 3706, I, TOOLS_I, saturate=True)
_lmcs_case("lmcs_crs_high_b_saturated_levels_ctu32", "crs_high", 3707, B, no_filters(TOOLS_A), W=200, H=136, l2=5, saturate=True)
_lmcs_case("lmcs_nearly_identity_full_b", "nearly_identity_full", 3708, B, no_filters(TOOLS_A), l2=6)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# chroma QPs that are not the luma QP: mapping tables, PPS / slice / CU-level offsets, the joint Cb-Cr table (vvdec_amd.synth.ChromaQpModel)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def chroma_qp_cells(d):
    """per 4x4 luma cell the [Cb, Cr] QP of the transform unit that owns its chroma (ISP: the last one of the CU), -1 where there is none"""
    q = np.full((d.h4, d.w4, 2), -1, np.int32)
    for tu in d.tu:
        if not int(tu["comp_mask"]) & 6:
            continue
        cu = d.cu[int(tu["cu"])]
        x, y, w, h = (int(cu[k]) for k in "xywh") if int(cu["isp_mode"]) else (int(tu[k]) for k in "xywh")
        q[y >> 2:(y + h + 3) >> 2, x >> 2:(x + w + 3) >> 2] = tu["qp"][1:3]
    return q


def _cqp_present(c, d, refs, st):
    m = d.chroma_qp_model
    qpbd = 6 * (c.bd - 8)
    own, joint = synth.model_chroma_qps(d)
    ch = (d.tu["comp_mask"] & 6) != 0
    j3 = d.tu["joint_cbcr"] == 3
    q = d.tu["qp"].astype(np.int32)
    # the description holds what the model gives (the generator's own restatement of QpParam, once more in Python; the reference's QpParam is asked on the CPU leg)
    assert np.array_equal(q[ch & ~j3][:, 1:3], own[ch & ~j3]) and np.array_equal(q[ch & j3][:, 1], joint[ch & j3]) and np.array_equal(q[ch & j3][:, 2], joint[ch & j3])
    cu_of = d.tu["cu"].astype(np.int64)
    n_cb_cr = int((ch & (q[:, 1] != q[:, 2])).sum())
    n_not_luma = int((ch & ((q[:, 1] != q[:, 0]) | (q[:, 2] != q[:, 0]))).sum())
    n_joint = int((ch & j3 & (joint != own[:, 0]) & (joint != own[:, 1])).sum())
    modes = {int(v) for v in d.tu["joint_cbcr"][ch]}
    apart = ch & (np.abs(own[:, 0] - own[:, 1]) >= 6) & (np.abs(own[:, 0] - joint) >= 6) & (np.abs(own[:, 1] - joint) >= 6)
    n_isp = int((ch & (q[:, 1] != q[:, 0]) & (d.cu["isp_mode"][cu_of] != 0)).sum())
    n_tree = int((ch & (q[:, 1] != q[:, 0]) & (d.cu["tree"][cu_of] == abi.TREE_CHROMA)).sum())
    cells = chroma_qp_cells(d)
    far = 0
    for dr in range(2):
        a, b = (cells[:, 1:], cells[:, :-1]) if dr == 0 else (cells[1:, :], cells[:-1, :])
        bs = d.lfp[dr]["bs"].reshape(d.h4, d.w4)
        bs = bs[:, 1:] if dr == 0 else bs[1:, :]
        for k in range(2):
            far += int(((a[..., k] >= 0) & (b[..., k] >= 0) & (np.abs(a[..., k] - b[..., k]) >= 12) & (((bs >> (2 * (k + 1))) & 3) > 0)).sum())
    c.found = dict(chroma_tus=int(ch.sum()), cb_differs_from_cr=n_cb_cr, chroma_differs_from_luma=n_not_luma, joint_mode_3_differs_from_both=n_joint,
                   cb_cr_joint_pairwise_6_apart=int(apart.sum()), isp_tus_among_them=n_isp, chroma_tree_tus_among_them=n_tree, filtered_chroma_edges_12_apart=far,
                   chroma_qp_min_max=[int(q[ch][:, 1:3].min()), int(q[ch][:, 1:3].max())])
    assert n_cb_cr > 0 and n_not_luma > 0, c.found
    want = c.want
    if "jccr" in want:
        assert modes >= {0, 1, 2, 3} and n_joint > 0, (sorted(modes), c.found)
        assert 2 * int(apart.sum()) > int(ch.sum()), "Cb, Cr and joint QPs are not 6 apart on most transform units: %r" % c.found
        b = _blocks(d)
        assert {abi.MTS_SKIP, abi.MTS_DCT2} <= {int(tu["mts_idx"][comp]) for w, h, comp, tu, cu in b if comp} and any(int(cu["bdpcm"][1]) for w, h, comp, tu, cu in b if comp)
        assert any(int(cu["lfnst_idx"]) for w, h, comp, tu, cu in b) and far > 0
    if "clip" in want:
        lum = q[ch][:, 0] - qpbd
        assert int(lum.min()) >= 24 and int(lum.max()) <= 40
        for k in (1, 2):
            assert int(q[ch][:, k].min()) == 0 and int(q[ch][:, k].max()) == 63 + qpbd, c.found
        assert far > 0
    if "dual_tree" in want:
        assert n_tree > 0 and int((d.cu["tree"] == abi.TREE_LUMA).sum()) > 0, c.found
    if "isp" in want:
        assert n_isp > 0, c.found
    if "deblock" in want:
        # luma QPs at which tc = 0 (below 18 with the offsets at 0: tcTable, LoopFilter.cpp:73), chroma QPs at which the chroma filters run
        assert int(d.cu["qp"].max()) <= 17 and int(q[ch][:, 1:3].min()) - qpbd >= 40 and all(int(v) == 0 for v in d.hdr.deblock_tc_offset_div2)
        a, bb = st(refdrv.STOP_AFTER_RECO), st(refdrv.STOP_AFTER_DBK)
        assert not differ(a[:1], bb[:1]), "the luma deblocking is not off at these QPs"
        for k in (1, 2):
            chc = a[k] != bb[k]
            gy, gx = np.mgrid[0:chc.shape[0], 0:chc.shape[1]]
            one_dir = (((gx & 7) == 1) | ((gx & 7) == 2) | ((gx & 7) == 5) | ((gx & 7) == 6)) & ((gy & 7) >= 3) & ((gy & 7) <= 4)
            assert int((chc & one_dir).sum()) > 0, "no strong chroma filter in component %d" % k


CQP_MIX = dict(RESI, p_coded_chroma=0.9, p_jccr=0.5, p_cclm=0.2)


def _cqp_case(id, want, seed, model, slice_type, tools, flavour=0, W=256, H=128, l2=7, bd=10, kinds=("noise", "checker"), post=None, **kw):
    @case(id, "chroma_qp", _cqp_present, derive_lfp=True, bd=bd, l2=l2)
    def make(extreme=True):
        d, refs = one_picture(W, H, l2, seed, tools, kinds, slice_type=slice_type, bd=bd, chroma_qp_model=model if extreme else 0, chroma_qp_flavour=flavour if extreme else 0,
                              **dict(CQP_MIX, **kw))
        if post:
            post(d, extreme)
        return d, refs
    CASES[-1].want = want


def _zero_tc_offsets(d, extreme):
    for k in range(3):
        d.hdr.deblock_tc_offset_div2[k] = d.hdr.deblock_beta_offset_div2[k] = 0


_cqp_case("chroma_qp_every_residual_tool_jccr_b", ("jccr",), 3801, 41, B, TOOLS_A, p_sbt=0.2, p_intra=0.4)
_cqp_case("chroma_qp_8bit_ctu64_no_dep_quant_scaling_lists", ("jccr",), 3802, 42, B, (TOOLS_A & ~abi.TOOL_DEP_QUANT) | abi.TOOL_SCALING_LIST, l2=6, bd=8, p_sbt=0.2, p_intra=0.4)
_cqp_case("chroma_qp_both_clips_luma_in_the_middle", ("clip",), 3803, 43, I, TOOLS_I, flavour=synth.CQP_CLIP)
_cqp_case("chroma_qp_dual_tree", ("dual_tree",), 3804, 44, I, TOOLS_I, l2=6, dual_tree=1.0)
_cqp_case("chroma_qp_isp_last_tu_ctu32", ("isp",), 3805, 45, I, TOOLS_I, W=200, H=136, l2=5, p_isp=0.6, p_mrl=0.0, p_bdpcm=0.0, p_mip=0.0)
_cqp_case("chroma_qp_deblock_steps_luma_off_chroma_strong", ("deblock",), 3808, 46, B, TOOLS, flavour=synth.CQP_LIFTED, kinds=("steps",), post=_zero_tc_offsets, base_qp=14,
          **dict(COPY, p_coded=0.5, p_coded_chroma=0.4, p_split_scale=0.45, p_small_corner=1.0, p_jccr=0.1))


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# min_qp_ts above 4: transform-skip and BDPCM blocks below, on and above the bound (per / rem of the raised QP)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _ts_present(c, d, refs, st):
    bound = int(d.hdr.min_qp_ts)
    assert bound == c.min_qp_ts
    n = {(ch, g): 0 for ch in ("luma", "chroma") for g in ("below", "on", "above")}
    bdpcm = {"luma": 0, "chroma": 0}
    for w, h, comp, tu, cu in _blocks(d):
        if int(tu["mts_idx"][comp]) != abi.MTS_SKIP:
            continue
        qp, ch = int(tu["qp"][comp]), "chroma" if comp else "luma"
        n[(ch, "below" if qp < bound else "on" if qp == bound else "above")] += 1
        bdpcm[ch] += int(cu["bdpcm"][1 if comp else 0] != 0)
    c.found = dict({"%s_%s" % k: v for k, v in n.items()}, bdpcm_luma=bdpcm["luma"], bdpcm_chroma=bdpcm["chroma"])
    assert all(v > 0 for v in n.values()) and bdpcm["luma"] > 0 and bdpcm["chroma"] > 0, c.found


def _whole_range(d, bound):
    """CU QPs over -QpBdOffset .. 63, every third one on the bound (identity chroma mapping: TU.qp of all three components is QP + QpBdOffset)"""
    qpbd = 6 * (int(d.hdr.bit_depth) - 8)
    k = np.arange(len(d.cu))
    synth.rewrite_qp(d, np.where(k % 3 == 0, bound - qpbd, (k * 7) % (64 + qpbd) - qpbd))


def _ts_case(id, seed, min_qp_ts, bd, tools, l2=7, **kw):
    @case(id, "ts_min_qp", _ts_present, bd=bd, l2=l2)
    def make(extreme=True):
        d, refs = one_picture(256, 128, l2, seed, tools, slice_type=I, bd=bd, min_qp_ts=min_qp_ts if extreme else 4, **dict(RESI, p_ts=0.5, p_bdpcm=0.4, p_split_scale=1.4, **kw))
        _whole_range(d, min_qp_ts)
        return d, refs
    CASES[-1].min_qp_ts = min_qp_ts


_ts_case("ts_min_qp_16_10bit", 3901, 16, 10, TOOLS_I)
_ts_case("ts_min_qp_52_10bit_ctu64_no_dep_quant", 3902, 52, 10, TOOLS_I & ~abi.TOOL_DEP_QUANT, l2=6)
_ts_case("ts_min_qp_10_8bit_scaling_lists", 3903, 10, 8, TOOLS_I | abi.TOOL_SCALING_LIST)


FAMILIES = sorted({c.family for c in CASES})

# three-picture streams from an uploaded extreme picture (POC 0), through _run_stream: kind of the picture, tools, seed, size, CTU, generator settings
STREAMS = [("bdof_checker", "checker", TOOLS_B, 3301), ("dmvr_bdof_steps", "steps", TOOLS_DB, 3302)]
STREAM_GEO = dict(W=128, H=64, frames=3, gop=2, log2_ctu=6)
STREAM_MIX = dict(p_bi=1.0, mv_sigma=2.0, p_coded=0.2, p_intra=0.0)


def plane_count(c):
    return 3 if c.cf else 1
