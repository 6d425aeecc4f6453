"""The cases of the range-limit tests: pictures whose QPs, samples, weights and filter taps sit at the ends of what the syntax allows.

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
    def __init__(self, id, family, make, present, derive_lfp=False, bd=10, cf=1, l2=7):
        self.id, self.family, self.make, self.present, self.derive_lfp, self.bd, self.cf, self.l2 = id, family, make, present, derive_lfp, bd, cf, l2


CASES = []


def case(id, family, present, derive_lfp=False, bd=10, cf=1, l2=7):
    def reg(make):
        CASES.append(Case(id, family, make, present, derive_lfp, bd, cf, l2))
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

FAMILIES = sorted({c.family for c in CASES})

# three-picture streams from an uploaded extreme picture (POC 0), through _run_stream: kind of the picture, tools, seed, size, CTU, generator settings
STREAMS = [("bdof_checker", "checker", TOOLS_B, 3301), ("dmvr_bdof_steps", "steps", TOOLS_DB, 3302)]
STREAM_GEO = dict(W=128, H=64, frames=3, gop=2, log2_ctu=6)
STREAM_MIX = dict(p_bi=1.0, mv_sigma=2.0, p_coded=0.2, p_intra=0.0)


def plane_count(c):
    return 3 if c.cf else 1
