"""k_itrans on packed 16-bit pairs (GPU, -m gpu): small pictures through the C ABI against the CPU oracle, bit-exact, with generator settings that force the
blocks where the paired layout of the levels, the intermediate and the basis rows can go wrong.  Every case asserts, from the picture's own TU / CU records, that
the blocks it is about are there; every picture holds inter (added onto the prediction) and intra (stored) blocks, so both modes share a launch."""
import numpy as np
import pytest

from vvdec_amd import abi, synth
from test_gpu_parity import _run_stream, TOOLS_A

pytestmark = pytest.mark.gpu

T = TOOLS_A | abi.TOOL_IMPLICIT_MTS


def _blocks(d):
    """(bw, bh, comp, tu record, cu record) of every coded transform block of a picture, as vvr_prepare lists them (copies: the picture's records
    lie in pinned memory that goes away with the reconstructor)"""
    out = []
    tus, cus = np.array(d.tu, copy=True), np.array(d.cu, copy=True)
    for tu in tus:
        cu = cus[int(tu["cu"])]
        if not int(cu["flags"]) & abi.CU_ROOT_CBF:
            continue
        for c in range(3):
            if not int(tu["comp_mask"]) & (1 << c):
                continue
            j = int(tu["joint_cbcr"])
            if c and j:
                if c != (1 if j >> 1 else 2):
                    continue
            elif not int(tu["cbf"]) & (1 << c):
                continue
            isp_c = c and int(cu["isp_mode"])
            w, h = (int(cu["w"]), int(cu["h"])) if isp_c else (int(tu["w"]), int(tu["h"]))
            out.append((w >> (1 if c else 0), h >> (1 if c else 0), c, tu, cu))
    return out


def _saturate(d):
    """every coded level to +-32767: dequantisation, the BDPCM sums, LFNST, both passes and the residual all run into their clips"""
    nz = d.coef != 0
    d.coef[nz] = np.where(d.coef[nz] > 0, 32767, -32767).astype(np.int16)


def _dst7_4x4_and_2xn(b):
    return (sum(1 for w, h, c, tu, cu in b if w == 4 and h == 4 and c == 0 and int(tu["tr_type"][0]) != 0 and int(tu["mts_idx"][0]) != abi.MTS_SKIP) > 0
            and sum(1 for w, h, c, tu, cu in b if c and (w == 2 or h == 2)) > 0)


def _isp_1d(b):
    return sum(1 for w, h, c, tu, cu in b if (w, h) == (1, 16)) > 0 and sum(1 for w, h, c, tu, cu in b if (w, h) == (16, 1)) > 0


def _odd_extents(b):
    ts = lambda tu, c: int(tu["mts_idx"][c]) == abi.MTS_SKIP
    return (sum(1 for w, h, c, tu, cu in b if not ts(tu, c) and int(tu["max_scan_x"][c]) % 2 == 0 and int(tu["max_scan_x"][c]) > 0 and min(w, h) >= 4) > 0
            and sum(1 for w, h, c, tu, cu in b if not ts(tu, c) and int(tu["max_scan_y"][c]) % 2 == 0 and int(tu["max_scan_y"][c]) > 0 and min(w, h) >= 4) > 0)


def _mts32(b):
    return sum(1 for w, h, c, tu, cu in b if c == 0 and (w == 32 and int(tu["tr_type"][0]) & 3 or h == 32 and int(tu["tr_type"][0]) >> 2)) > 0


def _size64(b):
    s = {(w, h) for w, h, c, tu, cu in b}
    return (64, 64) in s and (64, 16) in s and (16, 64) in s


def _lfnst(b):
    l = [(w, h, c, cu) for w, h, c, tu, cu in b if int(cu["lfnst_idx"]) and int(tu["mts_idx"][c]) != abi.MTS_SKIP]
    return (sum(1 for w, h, c, cu in l if min(w, h) == 4) > 0 and sum(1 for w, h, c, cu in l if min(w, h) >= 8) > 0
            and sum(1 for w, h, c, cu in l if c == 0 and int(cu["flags"]) & abi.CU_MIP) > 0
            and sum(1 for w, h, c, cu in l if c == 0 and 34 < int(cu["intra_dir"][0]) < 67) > 0 and sum(1 for w, h, c, cu in l if c == 0 and 2 <= int(cu["intra_dir"][0]) <= 34) > 0)


def _bdpcm_ts(b):
    return ({int(cu["bdpcm"][0]) for w, h, c, tu, cu in b if c == 0} >= {1, 2} and {int(cu["bdpcm"][1]) for w, h, c, tu, cu in b if c} >= {1, 2}
            and sum(1 for w, h, c, tu, cu in b if (w, h) == (32, 32) and int(tu["mts_idx"][c]) == abi.MTS_SKIP) > 0)


def _jccr(b):
    return {int(tu["joint_cbcr"]) for w, h, c, tu, cu in b if c} >= {1, 2, 3}


def _dc_only(b):
    return sum(1 for w, h, c, tu, cu in b if int(tu["max_scan_x"][c]) == 0 and int(tu["max_scan_y"][c]) == 0 and int(tu["tr_type"][c]) == 0
               and int(tu["mts_idx"][c]) != abi.MTS_SKIP and not int(cu["lfnst_idx"])) > 0


def _lfnst_and_plain(b):
    """coded blocks with LFNST (exempt from the scaling lists or not, by the tool flag) and without"""
    ts = lambda tu, c: int(tu["mts_idx"][c]) == abi.MTS_SKIP
    lf = lambda c, cu: int(cu["lfnst_idx"]) and (c == 0 or int(cu["tree"]) != abi.TREE_JOINT)
    return (sum(1 for w, h, c, tu, cu in b if lf(c, cu) and not ts(tu, c)) > 0 and sum(1 for w, h, c, tu, cu in b if not lf(c, cu) and not ts(tu, c)) > 0)


def _scaling_lists(b):
    """LFNST and plain blocks, transform skip (flat) beside them, rectangular and square blocks of intra and inter CUs (the list types)"""
    return (_lfnst_and_plain(b) and sum(1 for w, h, c, tu, cu in b if w != h) > 0 and sum(1 for w, h, c, tu, cu in b if w == h) > 0
            and {int(cu["pred_mode"]) for w, h, c, tu, cu in b} >= {abi.PRED_INTRA, abi.PRED_INTER} and {c for w, h, c, tu, cu in b} == {0, 1, 2})


def _lfnst_small_and_large(b):
    l = [(w, h) for w, h, c, tu, cu in b if int(cu["lfnst_idx"]) and int(tu["mts_idx"][c]) != abi.MTS_SKIP and (c == 0 or int(cu["tree"]) != abi.TREE_JOINT)]
    return sum(1 for w, h in l if min(w, h) == 4) > 0 and sum(1 for w, h in l if min(w, h) >= 8) > 0


def _bdpcm_both_and_ts(b):
    return ({int(cu["bdpcm"][0]) for w, h, c, tu, cu in b if c == 0} >= {1, 2} and {int(cu["bdpcm"][1]) for w, h, c, tu, cu in b if c} >= {1, 2}
            and sum(1 for w, h, c, tu, cu in b if int(tu["mts_idx"][c]) == abi.MTS_SKIP and not int(cu["bdpcm"][1 if c else 0])) > 0)


def _mts_and_ts(b):
    """without dependent quantisation: DCT-2, explicit MTS and transform-skip blocks"""
    return ({int(tu["mts_idx"][c]) for w, h, c, tu, cu in b} >= {abi.MTS_DCT2, abi.MTS_SKIP} and sum(1 for w, h, c, tu, cu in b if int(tu["mts_idx"][c]) > abi.MTS_SKIP) > 0)


SL = abi.TOOL_SCALING_LIST
CASES = [
    # id, W, H, log2_ctu, bit_depth, tools, generator settings, what must be there, levels saturated
    ("dst7_4x4_and_2xn_chroma", 128, 64, 6, 10, T, dict(min_cu_log2=2, p_split_scale=2.0, p_intra=0.3, p_sbt=0.4, p_mts=0.6, p_coded=0.9, p_coded_chroma=0.8), _dst7_4x4_and_2xn, False),
    ("isp_1x16_16x1", 256, 128, 7, 8, T, dict(dual_tree=3.0, p_isp=0.8, p_intra=0.5, p_lfnst=0.3, p_coded=0.9, p_split_scale=1.8), _isp_1d, False),
    ("odd_extents", 128, 64, 6, 8, T, dict(p_intra=0.3, p_coded=0.95, p_coded_chroma=0.9, p_small_corner=0.5), _odd_extents, False),
    ("mts_32_zero_out_16", 256, 128, 7, 10, T, dict(p_intra=0.3, p_mts=0.9, p_coded=0.95, p_split_scale=0.7, p_small_corner=0.0), _mts32, False),
    ("size_64_corner_32", 256, 128, 7, 10, T, dict(p_intra=0.3, p_coded=0.95, p_coded_chroma=0.9, p_split_scale=0.45, p_small_corner=0.0, p_ts=0.0), _size64, False),
    ("size_64_saturated", 256, 128, 7, 8, T, dict(p_intra=0.3, p_coded=0.95, p_coded_chroma=0.9, p_split_scale=0.45, p_small_corner=0.0, p_ts=0.0), _size64, True),
    ("lfnst_4_8_transposed_mip", 256, 128, 6, 10, T | abi.TOOL_LFNST, dict(dual_tree=2.0, p_intra=0.6, p_lfnst=0.8, p_mip=0.4, p_coded=0.9, p_split_scale=1.3), _lfnst, False),
    ("lfnst_saturated", 128, 64, 6, 8, T | abi.TOOL_LFNST, dict(dual_tree=2.0, p_intra=0.6, p_lfnst=0.8, p_mip=0.4, p_coded=0.9, p_split_scale=1.3), _lfnst_small_and_large, True),
    ("bdpcm_and_transform_skip", 256, 128, 7, 10, T, dict(p_intra=0.6, p_bdpcm=0.4, p_ts=0.5, p_coded=0.9, p_coded_chroma=0.8, p_split_scale=0.8), _bdpcm_ts, False),
    ("bdpcm_and_transform_skip_saturated", 256, 128, 6, 8, T, dict(p_intra=0.6, p_bdpcm=0.4, p_ts=0.5, p_coded=0.9, p_coded_chroma=0.8), _bdpcm_both_and_ts, True),
    ("joint_cbcr", 128, 64, 6, 10, T, dict(p_intra=0.3, p_jccr=0.8, p_coded_chroma=0.9), _jccr, False),
    ("joint_cbcr_sign", 128, 64, 6, 8, T | abi.TOOL_JCCR_SIGN, dict(p_intra=0.3, p_jccr=0.8, p_coded_chroma=0.9), _jccr, False),
    ("joint_cbcr_saturated", 128, 64, 7, 10, T | abi.TOOL_JCCR_SIGN, dict(p_intra=0.3, p_jccr=0.8, p_coded_chroma=0.9), _jccr, True),
    ("scaling_lists", 256, 128, 7, 10, T | abi.TOOL_LFNST | SL, dict(p_intra=0.4, p_lfnst=0.6, p_coded=0.9, p_coded_chroma=0.7, p_mts=0.3, p_ts=0.2), _scaling_lists, False),
    ("scaling_lists_not_for_lfnst", 256, 128, 6, 8, T | abi.TOOL_LFNST | SL | abi.TOOL_SCALING_LIST_NO_LFNST, dict(p_intra=0.4, p_lfnst=0.6, p_coded=0.9, p_coded_chroma=0.7), _scaling_lists, False),
    ("no_dependent_quantisation", 128, 64, 6, 10, T & ~abi.TOOL_DEP_QUANT, dict(p_intra=0.3, p_coded=0.9, p_coded_chroma=0.7, p_mts=0.3, p_ts=0.2), _mts_and_ts, False),
    ("dc_only", 128, 64, 7, 8, T, dict(p_intra=0.3, p_coded=0.9, p_coded_chroma=0.8, p_small_corner=1.0), _dc_only, False),
    ("dc_only_saturated", 128, 64, 6, 10, T, dict(p_intra=0.3, p_coded=0.9, p_coded_chroma=0.8, p_small_corner=1.0), _dc_only, True),
]


@pytest.mark.parametrize("name,W,H,log2_ctu,bit_depth,tools,kw,present,saturated", CASES, ids=[c[0] for c in CASES])
def test_packed_passes_bit_exact(built, name, W, H, log2_ctu, bit_depth, tools, kw, present, saturated):
    blocks, modes = [], set()

    def post(d):
        b = _blocks(d)
        blocks.extend(b)
        if int(d.hdr.slice_type) != abi.SLICE_I:
            modes.update("add" if int(cu["pred_mode"]) == abi.PRED_INTER else "store" for _, _, _, _, cu in b)
        if saturated:
            _saturate(d)
    _run_stream(W, H, 3, 2, 900 + len(name), tools, intra=True, log2_ctu=log2_ctu, bit_depth=bit_depth, post=post, **kw)
    assert present(blocks), "%s: the generated pictures do not hold the blocks the case is about" % name
    assert modes == {"add", "store"}, modes


def test_slices_switch_dependent_quantisation_and_scaling_lists(built):
    """the two slice bits of the dequantisation (dependent quantisation, scaling lists on) differ between the slices of a picture"""
    seen = []

    def vary(d):
        synth.vary_slices(d, 940 + d.hdr.poc)
        seen.append(len(set(int(f) & (abi.TOOL_DEP_QUANT | SL) for f in d.slices["tool_flags"])))
    _run_stream(256, 128, 3, 2, 941, T | abi.TOOL_LFNST | SL, intra=True, log2_ctu=5, num_slices=4, p_intra=0.3, p_coded=0.9, p_coded_chroma=0.7, p_lfnst=0.4, post=vary)
    assert max(seen) > 1
