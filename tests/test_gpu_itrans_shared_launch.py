"""The transform blocks of the 16 and of the 32 class in one launch (k_itrans_16_32; GPU, -m gpu): small pictures through the C ABI against the CPU oracle,
bit-exact.  A workgroup of that launch holds one block of the 32 class or two of the 16 class, one per wavefront, which never meet at a barrier: the cases put
blocks that take different paths through the body next to each other.  Every case asserts, from the pictures' own TU / CU records, that the blocks it is about
are there."""
import numpy as np
import pytest

from vvdec_amd import abi, synth, stream
from test_gpu_parity import _run_stream, TOOLS_I
from test_gpu_itrans_packed import _blocks

pytestmark = pytest.mark.gpu


def _tb_classes(d):
    """number of coded transform blocks of the 16, the 32 and the 64 class of one picture (as vvr_prepare sorts them)"""
    n = [0, 0, 0]
    for w, h, c, tu, cu in _blocks(d):
        n[0 if max(w, h) <= 16 else 1 if max(w, h) <= 32 else 2] += 1
    return n


def _paths16(b):
    """blocks of the 16 class that take different paths through the body: DC only, one-dimensional (4xN / Nx4 ISP partitions), transform skip, BDPCM, LFNST, joint Cb-Cr"""
    b = [x for x in b if max(x[0], x[1]) <= 16]
    ts = lambda tu, c: int(tu["mts_idx"][c]) == abi.MTS_SKIP
    return dict(
        dc=sum(1 for w, h, c, tu, cu in b if int(tu["max_scan_x"][c]) == 0 and int(tu["max_scan_y"][c]) == 0 and int(tu["tr_type"][c]) == 0 and not ts(tu, c) and not int(cu["lfnst_idx"])),
        one_d=sum(1 for w, h, c, tu, cu in b if (w == 1 or h == 1)),
        ts=sum(1 for w, h, c, tu, cu in b if ts(tu, c) and not int(cu["bdpcm"][1 if c else 0])),
        bdpcm=sum(1 for w, h, c, tu, cu in b if int(cu["bdpcm"][1 if c else 0])),
        lfnst=sum(1 for w, h, c, tu, cu in b if int(cu["lfnst_idx"]) and not ts(tu, c) and (c == 0 or int(cu["tree"]) != abi.TREE_JOINT)),
        jccr=sum(1 for w, h, c, tu, cu in b if c and int(tu["joint_cbcr"])),
        two_d=sum(1 for w, h, c, tu, cu in b if min(w, h) >= 4 and not ts(tu, c) and (int(tu["max_scan_x"][c]) or int(tu["max_scan_y"][c]))))


T_TB = TOOLS_I | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_IMPLICIT_MTS
TB_CASES = {
    # id: (seed, CTU log2, intra pictures and intra CUs, tools, generator settings)
    # POC 0 uploaded, so every CU is an inter CU; those above 16 samples lose their residual (_no_residual_above_16): no block above 16
    "only_16_odd_count": (6100, 6, False, T_TB, dict(p_split_scale=1.5, p_coded=0.8, p_coded_chroma=0.6, p_small_corner=0.3, p_mts=0.4)),
    # CTUs of 32 that stay whole, luma alone coded: no block below 32
    "only_32": (6200, 5, False, T_TB, dict(p_split_scale=0.02, p_coded=0.9, p_coded_chroma=0.0, p_jccr=0.0, p_small_corner=0.3, p_mts=0.5)),
    "both_classes": (6300, 6, True, T_TB, dict(p_split_scale=0.9, p_intra=0.3, p_coded=0.9, p_coded_chroma=0.7, p_small_corner=0.4, p_mts=0.4)),
    "paths_side_by_side": (6400, 6, True, T_TB, dict(dual_tree=3.0, p_split_scale=1.3, p_intra=0.5, p_isp=0.4, p_lfnst=0.5, p_bdpcm=0.25, p_ts=0.3, p_jccr=0.5, p_coded=0.9, p_coded_chroma=0.8,
                                                      p_small_corner=0.6)),
}


def _no_residual_above_16(d):
    """the inter CUs wider or higher than 16 samples become CUs without a residual (cu_coded_flag 0)"""
    big = (d.cu["w"] > 16) | (d.cu["h"] > 16)
    assert (d.cu["pred_mode"][big] == abi.PRED_INTER).all()
    d.cu["flags"][big] &= ~np.uint16(abi.CU_ROOT_CBF)


def _tb_present(name, counts, paths):
    if name == "only_16_odd_count":
        return all(n[1] == 0 and n[2] == 0 for n in counts) and any(n[0] > 1 and n[0] & 1 for n in counts)
    if name == "only_32":
        return all(n[0] == 0 for n in counts) and any(n[1] > 1 for n in counts)
    if name == "both_classes":
        return any(n[0] > 2 and n[1] > 1 and n[0] & 1 for n in counts) and any(n[0] > 2 and n[1] > 1 and not n[0] & 1 for n in counts)
    return any(n[0] > 2 and n[1] > 0 for n in counts) and all(v >= 3 for v in paths.values())


def _tb_args(name):
    seed, l2, intra, tools, kw = TB_CASES[name]
    return (128, 128, 5 if not intra else 3, 4 if not intra else 2, seed, tools), dict(log2_ctu=l2, intra=intra, **kw)


@pytest.mark.parametrize("name", list(TB_CASES))
def test_transform_classes_16_and_32_in_one_launch_bit_exact(built, name):
    counts, paths = [], {}

    def post(d):
        if name == "only_16_odd_count":
            _no_residual_above_16(d)
        counts.append(_tb_classes(d))
        for k, v in _paths16(_blocks(d)).items():
            paths[k] = paths.get(k, 0) + v
    a, kw = _tb_args(name)
    _run_stream(*a, post=post, **kw)
    assert _tb_present(name, counts, paths), "%s: the generated pictures do not hold the blocks the case is about: %r %r" % (name, counts, paths)


# ---- what the statistics count --------------------------------------------------------------------------------------
def test_itrans_launches_counted_per_picture(built):
    """with statistics on, k_itrans counts at most two launches per picture (the 16 and the 32 class together, the 64 class) and exactly two for a picture with
    blocks of all three classes - picture by picture, each checked against the oracle"""
    import vvdec_amd
    import refdrv
    W, H, seed = 256, 128, 6500
    tools = TOOLS_I | abi.TOOL_BDOF | abi.TOOL_DMVR
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=True)
    rec = vvdec_amd.Reconstructor(W, H, num_slots=nslots, num_streams=1, log2_ctu=7, bit_depth=10)
    rec.enable_stats()
    seed_pic = synth.natural_picture(W, H, seed)
    rec.write_picture(0, seed_pic)
    cpu = {0: seed_pic}
    before, seen_three_classes, seen_without_16 = {}, 0, 0
    for pl in plans:
        d = synth.picture_for_plan(pl, W, H, seed=seed, tool_flags=tools, alloc=rec.host_array, log2_ctu=7, bit_depth=10, p_intra=0.0, p_bi=0.7, mv_sigma=6.0, p_split_scale=0.7,
                                   p_coded=0.9, p_coded_chroma=0.7, p_small_corner=0.3)
        classes = _tb_classes(d)
        rec.wait(rec.decompress_picture(d))
        got, want = rec.read_picture(pl.slot), refdrv.oracle_reconstruct(d, cpu)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "POC %d comp %d differs" % (pl.poc, c)
        cpu[pl.slot] = want
        now = {e["name"]: e["launches"] for e in rec.stats()}
        n = {k: v - before.get(k, 0) for k, v in now.items()}
        before = now
        assert n.get("k_itrans", 0) == (1 if classes[0] or classes[1] else 0) + (1 if classes[2] else 0), (pl.poc, classes, n)
        seen_three_classes += 1 if all(classes) else 0
        seen_without_16 += 1 if not classes[0] and classes[1] and classes[2] else 0
    rec.close()
    assert seen_three_classes and seen_without_16, (seen_three_classes, seen_without_16)
