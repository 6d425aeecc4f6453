"""CPU: the plain-C oracle against the real reference classes at the ends of the picture partitioning (tests/partition_cases.py): tiles of one CTU and a last
column 8 samples wide, 20 tile columns, raster-scan slices that start in the middle of a tile row, rectangular slices inside tiles beside a slice of several
tiles, 256 slices, virtual boundaries at their extreme positions, sub-pictures of one CTU.  Every input of tests/test_gpu_partitions.py is pinned here first, so
a GPU failure there says that a kernel or the host glue is wrong, not the oracle.  Skipped where oracle/_ref is not built, like tests/test_oracle_vs_ref.py -
except the tests of the generator's refusals, which need nothing but the generator."""
import numpy as np
import pytest

import refdrv
import limits_cases as lc
import partition_cases as pc
from vvdec_amd import abi, synth, stream
from test_oracle_vs_ref import STAGES

needs_ref = pytest.mark.skipif(not refdrv.available(), reason="oracle/_ref not built")


def _pinned(d, refs, st=None):
    """oracle == reference in every stage, scalar and SIMD, with the description's edge tables and with the reference's own derivation"""
    st = st or lc.Stages(d, refs)
    nd = getattr(d, "num_dmvr", 0)
    for fl in STAGES:
        r = refdrv.reconstruct(d, refs, flags=fl, want_dmvr=nd)
        got = st(fl)
        for c in range(3):
            assert np.array_equal(got[c], r["planes"][c]), "flags %d comp %d: %d differ" % (fl, c, int((got[c] != r["planes"][c]).sum()))
        if nd and fl == 0:
            assert np.array_equal(st.dmvr, r["dmvr"][:nd]), "DMVR delta MVs differ"
    for fl in (refdrv.STOP_AFTER_DBK, 0):
        b = refdrv.reconstruct(d, refs, flags=fl | refdrv.DERIVE_LFP)["planes"]
        assert all(np.array_equal(x, y) for x, y in zip(st(fl), b)), "flags %d: the reference derives other edge parameters" % fl
    simd = refdrv.reconstruct(d, refs, flags=refdrv.SIMD)["planes"]
    assert all(np.array_equal(x, y) for x, y in zip(st(0), simd)), "the reference's SIMD path differs from its scalar path"
    return st


@needs_ref
@pytest.mark.parametrize("case", pc.PARTITION_CASES, ids=[c.id for c in pc.PARTITION_CASES])
def test_oracle_equals_reference_on_the_partitions(built, case):
    d, refs = case.make()
    st = _pinned(d, refs)
    case.present(case, d, refs, st)
    print("%s: %r" % (case.id, case.found))


@needs_ref
@pytest.mark.parametrize("name,W,H,l2,seed,tools,kw,vary", pc.STREAMS, ids=[s[0] for s in pc.STREAMS])
def test_oracle_equals_reference_on_the_partition_streams(built, name, W, H, l2, seed, tools, kw, vary):
    """the streams tests/test_gpu_partitions.py sends through the asynchronous path: the same descriptions, the oracle consuming its own pictures as references"""
    plans, _ = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    dpb = {}
    for pl in plans:
        d = synth.picture_for_plan(pl, W, H, seed=seed, tool_flags=tools, log2_ctu=l2, **dict(pc.STREAM_MIX, **kw))
        if vary:
            synth.vary_slices(d, seed + pl.poc)
        st = _pinned(d, dpb)
        dpb[pl.slot] = st(0)


@pytest.mark.parametrize("name,kw", pc.ILLEGAL, ids=[x[0] for x in pc.ILLEGAL])
def test_the_generator_refuses_what_no_stream_can_carry(name, kw):
    """tile grids that do not add up, slice maps no PPS expresses (raster: runs of complete tiles in tile order; rectangular: rectangles of complete tiles or complete
    CTU rows of one tile; numbered in the PPS's order), virtual boundaries off the 8-sample grid, outside the picture, not ascending or closer than one CTU"""
    p = synth.default_params(width=192, height=192, log2_ctu=5, slice_type=abi.SLICE_I, seed=1, **kw)
    what = "virtual boundaries" if name.startswith(("boundar", "four_boundar")) else "partitioning"
    with pytest.raises(RuntimeError, match=what):
        synth.generate(p)


@pytest.mark.parametrize("name,kw", pc.LEGAL, ids=[x[0] for x in pc.LEGAL])
def test_the_generator_accepts_the_neighbours_of_what_it_refuses(name, kw):
    d = synth.generate(synth.default_params(width=192, height=192, log2_ctu=5, slice_type=abi.SLICE_I, seed=1, **kw))
    if "slice_map" in kw:
        assert np.array_equal(d.ctu_slice, kw["slice_map"][1]) and np.array_equal(d.ctu_tile.reshape(6, 6), synth.tile_of_ctu((3, 3), (3, 3)))
    else:
        assert list(d.hdr.vb_pos_x) == [8, 40, 72] and list(d.hdr.vb_pos_y)[:2] == [152, 184] and (d.hdr.num_ver_vb, d.hdr.num_hor_vb) == (3, 2)


def test_every_layout_of_the_table_is_what_it_says():
    """needs nothing but the generator: the maps the cases are about, before any stage runs"""
    for case in pc.PARTITION_CASES:
        d, refs = case.make()
        l2, S, cx, cy = pc.geometry(d)
        if hasattr(case, "grid"):
            assert np.array_equal(d.ctu_tile.reshape(cy, cx), synth.tile_of_ctu(*case.grid)), case.id
        if hasattr(case, "vbs"):
            assert [int(v) for v in d.hdr.vb_pos_x[:d.hdr.num_ver_vb]] == list(case.vbs[0]) and [int(v) for v in d.hdr.vb_pos_y[:d.hdr.num_hor_vb]] == list(case.vbs[1]), case.id
        if case.family in ("raster_slices", "rect_slices"):
            assert d.ctu_slice is not None and len(np.unique(d.ctu_slice)) == int(d.ctu_slice.max()) + 1 > 1, case.id


@pytest.mark.parametrize("l2,W,H", [(5, 256, 192), (6, 512, 384)])
def test_ibc_block_vectors_stay_inside_the_slice_and_tile(l2, W, H):
    """the IBC virtual buffer starts empty at the first CTU of every CTU row of a tile and of a slice: a generated block vector never points into another slice or
    tile (vvr_prepare refuses such a CU: "the reference block is not reconstructed before the CU").  Raster-scan slices over 4 x 3 tiles of 2 x 2 CTUs"""
    tools = pc.TOOLS_P | abi.TOOL_IBC | pc.NO_SLICES
    p = synth.default_params(width=W, height=H, log2_ctu=l2, slice_type=abi.SLICE_I, seed=4700 + l2, tool_flags=tools, p_ibc=0.6, p_split_scale=1.4, **pc._RASTER)
    d = synth.generate(p)
    tile, slc = pc.ctu_maps(d)
    ibc = d.cu[d.cu["pred_mode"] == abi.PRED_IBC]
    near_an_edge = 0
    for cu in ibc:
        x, y, w, h = int(cu["x"]), int(cu["y"]), int(cu["w"]), int(cu["h"])
        rx, ry = x + (int(cu["mv"][0, 0, 0]) >> 4), y + (int(cu["mv"][0, 0, 1]) >> 4)
        own = (tile[y >> l2, x >> l2], slc[y >> l2, x >> l2])
        for (px, py) in ((rx, ry), (rx + w - 1, ry), (rx, ry + h - 1), (rx + w - 1, ry + h - 1)):
            assert (tile[py >> l2, px >> l2], slc[py >> l2, px >> l2]) == own, "IBC CU at (%d, %d) copies from another slice or tile" % (x, y)
        left = (x - 1) >> l2
        near_an_edge += x >= (1 << l2) and x % (1 << l2) < 16 and (tile[y >> l2, left], slc[y >> l2, left]) != own
    assert len(ibc) > 50 and near_an_edge > 0
