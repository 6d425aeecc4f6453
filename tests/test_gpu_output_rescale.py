"""GPU: vvr_read_output_scaled on the device (k_rescale) against the reference's own vvdec::rescalePlane (drop-in library, tests/rescale_ref.py): the
case matrix of the CPU test on planes written to a slot, windows of a picture smaller than its slot (vvr_slot_picture_size), the headline sizes
(1080p -> 4K, 4K -> 8K) and a reconstructed picture through Reconstructor.read_output(size=...)."""
import ctypes as C

import numpy as np
import pytest

import rescale_ref
from vvdec_amd import abi, synth, stream

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs /root/reference at build time)")]


def _backend():
    import vvdec_amd
    return vvdec_amd._LIBPATH


def _scaled(rec, slot, comp, win, ow, oh, col, bps, pad=0):
    x, y, w, h = win
    fill = 0xaa if bps == 1 else 0xaaaa
    a = np.full((oh, ow + pad), fill, np.uint8 if bps == 1 else np.uint16)
    rec._check(rec.L.vvr_read_output_scaled(rec.ctx, slot, comp, x, y, w, h, ow, oh, col, bps, a.ctypes.data, a.strides[0]))
    assert pad == 0 or (a[:, ow:] == fill).all(), "wrote beyond the row"
    return a[:, :ow]


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_matrix_on_the_device(built, tmp_path, bd, cf):
    import vvdec_amd
    W = H = 1024
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=bd, chroma_format=cf, num_slots=3, num_streams=1)
    rng = np.random.default_rng(bd * 10 + cf)
    ncomp = 3 if cf else 1
    planes = [rng.integers(0, 1 << bd, rec.plane_shape(c)).astype(np.uint16) for c in range(ncomp)]
    rec.write_picture(1, planes)
    # a picture smaller than its slot (an RPR picture): its planes at its own size
    PW, PH = 344, 200
    small = [rng.integers(0, 1 << bd, (PH >> (1 if c else 0), PW >> (1 if c else 0))).astype(np.uint16) for c in range(ncomp)]
    rec._check(rec.L.vvr_slot_picture_size(rec.ctx, 2, PW, PH))
    for c in range(ncomp):
        rec._check(rec.L.vvr_write_plane(rec.ctx, 2, c, small[c].ctypes.data, small[c].shape[1]))
    cases, got, names = [], [], []
    for (comp, x, y, w, h, ow, oh, col) in rescale_ref.matrix(cf):
        cases.append((planes[comp][y:y + h, x:x + w], ow, oh, comp, cf, bd, col & 1, col >> 1))
        got.append(_scaled(rec, 1, comp, (x, y, w, h), ow, oh, col, 2, pad=3))
        names.append(("slot", comp, x, y, w, h, ow, oh, col))
        if bd == 8:
            assert np.array_equal(_scaled(rec, 1, comp, (x, y, w, h), ow, oh, col, 1, pad=5), got[-1].astype(np.uint8))
    # 8x down over several tile rows: the tile height the launcher picks (16) fills the 128 rows of sums exactly
    for comp in range(ncomp):
        s = 1 if comp else 0
        cases.append((planes[comp][:H >> s, :W >> s], 128 >> s, 128 >> s, comp, cf, bd, 1, 0))
        got.append(_scaled(rec, 1, comp, (0, 0, W >> s, H >> s), 128 >> s, 128 >> s, 1, 2))
        names.append(("8x down", comp))
    for comp in range(ncomp):
        s = 1 if comp else 0
        for (x, y, w, h, ow, oh, col) in ((0, 0, PW >> s, PH >> s, 1024 >> s, 600 >> s, 1), (3 >> s, 5 >> s, 301 >> s, 187 >> s, 77, 61, 2)):
            cases.append((small[comp][y:y + h, x:x + w], ow, oh, comp, cf, bd, col & 1, col >> 1))
            got.append(_scaled(rec, 2, comp, (x, y, w, h), ow, oh, col, 2))
            names.append(("small picture", comp, x, y, w, h, ow, oh, col))
        with pytest.raises(vvdec_amd.VvrError):
            _scaled(rec, 2, comp, (0, 0, (PW >> s) + 1, PH >> s), 64, 64, 1, 2)      # beyond the picture, inside the slot
    for simd in (False, True):
        want = rescale_ref.rescale(cases, _backend(), simd, str(tmp_path))
        for name, g, w_ in zip(names, got, want):
            assert g.shape == w_.shape and np.array_equal(g, w_), "%r (simd %d): %d samples differ" % (name, simd, int((g != w_).sum()))
    rec.close()


@pytest.mark.parametrize("src,dst", [((1920, 1080), (3840, 2160)), ((3840, 2160), (7680, 4320))])
def test_headline_sizes(built, tmp_path, src, dst):
    """a 10-bit 4:2:0 frame to twice its size, all three planes through Reconstructor.read_output(size=...), against rescalePlane (SIMD path:
    what vvdecapp --upscale 2 runs)"""
    import vvdec_amd
    W, H = src
    rec = vvdec_amd.Reconstructor(W, H, num_slots=2, num_streams=1)
    planes = synth.natural_picture(W, H, 31)
    rec.write_picture(0, planes)
    got = rec.read_output(0, size=dst)
    cases = [(planes[c], dst[0] >> (1 if c else 0), dst[1] >> (1 if c else 0), c, 1, 10, True, False) for c in range(3)]
    want = rescale_ref.rescale(cases, _backend(), True, str(tmp_path))
    for c in range(3):
        assert np.array_equal(got[c], want[c]), "component %d: %d samples differ" % (c, int((got[c] != want[c]).sum()))
    rec.close()


@pytest.mark.parametrize("bd", [10, 8])
def test_reconstructed_picture(built, tmp_path, bd):
    """a picture reconstructed on the device, cropped and rescaled at the boundary (up and down, chroma sited both ways), as 16- and 8-bit samples"""
    import vvdec_amd
    W, H = 264, 136
    geo = dict(bit_depth=bd, chroma_format=1, log2_ctu=6)
    rec = vvdec_amd.Reconstructor(W, H, num_slots=3, num_streams=1, **geo)
    plans, _ = stream.ra_plan(1, gop=1, seed_poc0_is_external=False)
    tools = abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST
    d = synth.picture_for_plan(plans[0], W, H, seed=991, tool_flags=tools, **geo)
    rec.wait(rec.decompress_picture(d))
    full = rec.read_picture(plans[0].slot)
    win = (8, 4, 240, 120)
    x, y, w, h = win
    for size, col in (((480, 240), (True, False)), ((160, 90), (False, True)), ((530, 262), (False, False))):
        got = rec.read_output(plans[0].slot, window=win, size=size, collocated=col)
        cases = [(full[c][y >> s:(y + h) >> s, x >> s:(x + w) >> s], size[0] >> s, size[1] >> s, c, 1, bd, col[0], col[1]) for c, s in ((0, 0), (1, 1), (2, 1))]
        want = rescale_ref.rescale(cases, _backend(), True, str(tmp_path))
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "size %r component %d" % (size, c)
        if bd == 8:
            got8 = rec.read_output(plans[0].slot, window=win, size=size, collocated=col, bytes_per_sample=1)
            for c in range(3):
                assert got8[c].dtype == np.uint8 and np.array_equal(got8[c], want[c].astype(np.uint8))
    rec.close()
