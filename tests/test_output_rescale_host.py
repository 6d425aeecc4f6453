"""CPU: vvr_read_output_scaled, the host half (argument checks, scale factors and positions, packing, the caller's stride) on the stand-in runtime of
tests/hoststub, whose launch_rescale is a plain loop restating sampleRateConvCore (vvr_output.inc, compiled for the host only).  Ground truth is the
reference's own vvdec::rescalePlane from the drop-in library, on both of its paths (plain C++ and x86 SIMD, tests/rescale_ref.py)."""

import numpy as np
import pytest

import output_support as SUP
import rescale_ref
import test_host_glue as T
from vvdec_amd import abi

pytestmark = T.pytestmark


def _scaled(L, ctx, slot, comp, win, ow, oh, col, bps, pad=0):
    x, y, w, h = win
    a = np.full((oh, ow + pad), 0xaa if bps == 1 else 0xaaaa, np.uint8 if bps == 1 else np.uint16)
    rc = L.vvr_read_output_scaled(ctx, slot, comp, x, y, w, h, ow, oh, col, bps, a.ctypes.data, a.strides[0])
    assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
    assert pad == 0 or (a[:, ow:] == (0xaa if bps == 1 else 0xaaaa)).all(), "wrote beyond the row"
    return a[:, :ow]


def test_argument_checks():
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, 256, 128, 10, 1)
    buf = np.zeros(8192 * 16, np.uint16)

    def call(comp=0, x=0, y=0, w=64, h=32, ow=128, oh=64, col=1, bps=2, stride=None):
        return L.vvr_read_output_scaled(ctx, 0, comp, x, y, w, h, ow, oh, col, bps, buf.ctypes.data, stride if stride is not None else ow * bps)
    assert call() == abi.VVR_OK
    bad = [dict(x=200), dict(x=-1), dict(y=100), dict(comp=1, w=129), dict(comp=3),       # window outside the plane / no such plane
           dict(w=0), dict(h=0), dict(ow=0), dict(oh=0),                                 # zero sizes
           dict(ow=7), dict(oh=3), dict(ow=8 * 64 + 1), dict(oh=8 * 32 + 1), dict(w=2, ow=8193),      # ratio out of 1/8 .. 8, side beyond 8192
           dict(bps=1), dict(bps=3), dict(stride=127)]                                    # 8-bit output of a 10-bit context, sample size, stride
    for kw in bad:
        assert call(**kw) == abi.VVR_ERR_PARAMETER, kw
        if kw.get("comp") != 3:
            assert L.vvr_last_error(ctx), kw
    assert call(ow=8 * 64, oh=4) == abi.VVR_OK          # 8x up, 8x down: the ends of the range
    L.vvr_destroy(ctx)


@pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs /root/reference at build time)")
@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_values_are_rescale_plane(tmp_path, bd, cf):
    """every window of the case matrix against vvdec::rescalePlane, plain C++ and SIMD path; 8-bit content: rescalePlane of the samples widened
    to 16 bits, narrowed (what vvdecapp --upscale would do if it handed the frame's 8-bit samples over right)"""
    L = SUP.stub_lib()
    W = H = 1024
    ctx = SUP.make_ctx(L, W, H, bd, cf)
    rng = np.random.default_rng(bd * 10 + cf)
    planes = []
    for c in range(3 if cf else 1):
        s = 1 if c else 0
        p = rng.integers(0, 1 << bd, (H >> s, W >> s)).astype(np.uint16)
        assert L.vvr_write_plane(ctx, 1, c, p.ctypes.data, p.shape[1]) == abi.VVR_OK
        planes.append(p)
    cases, got = [], []
    for (comp, x, y, w, h, ow, oh, col) in rescale_ref.matrix(cf):
        cases.append((planes[comp][y:y + h, x:x + w], ow, oh, comp, cf, bd, col & 1, col >> 1))
        got.append(_scaled(L, ctx, 1, comp, (x, y, w, h), ow, oh, col, 2, pad=3))
        if bd == 8:
            assert np.array_equal(_scaled(L, ctx, 1, comp, (x, y, w, h), ow, oh, col, 1, pad=5), got[-1].astype(np.uint8))
    for simd in (False, True):
        want = rescale_ref.rescale(cases, T.build_stub(), simd, str(tmp_path))
        for n, (case, g, w_) in enumerate(zip(rescale_ref.matrix(cf), got, want)):
            assert g.shape == w_.shape and np.array_equal(g, w_), "case %d %r (simd %d): %d samples differ" % (n, case, simd, int((g != w_).sum()))
    L.vvr_destroy(ctx)
