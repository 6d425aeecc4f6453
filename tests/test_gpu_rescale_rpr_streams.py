"""GPU, end to end: the three RPR streams of tests/bitstreams decoded through the drop-in library (ctypes vvdec_* API in a child process, the frames
carry their sizes and seqInfo), every frame vvdecapp --upscale 2 would rescale (vvdecapp.cpp:1127-1163: progressive, cropped width AND height
below the SPS maximum; output at that maximum, chroma width / chromaSubX; chroma position from the VUI as upscaleFrame derives it) rescaled by the
back-end's vvr_read_output_scaled and compared with vvdec::rescalePlane (SIMD path) on the same frame.  For the 10-bit streams the concatenated
frames must also be the bytes oracle/_ref/vvdecapp_ref --upscale 2 -o writes, which pins the restated rule to the application.  (8-bit: vvdecapp
hands rescalePlane frames of one byte per sample that it reads as 16-bit samples - DESIGN.md section 3 - so only the rescalePlane comparison on
widened samples applies.)"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rescale_ref

HERE = os.path.dirname(os.path.abspath(__file__))
APP_REF = os.path.join(HERE, "..", "oracle", "_ref", "vvdecapp_ref")
STREAMS = ["mini_rpr_half_ctu64_384x256", "mini_rpr_four_sizes_ctu64_384x256", "mini_rpr_8bit_ctu128_256x256"]

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rescale_ref.available(), reason="oracle/_ref/libvvdec.so not built (needs /root/reference at build time)")]


def _rescaled(fr):
    return fr["progressive"] and fr["max_width"] > 0 and fr["width"] < fr["max_width"] and fr["height"] < fr["max_height"]


@pytest.mark.parametrize("name", STREAMS)
def test_rpr_stream_upscaled_like_vvdecapp(built, tmp_path, name):
    import vvdec_amd
    bit = os.path.join(HERE, "bitstreams", name, name + ".bit")
    frames = rescale_ref.decode(vvdec_amd._LIBPATH, bit, str(tmp_path))
    assert frames and all(f["color_format"] == 1 for f in frames)
    MW, MH, bd = frames[0]["max_width"], frames[0]["max_height"], frames[0]["bit_depth"]
    assert sum(_rescaled(f) for f in frames) >= 2, "the stream has no picture vvdecapp would rescale"
    rec = vvdec_amd.Reconstructor(MW, MH, bit_depth=bd, num_slots=2, num_streams=1)
    out, cases, got = [], [], []
    for f in frames:
        if not _rescaled(f):
            out.append(f["planes"])
            continue
        w, h = f["width"], f["height"]
        slot = []
        for c, pl in enumerate(f["planes"]):
            a = np.zeros(rec.plane_shape(c), np.uint16)
            a[:pl.shape[0], :pl.shape[1]] = pl
            slot.append(a)
        rec.write_picture(0, slot)
        g = rec.read_output(0, window=(0, 0, w, h), size=(MW, MH), collocated=f["collocated"])
        if bd == 8:
            g8 = rec.read_output(0, window=(0, 0, w, h), size=(MW, MH), collocated=f["collocated"], bytes_per_sample=1)
            assert all(np.array_equal(a.astype(np.uint8), b) for a, b in zip(g, g8))
        got.append(g)
        out.append(g)
        cases += [(f["planes"][c], MW >> (1 if c else 0), MH >> (1 if c else 0), c, 1, bd, f["collocated"][0], f["collocated"][1]) for c in range(3)]
    rec.close()
    want = rescale_ref.rescale(cases, vvdec_amd._LIBPATH, True, str(tmp_path))
    for n, g in enumerate(got):
        for c in range(3):
            assert np.array_equal(g[c], want[3 * n + c]), "rescaled frame %d component %d: %d samples differ" % (n, c, int((g[c] != want[3 * n + c]).sum()))
    if bd > 8:
        yuv = os.path.join(str(tmp_path), name + ".yuv")
        r = subprocess.run([APP_REF, "-b", bit, "--upscale", "2", "-o", yuv, "-v", "0"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
        ours = hashlib.md5(b"".join(np.ascontiguousarray(p, dtype="<u2").tobytes() for planes in out for p in planes)).hexdigest()
        assert ours == hashlib.md5(open(yuv, "rb").read()).hexdigest()
