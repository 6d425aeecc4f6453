"""GPU: antialiased resampling at the output on the device (vvr_set_output_resampling: k_output_resample).  The cases of
tests/test_output_resample_host.py - each filter x each geometry x each content at 8 and 10 bits and in 4:0:0, which between them hold
non-integer ratios, an axis at ratio 1, odd chroma sizes, the 8x limit over two tiles, a last tile of 18 columns, more taps than lanes and the
64x limit with 256 taps on both axes - the filter as context state, eight requests of different filters and formats in flight, requests
directly behind vvr_submit across the pictures of a small stream (ordered on the device: nothing here depends on timing), and, in a process
of its own (tests/resample_on_the_device.py, whose output the tests here read), the formats behind the resampler with torch tensors as device
destinations, a window into a (3, 20, 48) float32 tensor and the statistics entries.  Expected samples are tests/resample_ref.py's; every
comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import output_support as SUP
import resample_ref as R
import rgb_ref
import test_gpu_output_compare as GC
import test_output_resample_host as N
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bd", [10, 8])
def test_every_filter_geometry_and_content_on_the_device(built, bd):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, N.W, N.H_, bd, 1)
    N.check_geometries(L, ctx, SUP.writer(L), bd, 3)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_400_contexts_on_the_device(built, bd):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, N.W400, N.H400, bd, 0)
    N.check_geometries(L, ctx, SUP.writer(L), bd, 1)
    L.vvr_destroy(ctx)


def test_the_filter_is_context_state_on_the_device(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, N.W, N.H_, 10, 1)
    N.check_state(L, ctx, SUP.writer(L), 10)
    L.vvr_destroy(ctx)


def test_eight_requests_in_flight_collected_out_of_order(built):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, N.W, N.H_, 10, 1)
    N.check_in_flight(L, ctx, SUP.writer(L))
    L.vvr_destroy(ctx)


def test_resampled_frames_of_the_pictures_of_a_stream_in_flight(built):
    """the fixed-seed stream of five pictures, 256x128, of test_xpsnr_of_the_pictures_of_a_stream_in_flight.  Directly behind every vvr_submit,
    with `job` set and no wait in between: the picture as a cubic 64 x 32 RGB8 frame.  Expected: the restatement and rgb_ref on the CPU
    oracle's planes"""
    import refdrv
    import vvdec_amd
    Wd, Hd = 256, 128
    win, size = (0, 0, Wd, Hd), (64, 32)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **GC.GEO)
    rec.set_output_colour(1, False)
    rec.set_output_resampling("cubic")
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4714, tool_flags=GC.TOOLS, alloc=rec.host_array, **GC.GEO, **GC.MIX) for pl in plans]
    cpu, want = {}, []
    for pl, d in zip(plans, descs):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        want.append(rgb_ref.rgb(R.resample(cpu[pl.slot], R.CUBIC, size, 10), 10, "rgb8", 1, False, (True, False)))
    tickets = []
    for pl, d in zip(plans, descs):
        job = rec.decompress_picture(d)
        tickets.append(rec.output_submit(pl.slot, job=job, window=win, fmt="rgb8", size=size))
    got = [rec.output_wait(t) for t in tickets]
    rec.sync()
    for k, (g, w_) in enumerate(zip(got, want)):
        N.same(g, w_, "request %d of the stream" % k)
    rec.close()


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "resample_on_the_device.py"), "tensor", "formats-10", "formats-8", "stats"], capture_output=True, text=True, timeout=300)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


def test_a_window_into_a_float32_tensor(on_the_device):
    """(2, 2, 204, 76) of a 10-bit frame -> (3, 20, 48) float32 on the device, normalised, under every filter"""
    _passed(on_the_device, "tensor")


@pytest.mark.parametrize("bd", [10, 8])
def test_formats_behind_the_resampler_on_the_device(on_the_device, bd):
    """planar, P010, NV12 under the dither narrowing, RGB8, RGBF32 with a normalisation, YUV444P16, V210; grain, then resample; destinations in
    memory of vvr_host_alloc at a padded stride and in torch tensors inside a guard region"""
    _passed(on_the_device, "formats-%d" % bd)


def test_statistics_name_the_kernel(on_the_device):
    """vvr_get_stats: k_output_resample, one launch per component, and no k_rescale for a request under a filter"""
    _passed(on_the_device, "stats")
