"""GPU: many regions of one picture as a batch in one request on the device (vvr_output_submit_batch: the region as blockIdx.z of k_rescale,
k_output_resample, k_output_resample_h and k_output_rgb).  The cases of tests/test_output_batch_host.py - no scaling through the table of
origins, the three antialiased filters in the one-launch and the two-launch form, more than one tile across, the reference's DCTIF, the
transform and the LUT, 256 regions, destinations in pageable memory and in memory of vvr_host_alloc, eight batches in flight, the refusals - a
batch behind every vvr_submit of a small stream (ordered on the device: nothing here depends on timing), and, in a process of its own
(tests/batch_on_the_device.py, whose output the tests here read), torch tensors as destinations, device ranges inside guard regions, a torch
stream ordered behind the ticket and the launch counts.  Expected bytes are the restatements' (tests/resample_ref.py, rgb_ref, interleaved_ref,
...), never the code's; every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import output_support as SUP
import resample_ref as R
import rgb_ref
import test_gpu_output_compare as GC
import test_output_batch_host as B
import test_output_semiplanar_host as S
from vvdec_amd import stream, synth

pytestmark = pytest.mark.gpu


def _run(check, bd, *args, **kw):
    L = SUP.product_lib()
    ctx = SUP.make_ctx(L, B.W, B.H_, bd, 1)
    check(L, ctx, SUP.writer(L), *args, **kw)
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("bd", [10, 8])
def test_no_scaling_on_the_device(built, bd):
    _run(B.check_straight, bd, bd)


@pytest.mark.parametrize("bd", [10, 8])
def test_antialiased_one_launch_per_plane_on_the_device(built, bd):
    _run(B.check_antialiased, bd, bd)


@pytest.mark.parametrize("bd", [10, 8])
def test_more_than_one_tile_across_and_the_two_launch_form_on_the_device(built, bd):
    _run(B.check_wide_and_two_launch, bd, bd)


@B.need_ref
@pytest.mark.parametrize("bd", [10, 8])
def test_dctif_is_rescale_plane_on_the_device(built, tmp_path, bd):
    import vvdec_amd
    _run(B.check_dctif, bd, bd, vvdec_amd._LIBPATH, str(tmp_path))


def test_transform_and_lut_on_the_device(built):
    _run(B.check_transform_and_lut, 10)


def test_count_at_the_limit_on_the_device(built):
    _run(B.check_limit, 10)


def test_a_batch_of_one_is_the_single_request_on_the_device(built):
    _run(B.check_a_batch_of_one_is_the_single_request, 10)


def test_pageable_and_pinned_destinations(built):
    """(the device ranges: tests/batch_on_the_device.py, below)"""
    _run(B.check_destinations, 10, homes=(B.Pageable, B.Pinned, None))


def test_eight_batches_in_flight_collected_out_of_order(built):
    _run(B.check_in_flight, 10)


def test_refusals_leave_the_ring_alone_on_the_device(built):
    L = SUP.product_lib()
    B.check_refusals(L, lambda: SUP.make_ctx(L, B.W, B.H_, 10, 1), SUP.writer(L))


def test_batches_of_the_pictures_of_a_stream_in_flight(built):
    """the fixed-seed stream of five pictures, 256x128, of test_resampled_frames_of_the_pictures_of_a_stream_in_flight.  Directly behind every
    vvr_submit, with `job` set and no wait in between: a batch of four 128 x 64 -> 32 x 16 cubic RGB8 regions.  Expected: the restatement and
    rgb_ref on the crops of the CPU oracle's planes"""
    import refdrv
    import vvdec_amd
    Wd, Hd = 256, 128
    origins, wsize, size = [(0, 0), (128, 0), (0, 64), (128, 64)], (128, 64), (32, 16)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=4, host_threads=3, **GC.GEO)
    rec.set_output_colour(1, False)
    rec.set_output_resampling("cubic")
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=4714, tool_flags=GC.TOOLS, alloc=rec.host_array, **GC.GEO, **GC.MIX) for pl in plans]
    cpu, want = {}, []
    for pl, d in zip(plans, descs):
        cpu[pl.slot] = refdrv.oracle_reconstruct(d, cpu)
        want.append(np.stack([np.stack(rgb_ref.rgb(R.resample(S.crop(cpu[pl.slot], o + wsize), R.CUBIC, size, 10), 10, "rgb8", 1, False, (True, False))) for o in origins]))
    tickets = []
    for pl, d in zip(plans, descs):
        job = rec.decompress_picture(d)
        tickets.append(rec.output_submit_batch(pl.slot, origins, wsize, "rgb8", job=job, size=size))
    got = [rec.output_wait(t) for t in tickets]
    rec.sync()
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g.shape == (4, 3, 16, 32) and g.dtype == np.uint8
        B.N.same([g], [w_], "the batch behind picture %d of the stream" % k)
    rec.close()


CASES = ["tensors", "destinations", "stream-wait", "stats"]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "batch_on_the_device.py")] + CASES, capture_output=True, text=True, timeout=300)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


def test_tensors_as_destinations(on_the_device):
    """a (4, 3, 12, 28) float32 tensor and a (4, 12, 28, 4) uint8 tensor as into=, compared on the host"""
    _passed(on_the_device, "tensors")


def test_device_ranges_inside_guard_regions(on_the_device):
    """the direct store into a contiguous (N, 3, H, W) layout; batch_stride_bytes = extent + 6 through the entry's scratch; a base that is not
    aligned to 32 bytes - each inside a guard region that comes back untouched"""
    _passed(on_the_device, "destinations")


def test_a_torch_stream_ordered_behind_the_ticket(on_the_device):
    _passed(on_the_device, "stream-wait")


def test_launch_counts_do_not_depend_on_the_number_of_regions(on_the_device):
    """vvr_get_stats: a batch of 4 under the triangle filter is 3 launches of k_output_resample and 1 of k_output_rgb; the two-launch geometry
    counts what its single request counts"""
    _passed(on_the_device, "stats")
