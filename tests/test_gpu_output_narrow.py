"""GPU: 8-bit Y'CbCr frames from 9- and 10-bit pictures on the device (vvr_set_output_narrowing: k_output_narrow and the NARROW variants of
k_output_yuv, alone and behind k_film_grain / k_rescale).  The case matrix of tests/test_output_narrow_host.py with host destinations and with
torch tensors as destinations (Reconstructor.output_submit(into=...)); the new kernel and every new instantiation straight from the slot - on
windows stored whole, pair by pair, and on one of 18 x 6 samples whose pieces span three rows - with the checks that do not go through
tests/narrow_ref.py and the state of the context; a 3840x2160 frame and a window of it as nv12 under DITHER; a GOP whose frames are consumed on
the GPU as nv12 behind vvr_output_stream_wait without the host waiting for any of them; and the statistics entries.

The cases themselves are in tests/narrow_on_the_device.py, which runs in a process of its own, once for all of them (torch brings its own HIP
runtime, which has to be the first one the process initialises); the tests here read what it printed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
DEPTHS = [10, 9]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "narrow_on_the_device.py")] + ["matrix-%d" % bd for bd in DEPTHS] + ["straight-%d" % bd for bd in DEPTHS] + ["4k", "gop", "stats"], capture_output=True, text=True, timeout=600)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


@pytest.mark.parametrize("bd", DEPTHS)
def test_matrix_on_the_device(on_the_device, bd):
    _passed(on_the_device, "matrix-%d" % bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_the_new_kernels_straight_from_the_slot(on_the_device, bd):
    """k_output_narrow and the 20 new instantiations of k_output_yuv with values compared in every mode and phase; the cells of a dithered
    constant add up, multiples of 4 leave as their quarter, TRUNCATE is a shift, out-of-range words leave as 255; the mode as context state"""
    _passed(on_the_device, "straight-%d" % bd)


def test_a_4k_frame_and_a_window_of_it(on_the_device):
    """3840x2160, 10 bits, as nv12 under DITHER into contiguous tensors: the frame, and a window at an offset whose chroma rows are of odd length"""
    _passed(on_the_device, "4k")


def test_frames_consumed_on_the_gpu_without_the_host_waiting(on_the_device):
    """a GOP and the first pictures of the next one, every picture's nv12 output requested into its own tensors the moment the picture is
    submitted; a side stream waits for each request on the device and clones the tensors; the host waits for nothing until that stream is synchronised"""
    _passed(on_the_device, "gop")


def test_statistics_name_the_kernels(on_the_device):
    """vvr_get_stats: k_output_narrow with one launch per planar8 / nv12 request and its algorithmic bytes; the narrowed 4:2:2 / 4:4:4 formats
    under k_output_yuv"""
    _passed(on_the_device, "stats")
