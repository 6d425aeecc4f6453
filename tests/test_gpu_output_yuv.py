"""GPU: the Y'CbCr formats at 4:4:4 and 4:2:2 of the output queue on the device (k_output_yuv, alone and behind k_film_grain / k_rescale).  The case
matrix of tests/test_output_yuv_host.py with host destinations and with torch tensors as destinations (Reconstructor.output_submit(into=...)),
every instantiation of the kernel straight from the slot with the two cross-checks (the planes of yuv444p16 through the matrix are rgb16; phase 0
of yuv422p16 is the source row), a 3840x2160 frame and a window of it as v210 and as yuv444p16, a GOP whose frames are consumed on the GPU as
y210 behind vvr_output_stream_wait without the host waiting for any of them, and the statistics entry.

The cases themselves are in tests/yuv_on_the_device.py, which runs in a process of its own, once for all of them (torch brings its own HIP
runtime, which has to be the first one the process initialises); the tests here read what it printed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
DEPTHS = [10, 8, 9]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "yuv_on_the_device.py")] + ["matrix-%d" % bd for bd in DEPTHS] + ["straight-%d" % bd for bd in DEPTHS] + ["4k", "gop", "stats"], capture_output=True, text=True, timeout=600)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


@pytest.mark.parametrize("bd", DEPTHS)
def test_matrix_on_the_device(on_the_device, bd):
    _passed(on_the_device, "matrix-%d" % bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_every_instantiation_straight_from_the_slot(on_the_device, bd):
    """formats x chroma positions x whole and pair-by-pair stores: all 46 instantiations of k_output_yuv with values compared (26 of them at 9 and
    10 bits), and the two cross-checks that do not go through tests/yuv_ref.py"""
    _passed(on_the_device, "straight-%d" % bd)


def test_a_4k_frame_and_a_window_of_it(on_the_device):
    """3840x2160, 10 bits, as v210 and as yuv444p16 into contiguous tensors: the frame, and a window at an offset whose rows end in a group of
    four pixels and are no multiple of 8 samples"""
    _passed(on_the_device, "4k")


def test_frames_consumed_on_the_gpu_without_the_host_waiting(on_the_device):
    """a GOP and the first pictures of the next one, every picture's y210 output requested into its own tensor the moment the picture is
    submitted; a side stream waits for each request on the device and clones the tensor; the host waits for nothing until that stream is synchronised"""
    _passed(on_the_device, "gop")


def test_statistics_name_the_kernel(on_the_device):
    """vvr_get_stats: k_output_yuv with one launch per request of a new format and its algorithmic bytes; the checks of `into`"""
    _passed(on_the_device, "stats")
