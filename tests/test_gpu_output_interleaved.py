"""GPU: the interleaved RGB formats of the output queue (rgba8, bgra8, rgb24, bgr24, rgb10a2, rgba16f) and rgbf32 with its normalisation on the
device (the new stores of k_output_rgb, alone and behind k_film_grain / k_rescale).  The case matrix of tests/test_output_interleaved_host.py with
host destinations and with torch tensors as destinations (Reconstructor.output_submit(into=...): (h, w, C), (h, w) int32, (3, h, w) float32),
every instantiation of the store straight from the slot, the new formats against the planar requests of the same frame with the normalisation's
state, a GOP whose frames are consumed on the GPU as bgra8 and normalised rgbf32 behind vvr_output_stream_wait without the host waiting for any
of them, and the statistics entry.

The cases themselves are in tests/interleaved_on_the_device.py, which runs in a process of its own, once for all of them (torch brings its own
HIP runtime, which has to be the first one the process initialises); the tests here read what it printed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
DEPTHS = [10, 8, 9]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    cases = ["straight-%d" % bd for bd in DEPTHS] + ["matrix-%d" % bd for bd in DEPTHS] + ["cross-%d" % bd for bd in DEPTHS] + ["gop", "stats"]
    r = subprocess.run([sys.executable, os.path.join(here, "interleaved_on_the_device.py")] + cases, capture_output=True, text=True, timeout=600)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


@pytest.mark.parametrize("bd", DEPTHS)
def test_every_instantiation_straight_from_the_slot(on_the_device, bd):
    """classes x chroma positions x whole and pair-by-pair stores x with and without a transform, on 448x160, 200x64, 202x38, 196x38 and 198x38:
    all 80 new instantiations of k_output_rgb with values compared, into pageable memory and into aligned tensors (the kernel's own store)"""
    _passed(on_the_device, "straight-%d" % bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_matrix_on_the_device(on_the_device, bd):
    """every format plain, grained, rescaled, grained then rescaled; tensors at an aligned base, off it, and with padded rows, inside a guard region"""
    _passed(on_the_device, "matrix-%d" % bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_against_the_planar_formats_and_the_normalisation_state(on_the_device, bd):
    _passed(on_the_device, "cross-%d" % bd)


def test_frames_consumed_on_the_gpu_without_the_host_waiting(on_the_device):
    """a GOP, every picture's bgra8 and normalised rgbf32 output requested the moment the picture is submitted; a side stream waits for each
    request on the device and clones the tensor; the host waits for nothing until that stream is synchronised"""
    _passed(on_the_device, "gop")


def test_statistics_name_the_kernel(on_the_device):
    """vvr_get_stats: k_output_rgb with one launch per request of a new format"""
    _passed(on_the_device, "stats")
