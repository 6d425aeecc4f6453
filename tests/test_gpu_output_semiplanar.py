"""GPU: the semi-planar formats of the output queue on the device (k_output_frame's CbCr piece, NV12 / P010 stores) and destinations in device
memory.  The case matrix of tests/test_output_semiplanar_host.py with the device destinations in torch tensors (Reconstructor.output_submit(into=...))
and in memory of vvr_device_alloc, a 3840x2160 frame through the direct and the laid-out store, and a GOP whose frames are consumed on the GPU
behind vvr_output_stream_wait without the host waiting for any of them.

The cases themselves are in tests/semiplanar_on_the_device.py, which runs in a process of its own, once for all of them (torch brings its own HIP
runtime, which has to be the first one the process initialises - as test_reference_slots_replicated_between_two_back_ends_on_the_device does); the
tests here read what it printed."""
import os
import subprocess
import sys

import pytest

import test_output_semiplanar_host as S

pytestmark = pytest.mark.gpu
MATRIX = ["matrix-%d-%s" % v for v in S.VARIANTS]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "semiplanar_on_the_device.py")] + MATRIX + ["4k", "gop"], capture_output=True, text=True, timeout=600)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


@pytest.mark.parametrize("bd,fmt", S.VARIANTS)
def test_matrix_on_the_device(on_the_device, bd, fmt):
    _passed(on_the_device, "matrix-%d-%s" % (bd, fmt))


def test_a_4k_frame_direct_and_laid_out(on_the_device):
    """3840x2160, 10 bits, the frame and a window at an offset as P010: into contiguous tensors (k_output_frame stores straight into them) and into
    views with padded rows (scratch, then one device-to-device copy per plane), against the picture that was written"""
    _passed(on_the_device, "4k")


def test_frames_consumed_on_the_gpu_without_the_host_waiting(on_the_device):
    """a GOP and the first pictures of the next one, every picture's P010 output requested into its own tensors the moment the picture is submitted;
    a side stream waits for each request on the device and clones the tensors; the host waits for nothing until that stream is synchronised"""
    _passed(on_the_device, "gop")
