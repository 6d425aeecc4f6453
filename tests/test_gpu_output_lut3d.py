"""GPU: the 3-D LUT stage of the RGB formats of the output queue on the device (k_output_rgb in its LUT mode; vvr_set_output_lut3d,
vvr_output_lut3d_preset).  The cases of tests/test_output_lut3d_host.py at 10 and 8 bits, each request into host memory and into a (3, h, w) /
(h, w, c) torch tensor; three pictures of a GOP as rgba8 under the PQ LUT preset, consumed on the GPU behind vvr_output_stream_wait without the
host waiting for any of them; and the statistics entry: one k_output_rgb launch per request.

The cases themselves are in tests/output_lut3d_on_the_device.py, which runs in a process of its own, once for all of them (torch brings its own HIP
runtime, which has to be the first one the process initialises); the tests here read what it printed."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
DEPTHS = [10, 8]
KINDS = ["random", "extremes", "grey", "snapshot"]


@pytest.fixture(scope="module")
def on_the_device(built):
    here = os.path.dirname(os.path.abspath(__file__))
    cases = ["%s-%d" % (kind, bd) for kind in KINDS for bd in DEPTHS] + ["gop", "stats"]
    r = subprocess.run([sys.executable, os.path.join(here, "output_lut3d_on_the_device.py")] + cases, capture_output=True, text=True, timeout=300)
    return r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]


def _passed(on_the_device, case):
    lines, tail = on_the_device
    assert "ok " + case in lines, "%s did not pass (the cases run in order and stop at the first failure):\n%s" % (case, tail)


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_host_cases_on_the_device(on_the_device, kind, bd):
    """random: seeded LUTs of 17, 33 and 65 points, every RGB format and chroma position, whole and pair-by-pair stores, with and without a
    transform ahead, behind a rescale (the stage reads `tmp` planes) and behind grain and a rescale; extremes: all nodes 65535, all 0, 0 / 65535 by
    parity at 17 points; grey: all three fractions tie in every pixel; snapshot: two LUTs of different sizes in flight, the formats and the
    synchronous calls that ignore them, NULL"""
    _passed(on_the_device, "%s-%d" % (kind, bd))


def test_a_gop_under_the_pq_lut_preset_consumed_on_the_gpu(on_the_device):
    _passed(on_the_device, "gop")


def test_statistics_count_one_launch_per_request(on_the_device):
    """vvr_get_stats: k_output_rgb with one launch per RGB request, with a LUT or without"""
    _passed(on_the_device, "stats")
