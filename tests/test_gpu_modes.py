"""GPU parity over the mode tables (run with -m gpu): the pictures of tests/mode_cases.py - every luma intra mode and reference line on every CU shape in I
pictures (k_intra) and in intra CUs of B pictures (k_intra_leaf), every chroma mode and the three CCLM modes on every chroma shape, every MIP mode with and
without transposition, both ISP directions on every shape, both LFNST indices with every mode on every block class, explicit MTS, every SBT variant and
DCT-2 up to the last kept position, every GPM split on every shape that allows it, every pair of interpolation phases of plain motion
compensation - through the C ABI, bit-exact against the CPU oracle in every plane, and in the DMVR delta MVs where a picture has any.
tests/test_oracle_vs_ref_modes.py pins the same pictures against the reference classes on the CPU and shows, with one oracle run per instance, that every entry
of the legal sets is held by a CU whose samples depend on it; so a mismatch here is a kernel's.  Here every case asserts once more, from the description's
records alone (never from what the GPU returned), that each entry of its legal set is held by a CU with both neighbours inside the picture."""
import numpy as np
import pytest

import refdrv
import mode_cases as mc
from test_gpu_limits import _through_the_back_end

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", mc.CASES, ids=[c.id for c in mc.CASES])
def test_modes_bit_exact(built, case):
    pics = case.pictures()
    mc.held(case, pics)
    for n, (d, refs, l2) in enumerate(pics):
        want = refdrv.oracle_reconstruct(d, refs)
        nd = getattr(d, "num_dmvr", 0)
        want_dmvr = refdrv.oracle_dmvr(nd).copy() if nd else None
        got, dmvr = _through_the_back_end(d, refs, l2)
        for c in range(len(want)):
            g = got[c][:want[c].shape[0], :want[c].shape[1]]
            assert np.array_equal(g, want[c]), "%s picture %d (seed %d) comp %d: %d samples differ, the first at (x, y) = %r" % (
                case.id, n, case.specs[n][3], c, int((g != want[c]).sum()), tuple(int(v) for v in np.argwhere(g != want[c])[0][::-1]))
        if nd:
            assert np.array_equal(dmvr, want_dmvr), "%s picture %d: DMVR delta MVs differ" % (case.id, n)
