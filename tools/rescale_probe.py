"""Rescaled output of one 10-bit 4:2:0 1920x1080 frame to 3840x2160 (vvr_read_output_scaled, all three planes): wall time of the three calls
(device rescale + PCIe copy of the 24.9 MB result + rows to the caller), the same frame through the host's vvdec::rescalePlane (SIMD path, drop-in
library) for comparison.  Kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/rescale_probe.py` (k_rescale rows).
Usage: python tools/rescale_probe.py [reps]   |   (child) python tools/rescale_probe.py --host <reps>"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SRC, DST = (1920, 1080), (3840, 2160)


def host(reps):
    import vvdec_amd
    import rescale_ref
    C.CDLL(vvdec_amd._LIBPATH, mode=C.RTLD_GLOBAL)
    L = C.CDLL(rescale_ref.DROPIN_LIB)
    f = getattr(L, rescale_ref.RESCALE)
    f.argtypes = [C.POINTER(rescale_ref.Plane), C.POINTER(rescale_ref.Plane), C.c_int, C.c_int, C.c_int, C.c_bool, C.c_bool]
    L.vvdec_params_alloc.restype = C.POINTER(rescale_ref.Params)
    L.vvdec_decoder_open.restype = C.c_void_p
    L.vvdec_decoder_open.argtypes = [C.POINTER(rescale_ref.Params)]
    p = L.vvdec_params_alloc()
    L.vvdec_params_default(p)
    p.contents.threads = 0
    assert L.vvdec_decoder_open(p)           # (the SIMD buffer operations from here on)
    from vvdec_amd import synth
    planes = synth.natural_picture(SRC[0], SRC[1], 31)
    outs = [np.zeros((DST[1] >> (1 if c else 0), DST[0] >> (1 if c else 0)), np.uint16) for c in range(3)]
    ts = []
    for r in range(reps):
        t0 = time.perf_counter()
        for c in range(3):
            s = np.ascontiguousarray(planes[c])
            sp = rescale_ref.Plane(s.ctypes.data, s.shape[1], s.shape[0], s.strides[0], 2, None)
            dp = rescale_ref.Plane(outs[c].ctypes.data, outs[c].shape[1], outs[c].shape[0], outs[c].strides[0], 2, None)
            f(C.byref(sp), C.byref(dp), c, 1, 10, True, False)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"host_rescalePlane_simd_ms_median": round(1e3 * float(np.median(ts)), 2), "reps": reps}))


def device(reps):
    import vvdec_amd
    from vvdec_amd import synth
    rec = vvdec_amd.Reconstructor(SRC[0], SRC[1], num_slots=2, num_streams=1)
    rec.write_picture(0, synth.natural_picture(SRC[0], SRC[1], 31))
    outs = [np.zeros((DST[1] >> (1 if c else 0), DST[0] >> (1 if c else 0)), np.uint16) for c in range(3)]
    ts = []
    for r in range(reps + 3):
        t0 = time.perf_counter()
        for c in range(3):
            s = 1 if c else 0
            rec._check(rec.L.vvr_read_output_scaled(rec.ctx, 0, c, 0, 0, SRC[0] >> s, SRC[1] >> s, DST[0] >> s, DST[1] >> s, 1, 2, outs[c].ctypes.data, outs[c].strides[0]))
        ts.append(time.perf_counter() - t0)
    rec.close()
    mb = sum(o.nbytes for o in outs) / 1e6
    print(json.dumps({"device_three_calls_ms_median": round(1e3 * float(np.median(ts[3:])), 2), "ms_min": round(1e3 * min(ts[3:]), 2), "result_MB": round(mb, 1), "reps": reps}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--host":
        host(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
        device(reps)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--host", "5"], timeout=600)
