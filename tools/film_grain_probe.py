"""Film grain on one 10-bit 4:2:0 3840x2160 frame: wall time of vvr_read_output_grain (blocks' words on the host, device grain + crop + packing,
PCIe copy of the 24.9 MB result, rows to the caller) against three vvr_read_output calls on the same window, and the reference's own
FilmGrain::add_grain_line over the frame on the host, one thread (oracle/_ref/libvvref.so, in a child process).  Kernel time: run under
`rocprofv3 --kernel-trace --stats -- python tools/film_grain_probe.py` (k_film_grain rows).
Usage: python tools/film_grain_probe.py [reps]   |   (child) python tools/film_grain_probe.py --host <reps>"""
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
W, H = 3840, 2160


def _sei():
    import film_grain_ref
    return film_grain_ref.random_sei(np.random.default_rng(1), 0, 8, 5)


def host(reps):
    import film_grain_ref as F
    from vvdec_amd import synth
    L = C.CDLL(F.REF_LIB)
    f = {k: getattr(L, v) for k, v in F.SYM.items()}
    for fn in f.values():
        fn.restype = None
    obj = (C.c_uint64 * 8192)()
    fg = C.addressof(obj)
    f["ctor"].argtypes = [C.c_void_p]
    f["ctor"](fg)
    s = F.sei_struct(_sei())
    f["update"].argtypes = [C.c_void_p, C.c_void_p]
    f["update"](fg, C.addressof(s))
    impl = C.c_uint64.from_address(fg).value
    f["depth"].argtypes = [C.c_void_p, C.c_int]
    f["depth"](impl, 10)
    f["color"].argtypes = [C.c_void_p, C.c_int]
    f["color"](fg, 1)
    f["seeds"].argtypes = [C.c_void_p, C.c_int, C.c_int]
    line = f["line"]
    line.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    planes = [np.ascontiguousarray(np.pad(p, ((0, 0), (0, 64)), mode="edge")) for p in synth.natural_picture(W, H, 7)]
    rows = [[planes[0].ctypes.data + planes[0].strides[0] * y, planes[1].ctypes.data + planes[1].strides[0] * (y // 2),
             planes[2].ctypes.data + planes[2].strides[0] * (y // 2)] for y in range(H)]
    ts = []
    for r in range(reps):
        t0 = time.perf_counter()
        f["seeds"](fg, W, H)
        for y in range(H):
            line(fg, rows[y][0], rows[y][1], rows[y][2], y, W)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"host_add_grain_line_one_thread_ms_median": round(1e3 * float(np.median(ts)), 2), "reps": reps}))


def device(reps):
    import vvdec_amd
    import film_grain_ref
    from vvdec_amd import synth
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        bank = film_grain_ref.expected([], [("fgc", _sei())], 10, 1, tmp, "probe")[0][0]
    rec = vvdec_amd.Reconstructor(W, H, num_slots=2, num_streams=1)
    rec.write_picture(0, synth.natural_picture(W, H, 7))
    rec.set_film_grain(bank)
    outs = [np.zeros((H >> (1 if c else 0), W >> (1 if c else 0)), np.uint16) for c in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
    strides = (C.c_size_t * 3)(*[o.strides[0] for o in outs])
    tg, tp = [], []
    for r in range(reps + 3):
        t0 = time.perf_counter()
        rec._check(rec.L.vvr_read_output_grain(rec.ctx, 0, 0, 0, W, H, 2, ptrs, strides))
        t1 = time.perf_counter()
        for c in range(3):
            s = 1 if c else 0
            rec._check(rec.L.vvr_read_output(rec.ctx, 0, c, 0, 0, W >> s, H >> s, 2, outs[c].ctypes.data, outs[c].strides[0]))
        tg.append(t1 - t0)
        tp.append(time.perf_counter() - t1)
    rec.close()
    g, p = float(np.median(tg[3:])), float(np.median(tp[3:]))
    print(json.dumps({"grain_call_ms_median": round(1e3 * g, 3), "grain_call_ms_min": round(1e3 * min(tg[3:]), 3),
                      "three_read_output_ms_median": round(1e3 * p, 3), "three_read_output_ms_min": round(1e3 * min(tp[3:]), 3),
                      "ratio_median": round(g / p, 3), "result_MB": round(sum(o.nbytes for o in outs) / 1e6, 1), "reps": reps}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--host":
        host(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
        device(reps)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--host", "3"], timeout=600)
