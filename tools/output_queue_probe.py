"""Pictures per second DELIVERED TO THE HOST while a 10-bit 4:2:0 3840x2160 random-access stream is reconstructed (bench.py's 4k stream and window:
K timed pictures behind pre-roll and warm-up, every window from the first picture of the stream), these ways in turn in one process:
  A  the synchronous calls: vvr_wait, then three vvr_read_output (each drains the context) - the only way to output every picture before the queue
  B  the output queue, VVR_OUT_PLANAR16 into pageable memory (the rows leave pinned staging in vvr_output_wait)
  C  the output queue, VVR_OUT_PLANAR16 into memory of vvr_host_alloc (the device copies straight there)
  D  the output queue, VVR_OUT_PACKED10 into memory of vvr_host_alloc
  E  the output queue, VVR_OUT_P010 into memory of vvr_host_alloc
  F  the output queue, VVR_OUT_P010 into device memory (vvr_device_alloc): nothing crosses PCIe
  G  the output queue, VVR_OUT_RGB16 into device memory: one (3, H, W) tensor per request, BT.709 limited range (k_output_rgb)
  H  the output queue, VVR_OUT_RGBF16 into device memory, likewise
  I  the output queue, VVR_OUT_BGRA8 into device memory: one (H, W, 4) tensor of bytes per request
  J  the output queue, VVR_OUT_RGB24 into device memory: one (H, W, 3) tensor of bytes
  K  the output queue, VVR_OUT_RGBA16F into device memory: one (H, W, 4) tensor of halves
  L  the output queue, VVR_OUT_RGBF32 into device memory: one (3, H, W) tensor of float32, ImageNet mean and standard deviation applied
and the decode-only rate of the same window (nothing leaves the device).  The ways alternate window by window; every way runs at least --windows
windows and --min-seconds of timed work; median, minimum and maximum are reported.  Before the timed runs the outputs of A and B of the timed pictures
are compared (they must be identical).  Requests are submitted without blocking behind their picture and collected when 8 are in flight.
Kernel time: `rocprofv3 --kernel-trace --stats -- python tools/output_queue_probe.py --ways D --windows 2 --min-seconds 0` in a run of its own
(--ways FG: k_output_frame storing P010 and k_output_rgb on the same frames in one trace).
--frame N: one 3840x2160 10-bit frame instead of a stream, N repeats of every configuration in turn (planar16 and p010 into memory of
vvr_host_alloc and into device memory, every RGB format into device memory): the time of k_output_frame or k_output_rgb (HIP events around the launch, vvr_get_stats) and the time from
vvr_output_submit to the return of vvr_output_wait, median / minimum / maximum; and what a caller without the interleaved and float32 formats does
behind a planar request, timed with torch events: torch.stack( rgb8 planes, dim = -1 ), and rgbf16 .float() with mean and standard deviation.  --root DIR measures the package of another checkout of the project
(the parent commit, say) with this script, so that both can run in one call on one box; configurations that checkout does not have are left out.
Usage: python tools/output_queue_probe.py [--steps 64] [--warmup 16] [--windows 5] [--min-seconds 1.0] [--ways ABCDEFGHIJKLN] [--out FILE]
       python tools/output_queue_probe.py --frame 50 [--root DIR] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # (ImageNet's, as torchvision documents them)


def frame_mode(a):
    """one 4K 10-bit frame: kernel time and submit-to-completion time per configuration"""
    import vvdec_amd
    from vvdec_amd import abi
    W, H = 3840, 2160
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    rng = np.random.default_rng(7)
    rec.write_picture(0, [rng.integers(0, 1024, (H >> s, W >> s), dtype=np.uint16) for s in (0, 1, 1)])
    rec.enable_stats()
    win = (0, 0, W, H)

    def kernel_ms():
        return sum(s["total_ms"] for s in rec.stats() if s["name"] in ("k_output_frame", "k_output_rgb"))
    configs = {}
    if "rgb16" in abi.OUT_FORMATS:
        rec.set_output_colour(1, False)
    if hasattr(rec, "set_output_normalisation"):
        rec.set_output_normalisation(MEAN, STD)
    for fmt in ("planar16", "p010", "rgb8", "rgb16", "rgbf16", "rgbf32", "rgba8", "bgra8", "rgb24", "bgr24", "rgb10a2", "rgba16f"):
        for where in ("pinned", "device"):
            if fmt not in abi.OUT_FORMATS or (where == "device" and not hasattr(rec, "device_array")) or (fmt[:3] in ("rgb", "bgr") and where == "pinned"):
                continue
            shapes, dt = abi.output_plane_shapes(win, fmt, None, 3)
            item = np.dtype(dt).itemsize
            if where == "pinned":
                planes = [rec.host_array(r * n, dt).reshape(r, n) for r, n in shapes]
            else:
                import torch
                planes = [rec.device_array(r * n * item).view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[item]).view(r, n) for r, n in shapes]
            configs[fmt + "_" + where] = abi.output_request(0, None, win, fmt, None, (True, False), False, True, planes), planes
    times = {name: ([], []) for name in configs}
    for n in range(3 + a.frame):                  # (the first three rounds warm up: ring entries, scratch)
        for name, (req, _) in configs.items():
            k0, t0 = kernel_ms(), time.perf_counter()
            t = rec._check(rec.L.vvr_output_submit(rec.ctx, C.byref(req)))
            rec._check(rec.L.vvr_output_wait(rec.ctx, t))
            t1 = time.perf_counter()
            if n >= 3:
                times[name][0].append(kernel_ms() - k0)
                times[name][1].append((t1 - t0) * 1e3)
    res = {"mode": "frame", "size": [W, H], "bit_depth": 10, "repeats": a.frame, "root": os.path.abspath(a.root or ROOT)}
    for name, (k, t) in times.items():
        res[name] = {("k_output_rgb_ms" if name[:3] in ("rgb", "bgr") else "k_output_frame_ms"): {"median": round(float(np.median(k)), 4), "min": round(min(k), 4), "max": round(max(k), 4)},
                     "submit_to_completion_ms": {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}}
    # what a caller does today behind the planar request (the planes are in device memory already): the extra passes, torch events around them
    if "rgb8_device" in configs and "rgbf16_device" in configs:
        import torch
        p8 = configs["rgb8_device"][1]
        pf = [p.view(torch.float16) for p in configs["rgbf16_device"][1]]
        mean, std = [torch.tensor(v, dtype=torch.float32, device=p8[0].device).view(3, 1, 1) for v in (MEAN, STD)]
        todays = {"torch_stack_of_rgb8": lambda: torch.stack(p8, dim=-1), "float_and_normalise_of_rgbf16": lambda: (torch.stack(pf).float() - mean) / std}
        for name, fn in todays.items():
            ms = []
            for n in range(3 + a.frame):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if n >= 3:
                    ms.append(e0.elapsed_time(e1))
            res[name] = {"torch_ms": {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}}
    rec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--ways", default="ABCDEFGHIJKLN")
    ap.add_argument("--config", default="4k")
    ap.add_argument("--out", default="")
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--root", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: torch brings its own HIP runtime, which has to be the one the process initialises - way F and --frame use tensors)
    sys.path.insert(0, a.root or ROOT)
    if a.frame:
        line = json.dumps(frame_mode(a))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import bench
    import vvdec_amd
    from vvdec_amd import abi, synth
    from concurrent.futures import ThreadPoolExecutor
    W, H, mix, intra_period, _ = bench.CONFIGS[a.config]
    tools = bench._tools(abi) | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE
    K, Wm = a.steps, a.warmup
    plans, nslots, orders = bench.stream_plan(a.config, 32, intra_period, 8, 48, K, Wm)
    order, first = orders[8]
    rec = vvdec_amd.Reconstructor(W, H, num_slots=nslots, num_streams=4, host_threads=8)
    L, ctx = rec.L, rec.ctx
    needed = max(order[:first + K]) + 1
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as tp:
        descs = list(tp.map(lambda pl: synth.picture_for_plan(pl, W, H, seed=1234, tool_flags=tools, alloc=rec.host_array, **mix), plans[:needed]))
    cpics = [d.c() for d in descs]
    timed = order[first:first + K]

    # destinations: one set per ring entry and kind
    def planes(fmt, pinned, device=False):
        shapes, dt = abi.output_plane_shapes((0, 0, W, H), fmt, None, 3)
        if device:
            import torch
            item = np.dtype(dt).itemsize
            tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[item]
            if len(shapes) == 3 and fmt.startswith("rgb"):      # (as a model takes it: the planes of one contiguous (3, H, W) tensor)
                return list(rec.device_array(3 * H * W * item).view(tdt).view(3, H, W))
            return [rec.device_array(r * n * item).view(tdt).view(r, n) for r, n in shapes]      # (an interleaved format: the (H, W, C) tensor as its one plane of rows)
        return [rec.host_array(r * n, dt).reshape(r, n) if pinned else np.zeros((r, n), dt) for r, n in shapes]
    sets = {"B": ("planar16", [planes("planar16", False) for _ in range(8)]), "C": ("planar16", [planes("planar16", True) for _ in range(8)]),
            "D": ("packed10", [planes("packed10", True) for _ in range(8)])}
    if "E" in a.ways:
        sets["E"] = ("p010", [planes("p010", True) for _ in range(8)])
    if "F" in a.ways:
        sets["F"] = ("p010", [planes("p010", False, True) for _ in range(8)])
    if "L" in a.ways and hasattr(rec, "set_output_normalisation"):
        rec.set_output_normalisation(MEAN, STD)
    for way, fmt in (("G", "rgb16"), ("H", "rgbf16"), ("I", "bgra8"), ("J", "rgb24"), ("K", "rgba16f"), ("L", "rgbf32")):
        if way in a.ways and fmt in abi.OUT_FORMATS:      # (--root of a checkout without the RGB formats: the ways are left out)
            rec.set_output_colour(1, False)
            sets[way] = (fmt, [planes(fmt, False, True) for _ in range(8)])
    reqs = {w: [abi.output_request(0, 0, (0, 0, W, H), fmt, None, (True, False), False, False, p) for p in ps] for w, (fmt, ps) in sets.items()}
    sync_out = planes("planar16", False)
    pcie = {"A": sum(p.nbytes for p in sync_out), "B": sum(p.nbytes for p in sets["B"][1][0]), "C": sum(p.nbytes for p in sets["C"][1][0]),
            "D": sum(p.nbytes for p in sets["D"][1][0]), "E": W * H * 3, "F": 0, "G": 0, "H": 0, "I": 0, "J": 0, "K": 0, "L": 0, "N": 0}

    def run(way, idx, digests=None):
        """the pictures `idx` through vvr_submit, every one of them delivered the way `way` says"""
        if way == "N":
            for i in idx:
                rec.submit_c(cpics[i])
            rec.sync()
            return
        if way == "A":
            for i in idx:
                job = rec.submit_c(cpics[i])
                rec._check(L.vvr_wait(ctx, job))
                for c, o in enumerate(sync_out):
                    rec._check(L.vvr_read_output(ctx, plans[i].slot, c, 0, 0, o.shape[1], o.shape[0], 2, o.ctypes.data, o.strides[0]))
                if digests is not None:
                    digests.append(hashlib.blake2b(b"".join(o.tobytes() for o in sync_out)).digest())
            rec.sync()
            return
        pending, flight, free = [], [], list(range(8))

        def collect():
            t, e = flight.pop(0)
            rec._check(L.vvr_output_wait(ctx, t))
            if digests is not None:
                digests.append(hashlib.blake2b(b"".join(o.tobytes() for o in sets[way][1][e])).digest())
            free.append(e)

        def drain(block):
            while pending:
                if not free:
                    collect()
                job, slot = pending[0]
                r = reqs[way][free[0]]
                r.job, r.slot, r.blocking = job, slot, 1 if block else 0
                t = rec._check(L.vvr_output_submit(ctx, C.byref(r)))
                if t == abi.VVR_NOT_READY:
                    return
                pending.pop(0)
                flight.append((t, free.pop(0)))
        for i in idx:
            pending.append((rec.submit_c(cpics[i]), plans[i].slot))
            drain(False)
        drain(True)
        while flight:
            collect()
        rec.sync()

    def window(way, digests=None):
        run("N", order[:first - Wm])
        run(way, order[first - Wm:first])
        t0 = time.perf_counter()
        run(way, timed, digests)
        return time.perf_counter() - t0

    res = {"config": a.config, "size": [W, H], "steps": K, "warmup": Wm, "pcie_bytes_per_frame": pcie}
    if "A" in a.ways and "B" in a.ways:
        da, db = [], []
        window("A", da)
        window("B", db)
        res["outputs_A_equal_B"] = len(da) == K and da == db
    ways = [w for w in "ABCDEFGHIJKLN" if w in a.ways and (w in "AN" or w in sets)]
    times = {w: [] for w in ways}
    for w in ways:                                   # warm-up: every way once (ring entries, pinned staging)
        window(w)
    while any(len(times[w]) < a.windows or sum(times[w]) < a.min_seconds for w in ways):
        for w in ways:
            times[w].append(window(w))
    for w in ways:
        fps = sorted(K / t for t in times[w])
        res["decode_only" if w == "N" else w] = {"pictures_per_s_median": round(float(np.median(fps)), 1), "min": round(fps[0], 1), "max": round(fps[-1], 1),
                                                 "windows": len(fps), "timed_seconds": round(sum(times[w]), 3),
                                                 "pcie_GB_per_s_at_median": round(float(np.median(fps)) * pcie[w] / 1e9, 2)}
    rec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
