"""What it costs to verify the decoded picture hash of every picture while a 10-bit 4:2:0 3840x2160 random-access stream is reconstructed
(bench.py's 4k stream and window: K timed pictures behind pre-roll and warm-up, every window from the first picture of the stream), three ways
in turn in one process:
  N  no hashing
  Q  a CRC request per picture through the output queue (vvr_hash_submit behind the picture, without blocking; collected when 8 are in flight)
  S  vvr_picture_hash( CRC ) per picture, which drains the context every time
The ways alternate window by window; the median, minimum and maximum of --windows windows are reported, and whether Q's median lies within the
spread (minimum .. maximum) of N's windows.  The digests of Q and S for the timed pictures are compared first (they must be identical).
--frame N: one 3840x2160 10-bit frame instead of a stream: the kernel time (HIP events around the launches, vvr_get_stats) of a CRC and of a
checksum, k_hash_rows + k_hash_combine of a request against the three k_plane_hash_rows launches of vvr_picture_hash, N repeats of each in turn,
median / minimum / maximum; and the time from vvr_hash_submit to the return of vvr_output_wait.
Usage: python tools/hash_verify_cost.py [--steps 20] [--warmup 5] [--windows 5] [--out FILE]
       python tools/hash_verify_cost.py --frame 30 [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v, digits=4):
    return {"median": round(float(np.median(v)), digits), "min": round(float(min(v)), digits), "max": round(float(max(v)), digits)}


def frame_mode(a):
    import vvdec_amd
    from vvdec_amd import abi
    W, H = 3840, 2160
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    rng = np.random.default_rng(7)
    rec.write_picture(0, [rng.integers(0, 1024, (H >> s, W >> s), dtype=np.uint16) for s in (0, 1, 1)])
    rec.enable_stats()

    def kernel_ms():
        return {s["name"]: s["total_ms"] for s in rec.stats()}
    res = {"mode": "frame", "size": [W, H], "bit_depth": 10, "repeats": a.frame}
    for name, method in (("crc", abi.HASH_CRC), ("checksum", abi.HASH_CHECKSUM)):
        new, rows, comb, old, turn = [], [], [], [], []
        for n in range(3 + a.frame):                  # (the first three rounds warm up: ring entry, scratch, code objects)
            k0, t0 = kernel_ms(), time.perf_counter()
            queued = rec.hash_wait(rec.hash_submit(0, method=method))[0]
            t1, k1 = time.perf_counter(), kernel_ms()
            assert rec.picture_hash(0, method) == queued
            k2 = kernel_ms()
            if n >= 3:
                rows.append(k1["k_hash_rows"] - k0.get("k_hash_rows", 0.))
                comb.append(k1["k_hash_combine"] - k0.get("k_hash_combine", 0.))
                new.append(rows[-1] + comb[-1])
                old.append(k2["k_plane_hash_rows"] - k1.get("k_plane_hash_rows", 0.))
                turn.append((t1 - t0) * 1e3)
        res[name] = {"k_hash_rows_ms": spread(rows), "k_hash_combine_ms": spread(comb), "request_kernels_ms": spread(new),
                     "k_plane_hash_rows_three_launches_ms": spread(old), "submit_to_completion_ms": spread(turn)}
    rec.close()
    return res


def stream_mode(a):
    import bench
    import vvdec_amd
    from vvdec_amd import abi, synth
    from concurrent.futures import ThreadPoolExecutor
    W, H, mix, intra_period, _ = bench.CONFIGS["4k"]
    if a.width:
        W, H = a.width, a.height
    tools = bench._tools(abi) | abi.TOOL_LFP_ON_DEVICE | abi.TOOL_AFFINE_MV_ON_DEVICE
    K, Wm = a.steps, a.warmup
    plans, nslots, orders = bench.stream_plan("4k", 32, intra_period, 8, 48, K, Wm)
    order, first = orders[8]
    rec = vvdec_amd.Reconstructor(W, H, num_slots=nslots, num_streams=4, host_threads=8)
    L, ctx = rec.L, rec.ctx
    needed = max(order[:first + K]) + 1
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as tp:
        descs = list(tp.map(lambda pl: synth.picture_for_plan(pl, W, H, seed=1234, tool_flags=tools, alloc=rec.host_array, **mix), plans[:needed]))
    cpics = [d.c() for d in descs]
    timed = order[first:first + K]
    # one request and one digest buffer per ring entry
    bufs = [(C.c_uint8 * 6)() for _ in range(8)]
    reqs = []
    for b in bufs:
        r = abi.HashRequest()
        r.struct_size, r.method, r.digest = C.sizeof(abi.HashRequest), abi.HASH_CRC, C.addressof(b)
        reqs.append(r)
    sync_buf, sync_len = (C.c_uint8 * 48)(), C.c_int()

    def run(way, idx, digests=None):
        if way == "N":
            for i in idx:
                rec.submit_c(cpics[i])
            rec.sync()
            return
        if way == "S":
            for i in idx:
                rec.submit_c(cpics[i])
                rec._check(L.vvr_picture_hash(ctx, plans[i].slot, abi.HASH_CRC, sync_buf, C.byref(sync_len)))
                if digests is not None:
                    digests.append(bytes(sync_buf[:6]))
            rec.sync()
            return
        pending, flight, free = [], [], list(range(8))

        def collect():
            t, e = flight.pop(0)
            rec._check(L.vvr_output_wait(ctx, t))
            if digests is not None:
                digests.append(bytes(bufs[e]))
            free.append(e)

        def drain(block):
            while pending:
                if not free:
                    collect()
                r = reqs[free[0]]
                r.job, r.slot = pending[0]
                r.blocking = 1 if block else 0
                t = rec._check(L.vvr_hash_submit(ctx, C.byref(r)))
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

    res = {"mode": "stream", "config": "4k", "size": [W, H], "steps": K, "warmup": Wm, "windows": a.windows}
    dq, ds = [], []
    window("Q", dq)
    window("S", ds)
    res["digests_Q_equal_S"] = len(dq) == K and dq == ds
    times = {w: [] for w in "NQS"}
    for w in "NQS":                                   # warm-up: every way once
        window(w)
    for _ in range(a.windows):
        for w in "NQS":
            times[w].append(window(w))
    for w, name in (("N", "no_hashing"), ("Q", "crc_request_per_picture"), ("S", "vvr_picture_hash_per_picture")):
        fps = [K / t for t in times[w]]
        res[name] = {"pictures_per_s": spread(fps, 1), "window_ms": spread([t * 1e3 for t in times[w]], 3), "windows_ms": [round(t * 1e3, 3) for t in times[w]]}
    lo, hi = min(times["N"]), max(times["N"])
    for w, name in (("Q", "crc_request_per_picture"), ("S", "vvr_picture_hash_per_picture")):
        res[name]["median_within_spread_of_no_hashing"] = bool(lo <= float(np.median(times[w])) <= hi)
    rec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--width", type=int, default=0, help="stream mode: override the picture size (rehearsals)")
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # (as bench.py: one hardware queue per lane; read when HIP initialises)
    sys.path.insert(0, ROOT)
    res = frame_mode(a) if a.frame else stream_mode(a)
    res["gpu_max_hw_queues"] = os.environ.get("GPU_MAX_HW_QUEUES")      # (the value in force: set in front of the command, or the default above)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
