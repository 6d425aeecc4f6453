"""What a batch of regions costs against the same regions as single requests (vvr_output_submit_batch against vvr_output_submit), on the model
of tools/output_resample_cost.py: a 3840x2160 10-bit slot, 64 regions of 640 x 640 on an 8 x 8 overlapping grid, to 224 x 224 under the
triangle filter as normalised RGBF32 into one ( N, 3, H, W ) device tensor - (a) as one batch request, (b) as N single requests through the
ring of 8, the oldest waited for when the ring is full - then the same with no scaling, and both with 16 regions.  One process on the GPU.

  python tools/output_batch_cost.py --measure --out profiles/output_batch_4k.txt [--reps 20] [--warmup 3]
        wall time from the first submit to the last wait (requests built beforehand, the tensor registered once, plain ctypes calls), per
        repetition; then, in a pass of its own with vvr_enable_stats, the kernel time of vvr_get_stats summed over k_output_resample and
        k_output_rgb.  Median and spread (smallest .. largest) of the repetitions behind the warm-up.
  python tools/output_batch_cost.py --compare PARENT.json THIS.json --out profiles/output_batch_4k.txt
        appends the single-request kernels of two runs of tools/output_resample_cost.py --parse (the parent commit's library and this one, same
        box, same session): per kind, this commit's median against the parent's median and the spread the tool shows for the parent"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
KERNELS = ("k_output_resample", "k_output_rgb")


def grid(n_side, win):
    xs = [int(round(i * (W - win) / (n_side - 1))) & ~1 for i in range(n_side)]
    ys = [int(round(j * (H - win) / (n_side - 1))) & ~1 for j in range(n_side)]
    return [(x, y) for y in ys for x in xs]


def measure(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    from vvdec_amd import abi
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (H, W))).clip(0, 1023).astype(np.uint16)
    planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3).clip(0, 1023).astype(np.uint16), (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4).clip(0, 1023).astype(np.uint16)]
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    L, ctx = rec.L, rec.ctx
    rec.write_picture(0, planes)
    rec.set_output_colour(1, False)
    rec.set_output_normalisation(*NORM)
    rec.set_output_resampling("triangle")
    rec.sync()
    results = []
    for label, win, size, side in (("64 regions 640x640 -> 224x224, triangle", 640, (224, 224), 8), ("64 regions 640x640, no scaling", 640, None, 8),
                                   ("16 regions 640x640 -> 224x224, triangle", 640, (224, 224), 4), ("16 regions 640x640, no scaling", 640, None, 4)):
        origins = grid(side, win)
        n = len(origins)
        ow, oh = size or (win, win)
        out = torch.empty((n, 3, oh, ow), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        plane, region = oh * ow * 4, 3 * oh * ow * 4
        assert L.vvr_device_register(ctx, out.data_ptr(), n * region) == abi.VVR_OK

        def request(x, y, base):
            r = abi.OutputRequest()
            r.struct_size, r.slot, r.job = C.sizeof(abi.OutputRequest), 0, -1
            r.x, r.y, r.w, r.h = x, y, win, win
            r.out_w, r.out_h = size or (0, 0)
            r.collocated, r.format, r.grain, r.blocking = 1, abi.OUT_FORMATS["rgbf32"], 0, 1
            for k in range(3):
                r.dst[k], r.dst_stride_bytes[k] = base + k * plane, ow * 4
            return r
        breq = request(0, 0, out.data_ptr())
        batch, keep = abi.output_batch(origins, [region] * 3)
        singles = [request(x, y, out.data_ptr() + i * region) for i, (x, y) in enumerate(origins)]

        def as_batch():
            t = L.vvr_output_submit_batch(ctx, C.byref(breq), C.byref(batch))
            assert t >= 2, L.vvr_last_error(ctx)
            assert L.vvr_output_wait(ctx, t) == abi.VVR_OK

        def as_singles():
            flight = []
            for r in singles:
                if len(flight) == 8:
                    assert L.vvr_output_wait(ctx, flight.pop(0)) == abi.VVR_OK
                t = L.vvr_output_submit(ctx, C.byref(r))
                assert t >= 2, L.vvr_last_error(ctx)
                flight.append(t)
            for t in flight:
                assert L.vvr_output_wait(ctx, t) == abi.VVR_OK

        def kernel_ms():
            return sum(s["total_ms"] for s in rec.stats() if s["name"] in KERNELS)
        # the two paths store the same bytes
        as_batch()
        first = out.clone()
        out.zero_()
        torch.cuda.synchronize()
        as_singles()
        same = bool(torch.equal(first, out))
        entry = {"what": label, "regions": n, "same_bytes": same}
        for name, run in (("batch", as_batch), ("singles", as_singles)):
            wall = []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                run()
                wall.append((time.perf_counter() - t0) * 1e6)
            wall = np.array(wall[a.warmup:])
            rec.enable_stats(True)
            kern = []
            for rep in range(a.warmup + a.reps):
                k0 = kernel_ms()
                run()
                kern.append((kernel_ms() - k0) * 1e3)
            rec.enable_stats(False)
            kern = np.array(kern[a.warmup:])
            entry[name] = {"wall_us": [round(float(np.median(wall)), 1), round(float(wall.min()), 1), round(float(wall.max()), 1)],
                           "kernel_us": [round(float(np.median(kern)), 1), round(float(kern.min()), 1), round(float(kern.max()), 1)]}
        results.append(entry)
        assert L.vvr_device_unregister(ctx, out.data_ptr()) == abi.VVR_OK
        del out, first
    rec.close()
    lines = ["output queue, many regions of one picture as a batch in one request (vvr_output_submit_batch) against the same regions as single requests",
             "(vvr_output_submit through the ring of 8, the oldest waited for when the ring is full); 3840x2160, 10-bit 4:2:0 slot, regions on an overlapping",
             "grid, normalised RGBF32 into one ( N, 3, H, W ) device tensor (stored by k_output_rgb itself in both paths: no copies).", "",
             "one MI355X, one process (tools/output_batch_cost.py --measure); %d repetitions behind %d of warm-up, the paths one after the other per case." % (a.reps, a.warmup),
             "wall: from the first submit to the last wait, requests built beforehand, plain ctypes calls.  kernel: vvr_get_stats, k_output_resample +",
             "k_output_rgb, in a pass of its own with vvr_enable_stats (its events are not part of the wall figures).  median (smallest .. largest), microseconds.", ""]
    for e in results:
        b, s = e["batch"], e["singles"]
        lines.append("%s   [the two paths store the same bytes: %s]" % (e["what"], "yes" if e["same_bytes"] else "NO"))
        for name, d in (("(a) one batch request", b), ("(b) %d single requests" % e["regions"], s)):
            lines.append("  %-24s wall %9.1f (%9.1f .. %9.1f)   kernel %9.1f (%9.1f .. %9.1f)" % ((name,) + tuple(d["wall_us"]) + tuple(d["kernel_us"])))
        ratio = s["wall_us"][0] / b["wall_us"][0]
        lines.append("  wall: (a) is %s than (b), (b) / (a) = %.2f; kernel: (b) / (a) = %.2f" % ("faster" if ratio > 1 else "NOT faster", ratio, s["kernel_us"][0] / max(b["kernel_us"][0], 1e-9)))
        lines.append("")
    lines += ["Stated limits, not measurements: 256 regions per request (VVR_OUT_BATCH_MAX) and 512 MiB of device buffers of a batch in its ring entry."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
        json.dump(results, f, indent=1)
    print("\n".join(lines))


def compare(a):
    parent, this = (json.load(open(p)) for p in a.compare)
    lines = ["", "the single request is no slower: tools/output_resample_cost.py (rocprofv3 --kernel-trace, a run of its own each) with the parent commit's library",
             "and with this one, same box, same session; per request kind the kernel time of the request's launches, median of the round medians, microseconds.",
             "The margin is the spread (largest - smallest round median) the tool shows for the parent.", ""]
    for what, p in parent["kernel_us"].items():
        t = this["kernel_us"][what]
        ok = t["median"] <= p["median"] + p["spread"]
        lines.append("  %-22s %-18s parent %8.2f (spread %6.2f, rounds %r)   this %8.2f (spread %6.2f, rounds %r)   %s" % (
            what, p["kernel"], p["median"], p["spread"], p["round_medians"], t["median"], t["spread"], t["round_medians"], "within the parent's spread" if ok else "SLOWER beyond the parent's spread"))
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.measure:
        measure(a)
    elif a.compare:
        compare(a)


if __name__ == "__main__":
    main()
