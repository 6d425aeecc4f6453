"""What a statistics request of the output queue costs (vvr_stats_submit) next to the RGB request it spares: on the 3840x2160 window of one 10-bit
picture, k_output_rgb for rgb8, rgb16 and rgbf16 into a contiguous (3, h, w) device tensor, and - where the library has them - the statistics
kernels in RGB and in luma mode (k_output_stats, and k_output_stats_sum which folds the copies of the words) on that picture and on a flat frame,
the case in which every lane adds to one bin.  The configurations take turns inside a round (--repeats launches of each behind three of warm-up);
a process runs --rounds rounds and reports, per configuration, the median of every round and the spread of those medians, which is the run-to-run
spread a difference has to exceed.  The kernel time is the library's (HIP events around the launch, vvr_enable_stats / vvr_get_stats).
--yuv FILE: the picture, frame --frame of a file of 4:2:0 frames of 16-bit samples at --size (a picture some decoder wrote); without it a structured
synthetic picture (tools/output_lut3d_cost.py's).
--root DIR: import vvdec_amd from another checkout - the parent commit's, which gives the yardstick (a library without vvr_stats_submit reports the
RGB requests only).  --rgb-only: this library's RGB requests alone, in the parent's order of launches - what compares with the parent's figures
without the statistics requests in between (they read a second slot and change what the caches hold).
--compose NOTE JSON...: no measurement; writes NOTE from the JSON files of earlier runs (in the order they were made) and the compiler's resource
tables given with --tables PARENT THIS (tools/kernel_resources.sh of the two commits).
Usage: python tools/output_stats_cost.py [--yuv FILE --size 3840x2176 --frame 8] [--repeats 30] [--rounds 5] [--root DIR] [--out FILE]
       python tools/output_stats_cost.py --compose profiles/output_stats_4k.txt --tables parent.txt this.txt run1.json run2.json ..."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB = ("rgb8", "rgb16", "rgbf16")


def measure(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, a.root)
    import vvdec_amd
    PW, PH = [int(v) for v in a.size.split("x")]
    W, H = 3840, 2160
    assert PW >= W and PH >= H
    if a.yuv:
        n = PW * PH * 3 // 2
        raw = np.fromfile(a.yuv, np.uint16, n, offset=2 * n * a.frame)
        planes = [raw[:PW * PH].reshape(PH, PW), raw[PW * PH:PW * PH * 5 // 4].reshape(PH // 2, PW // 2), raw[PW * PH * 5 // 4:].reshape(PH // 2, PW // 2)]
        assert int(raw.max()) < 1024
    else:
        rng = np.random.default_rng(7)
        yy, xx = np.mgrid[0:PH, 0:PW]
        luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (PH, PW))).clip(0, 1023).astype(np.uint16)
        planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (PH // 2, PW // 2))).clip(0, 1023).astype(np.uint16),
                  (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (PH // 2, PW // 2))).clip(0, 1023).astype(np.uint16)]
    flat = [np.full(planes[0].shape, 385, np.uint16), np.full(planes[1].shape, 505, np.uint16), np.full(planes[2].shape, 521, np.uint16)]
    rec = vvdec_amd.Reconstructor(PW, PH, bit_depth=10, num_slots=2, num_streams=1)
    rec.write_picture(0, planes)
    rec.write_picture(1, flat)
    rec.set_output_colour(9, False)
    rec.enable_stats()
    has = hasattr(rec, "stats_submit") and not a.rgb_only
    into = {"rgb8": torch.empty((3, H, W), dtype=torch.uint8, device="cuda"), "rgb16": torch.empty((3, H, W), dtype=torch.int16, device="cuda"),
            "rgbf16": torch.empty((3, H, W), dtype=torch.float16, device="cuda")}
    torch.cuda.synchronize()
    configs = [("rgb", fmt, 0) for fmt in RGB]
    if has:
        configs += [("stats", mode, slot) for slot in (0, 1) for mode in ("rgb", "luma")]
    names = ("k_output_rgb", "k_output_stats", "k_output_stats_sum")

    def kernel_ms():
        st = {s["name"]: s["total_ms"] for s in rec.stats()}
        return [st.get(k, 0.) for k in names]

    medians = {c: [] for c in configs}
    for _ in range(a.rounds):
        times = {c: [] for c in configs}
        for k in range(3 + a.repeats):
            for c in configs:
                kind, what, slot = c
                k0 = kernel_ms()
                if kind == "rgb":
                    rec.output_wait(rec.output_submit(slot, window=(0, 0, W, H), fmt=what, into=into[what]))
                else:
                    rec.stats_wait(rec.stats_submit(slot, window=(0, 0, W, H), mode=what))
                if k >= 3:
                    times[c].append([b - a_ for a_, b in zip(k0, kernel_ms())])
        for c in configs:
            medians[c].append([float(v) for v in np.median(np.array(times[c]), axis=0)])
    rec.close()
    res = {"size": [W, H], "bit_depth": 10, "picture": "%s, frame %d" % (os.path.basename(a.yuv), a.frame) if a.yuv else "structured synthetic", "repeats": a.repeats,
           "rounds": a.rounds, "library": vvdec_amd.lib().vvr_version().decode(), "root": os.path.basename(os.path.abspath(a.root)) + (", RGB requests only" if a.rgb_only else ""), "kernel_us": {}}
    for (kind, what, slot), m in medians.items():
        m = np.array(m) * 1000
        if kind == "rgb":
            res["kernel_us"]["request %s" % what] = summary(m[:, 0])
        else:
            name = "statistics %s mode, %s" % (what, "flat frame" if slot else "the picture")
            res["kernel_us"][name] = summary(m[:, 1] + m[:, 2])
            res["kernel_us"][name + ": k_output_stats_sum alone"] = summary(m[:, 2])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def summary(v):
    return {"round_medians": [round(float(x), 2) for x in v], "median": round(float(np.median(v)), 2), "spread": round(float(v.max() - v.min()), 2)}


def compose(a):
    runs = [json.load(open(p)) for p in a.inputs]
    out = ["Light-level statistics of the output queue (vvr_stats_submit): the compiler's resource table and the kernels' time on the 3840x2160 window of",
           "one 10-bit picture, next to the RGB request of the same window into a contiguous (3, 2160, 3840) device tensor that a caller without the",
           "statistics request would pull over PCIe and reduce on the host.", ""]
    if a.tables:
        parent = [l.rstrip() for l in open(a.tables[0])]
        this = [l.rstrip() for l in open(a.tables[1])]
        new = [l for l in this if l not in parent]
        gone = [l for l in parent if l not in this]
        out += ["== Compiler table (tools/kernel_resources.sh: hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) ==",
                "The parent commit's table has %d lines, this commit's %d.  Lines of the parent's table that this commit's does not have: %d%s" % (len(parent), len(this), len(gone), " - every kernel the" if not gone else ""),
                "library had, the %d instantiations of k_output_rgb among them, keeps its line." % sum("k_output_rgb" in l for l in parent) if not gone else "\n".join(gone),
                "The lines this commit adds (format class 255: the statistics class of k_output_rgb, by chroma position and kind of store):", ""] + new + [""]
    out += ["== Kernel time at 4K ==",
            "Measured on one MI355X in one session, the processes in the order below.  A process runs %d rounds; in a round the configurations take turns," % runs[0]["rounds"],
            "%d timed launches of each behind three of warm-up; the kernel time is HIP events around the launch (vvr_enable_stats).  Picture: %s" % (runs[0]["repeats"], runs[0]["picture"]),
            "(window 0, 0, 3840, 2160, BT.2020 limited range); the flat frame: Y 385, Cb 505, Cr 521 everywhere.  A statistics request's time is",
            "k_output_stats (RGB mode: the statistics class of k_output_rgb) plus k_output_stats_sum.  Per configuration: the median of the round",
            "medians, their spread (largest - smallest) and the round medians, in microseconds.", ""]
    for n, r in enumerate(runs):
        out.append("-- process %d: %s (%s)" % (n + 1, r["root"], r["library"]))
        for name, s in r["kernel_us"].items():
            out.append("  %-58s median %7.2f  spread %5.2f  %r" % (name, s["median"], s["spread"], s["round_medians"]))
        out.append("")
    old = [r for r in runs if not any(k.startswith("statistics") for k in r["kernel_us"])]
    new = [r for r in runs if any(k.startswith("statistics") for k in r["kernel_us"])]
    if old and new:
        def rng(rs, key):
            v = [x for r in rs for x in r["kernel_us"][key]["round_medians"]]
            return min(v), max(v), float(np.median([r["kernel_us"][key]["median"] for r in rs]))
        out.append("Requests of the existing formats, parent against this commit (smallest .. largest round median over the processes; median of the processes' medians):")
        for fmt in RGB:
            p, t = rng(old, "request " + fmt), rng(new, "request " + fmt)
            inside = p[0] <= t[0] and t[1] <= p[1]
            out.append("  %-7s parent %6.2f .. %6.2f (%6.2f)   this %6.2f .. %6.2f (%6.2f)   %s" % (fmt, p[0], p[1], p[2], t[0], t[1], t[2],
                       "every round median of this commit inside the parent's range" if inside else "this commit's round medians leave the parent's range by %.2f us at most" % max(p[0] - t[0], t[1] - p[1])))
        out.append("")
        y = rng(old, "request rgb16")
        spread = max(r["kernel_us"]["request rgb16"]["spread"] for r in old)
        out.append("The yardstick: the parent's rgb16 request, %.2f us (round medians %.2f .. %.2f, spread inside a process up to %.2f)." % (y[2], y[0], y[1], spread))
        nat, fl = rng(new, "statistics rgb mode, the picture"), rng(new, "statistics rgb mode, flat frame")
        lnat, lfl = rng(new, "statistics luma mode, the picture"), rng(new, "statistics luma mode, flat frame")
        out.append("RGB-mode statistics of the picture: %.2f us (%.2f .. %.2f): %s" % (nat[2], nat[0], nat[1],
                   "not longer than that request." if nat[2] <= y[2] + spread else "LONGER than that request by %.2f us, more than the parent's spread." % (nat[2] - y[2])))
        out.append("RGB-mode statistics of the flat frame: %.2f us (%.2f .. %.2f), %.2f times the picture's: %s" % (fl[2], fl[0], fl[1], fl[2] / nat[2],
                   "MORE THAN TWICE - the handling of conflicts is not doing its job." if fl[2] > 2 * nat[2] else "run merging, the uniform path and the copies of the words keep it %s." % ("within the picture's time" if fl[2] <= nat[2] else "within twice the picture's time, but above it")))
        out.append("Luma mode: %.2f us on the picture, %.2f us on the flat frame." % (lnat[2], lfl[2]))
    with open(a.compose, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yuv", default="")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default="")
    ap.add_argument("--rgb-only", action="store_true")
    ap.add_argument("--compose", default="")
    ap.add_argument("--tables", nargs=2, default=None)
    ap.add_argument("inputs", nargs="*")
    a = ap.parse_args()
    if a.compose:
        compose(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
