"""What 8-bit Y'CbCr frames from 10-bit pictures cost (vvr_set_output_narrowing: k_output_narrow and the NARROW variants of k_output_yuv), on the
model of profiles/output_yuv_4k.txt: the compiler's resource table of the new kernel and the new instantiations, the bytes a 3840x2160 frame
moves, and the kernels' times from one rocprofv3 kernel trace in which k_output_narrow stores nv12 in each of the three modes beside the
unchanged k_output_frame storing p010, on the same frame.

  python tools/output_narrow_cost.py --table FILE          the resource table (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) as JSON
  rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/output_narrow_cost.py --workload [--rounds 6] [--repeats 20]
                                                           the requests: a run of its own, into device tensors, the modes and p010 taking turns
                                                           inside a round; the first round is warm-up
  python tools/output_narrow_cost.py --parse DIR --times FILE [--rounds 6] [--repeats 20]
                                                           per request kind the median of every round's median and the spread of those medians, as JSON
  python tools/output_narrow_cost.py --compose profiles/output_narrow_4k.txt --table FILE [--times FILE]
                                                           the sheet; without --times the times are written as "not measured" """
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
CODES = {64: "yuv444p8", 66: "yuv422p8", 68: "uyvy", 69: "yuy2"}
# the order of a round: nv12 in the three modes (k_output_narrow: told apart by their place in the round), then p010 (k_output_frame)
TRACED = [("nv12 truncate", "k_output_narrow", "truncate"), ("nv12 round", "k_output_narrow", "round"), ("nv12 dither", "k_output_narrow", "dither"), ("p010", "k_output_frame", None)]
READ = W * H * 3                                   # 12.4 M samples of 2 bytes
WRITTEN = {"nv12": W * H * 3 // 2, "planar8": W * H * 3 // 2, "p010": W * H * 3, "yuv444p8": W * H * 3, "yuv422p8": W * H * 2, "uyvy": W * H * 2, "yuy2": W * H * 2}


def table(a):
    src = os.path.join(ROOT, "vvdec_amd", "csrc")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-scalarize-global-loads=false", "-w", "-c", "--cuda-device-only",
                          "-x", "hip", "vvr_kernels.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=src, capture_output=True, text=True, check=True)
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    rows, before = [], []
    for k, v in kernels.items():
        m = re.match(r"_Z12k_output_yuvILi(\d)ELi(\d+)ELb([01])ELb1EEv", k)
        if m:
            rows.append(dict(col=int(m.group(1)), fmt=CODES[int(m.group(2))], whole=bool(int(m.group(3))), **v))
        m = re.match(r"_Z12k_output_yuvILi(\d)ELi(\d+)ELb([01])EEv", k)
        if m and int(m.group(2)) in CODES:
            before.append(dict(col=int(m.group(1)), fmt=CODES[int(m.group(2))], whole=bool(int(m.group(3))), **v))
    one = {k: v for k, v in kernels.items() if k.startswith("_Z15k_output_narrow") or k.startswith("_Z14k_output_frame")}
    assert len(one) == 2 and len(rows) == 20 and len(before) == 20, (list(one), len(rows), len(before))
    with open(a.table, "w") as f:
        json.dump({"k_output_yuv_narrow": rows, "k_output_yuv_same_formats_without": before, "kernels": one}, f, indent=1)
    new = rows + [v for k, v in one.items() if "narrow" in k]
    print("k_output_narrow and %d new instantiations of k_output_yuv: scratch in %d, spills in %d" % (len(rows), sum(1 for r in new if r["scratch"]), sum(1 for r in new if r["vspill"] or r["sspill"])))


def workload(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (H, W))).clip(0, 1023).astype(np.uint16)
    planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16),
              (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16)]
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    nv12 = [torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty((H // 2, W), dtype=torch.uint8, device="cuda")]
    p010 = [torch.empty((H, W), dtype=torch.int16, device="cuda"), torch.empty((H // 2, W), dtype=torch.int16, device="cuda")]
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for _, _, mode in TRACED:
            if mode:
                rec.set_output_narrowing(mode, 0)
            for _ in range(a.repeats):
                rec.output_wait(rec.output_submit(0, fmt="nv12" if mode else "p010", into=nv12 if mode else p010))
    rec.close()
    print("workload done: %d rounds x %d requests of %s" % (a.rounds, a.repeats, ", ".join(t[0] for t in TRACED)))


def parse(a):
    files = glob.glob(os.path.join(a.parse, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {"k_output_narrow": [], "k_output_frame": []}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            row = {k.lower(): v for k, v in row.items()}
            for kernel in spans:
                if kernel in row["kernel_name"]:
                    spans[kernel].append((int(row["start_timestamp"]), int(row["end_timestamp"])))
    us = {k: np.array([e - s for s, e in sorted(v)], np.float64) / 1000. for k, v in spans.items()}
    assert len(us["k_output_narrow"]) == a.rounds * 3 * a.repeats and len(us["k_output_frame"]) == a.rounds * a.repeats, {k: len(v) for k, v in us.items()}
    narrow = us["k_output_narrow"].reshape(a.rounds, 3, a.repeats)      # (in start order: round, mode, repeat)
    res = {"rounds": a.rounds, "repeats": a.repeats, "kernel_us": {}}
    for n, (what, kernel, mode) in enumerate(TRACED):
        d = narrow[:, n] if mode else us["k_output_frame"].reshape(a.rounds, a.repeats)
        med = np.median(d[1:], axis=1)      # (the first round is warm-up)
        res["kernel_us"][what] = {"kernel": kernel, "round_medians": [round(float(v), 2) for v in med], "median": round(float(np.median(med)), 2), "spread": round(float(med.max() - med.min()), 2)}
    with open(a.times, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def compose(a):
    tab = json.load(open(a.table))
    span = lambda rs, key: "%d" % rs[0][key] if len(set(r[key] for r in rs)) == 1 else "%d - %d" % (min(r[key] for r in rs), max(r[key] for r in rs))
    out = ["output queue, 8-bit Y'CbCr frames from 10-bit pictures (vvr_set_output_narrowing): VVR_OUT_PLANAR8, _NV12 (k_output_narrow), _YUV444P8, _YUV422P8, _UYVY, _YUY2",
           "(k_output_yuv<COL, FMT, WHOLE, NARROW>), 3840x2160, 10-bit 4:2:0", "",
           "compiler's resource table (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage):"]
    for k, v in sorted(tab["kernels"].items(), reverse=True):
        out.append("  %-52s %d VGPRs, %d SGPRs, %d bytes of LDS, scratch %d, spills %d + %d, occupancy %d waves/SIMD%s" % (
            k[:52], v["vgpr"], v["sgpr"], v["lds"], v["scratch"], v["vspill"], v["sspill"], v["occ"], "" if "narrow" in k else "   (unchanged, for comparison)"))
    out.append("  the %d new instantiations of k_output_yuv (NARROW; in brackets the instantiation of the same format without it, unchanged):" % len(tab["k_output_yuv_narrow"]))
    for fmt in CODES.values():
        for whole in (True, False):
            rs = [r for r in tab["k_output_yuv_narrow"] if r["fmt"] == fmt and r["whole"] == whole]
            bs = [r for r in tab["k_output_yuv_same_formats_without"] if r["fmt"] == fmt and r["whole"] == whole]
            out.append("  %-10s %-13s %d positions   %8s [%8s] VGPRs   %8s SGPRs   %6s bytes of LDS   scratch %s   spills %s   occupancy %s [%s] waves/SIMD" % (
                fmt, "whole" if whole else "pair by pair", len(rs), span(rs, "vgpr"), span(bs, "vgpr"), span(rs, "sgpr"), span(rs, "lds"), span(rs, "scratch"),
                span([dict(s=r["vspill"] + r["sspill"]) for r in rs], "s"), span(rs, "occ"), span(bs, "occ")))
    new = tab["k_output_yuv_narrow"] + [v for k, v in tab["kernels"].items() if "narrow" in k]
    out += ["  the new code: %s." % ("no scratch, no spills" if not any(r["scratch"] or r["vspill"] or r["sspill"] for r in new) else "SCRATCH OR SPILLS - see above"),
            "  k_output_narrow keeps the thresholds of a lane's 8 dwords beside its samples: %d VGPRs against k_output_frame's %d; no LDS in either." % tuple(
                [v["vgpr"] for k, v in sorted(tab["kernels"].items(), reverse=True)]), "",
            "bytes per 4K frame: %.1f MB read by every format (12.4 M samples of 2 bytes; k_output_frame storing P010 alike); written:" % (READ / 1e6)]
    for fmt, n in WRITTEN.items():
        out.append("  %-10s %5.1f MB%s" % (fmt, n / 1e6, "   (k_output_frame)" if fmt == "p010" else "   (k_output_narrow)" if fmt in ("nv12", "planar8") else "   (k_output_yuv)"))
    out += ["", "kernel time (rocprofv3 --kernel-trace --stats, a run of its own: tools/output_narrow_cost.py --workload; k_output_narrow storing nv12 in each mode",
            "beside the unchanged k_output_frame storing p010, on the same frame in the same trace, into device tensors):"]
    if not a.times:
        out.append("  not measured")
    else:
        t = json.load(open(a.times))
        out.append("  one MI355X, one process; %d rounds in which the modes and p010 take turns, %d launches of each in a round, the first round warm-up.  Per kind: the" % (t["rounds"], t["repeats"]))
        out.append("  median of the rounds' medians, their spread (largest - smallest) and the round medians, in microseconds; GB/s: read + written bytes over the median.")
        for what, s in t["kernel_us"].items():
            out.append("  %-14s %-16s median %7.2f   spread %5.2f   %5.0f GB/s   %r" % (what, s["kernel"], s["median"], s["spread"], (READ + WRITTEN[what.split()[0]]) / s["median"] / 1e3, s["round_medians"]))
        k = t["kernel_us"]
        p = k["p010"]
        out += ["", "  the yardstick: k_output_frame storing p010 in this trace, %.2f us (the parent commit's kernel, unchanged), margin: the spread of its round medians, %.2f us." % (p["median"], p["spread"])]
        for what in ("nv12 truncate", "nv12 round", "nv12 dither"):
            s = k[what]
            out.append("  %s reads the same %.1f MB and writes %.1f MB instead of %.1f: %.2f us, %s" % (what, READ / 1e6, WRITTEN["nv12"] / 1e6, WRITTEN["p010"] / 1e6, s["median"],
                       "not slower than p010 beyond that margin." if s["median"] <= p["median"] + p["spread"] else "SLOWER than p010 by %.2f us, more than that margin: the expectation fails." % (s["median"] - p["median"])))
    out += ["", "the NARROW variants of k_output_yuv, and pictures per second delivered through the queue:", "  not measured"]
    with open(a.compose, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="")
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--parse", default="")
    ap.add_argument("--times", default="")
    ap.add_argument("--compose", default="")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    if a.workload:
        workload(a)
    elif a.parse:
        parse(a)
    elif a.compose:
        compose(a)
    else:
        table(a)


if __name__ == "__main__":
    main()
