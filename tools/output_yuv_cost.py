"""What the Y'CbCr formats at 4:4:4 / 4:2:2 of the output queue cost (k_output_yuv), on the model of profiles/output_rgb_4k.txt: the compiler's resource
table of every instantiation, the bytes a 3840x2160 frame moves per format, and the kernels' times from one rocprofv3 kernel trace in which
k_output_yuv (storing yuv444p16, v210 and y210) runs on the same frames as the unchanged k_output_rgb storing rgb16 and k_output_frame storing p010.

  python tools/output_yuv_cost.py --table FILE          the resource table (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) as JSON
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/output_yuv_cost.py --workload [--rounds 6] [--repeats 20]
                                                        the requests: a run of its own, every format into device tensors, the formats taking turns
                                                        inside a round; the first round is warm-up
  python tools/output_yuv_cost.py --parse DIR --times FILE [--rounds 6] [--repeats 20]
                                                        per kernel the median of every round's median and the spread of those medians, as JSON
  python tools/output_yuv_cost.py --compose profiles/output_yuv_4k.txt --table FILE [--times FILE]
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
CODES = {64: "yuv444p8", 65: "yuv444p16", 66: "yuv422p8", 67: "yuv422p16", 68: "uyvy", 69: "yuy2", 70: "y210", 71: "v210", 72: "y410"}
TRACED = [("yuv444p16", "k_output_yuv", 65), ("v210", "k_output_yuv", 71), ("y210", "k_output_yuv", 70), ("rgb16", "k_output_rgb", 33), ("p010", "k_output_frame", None)]


def written(fmt, w=W, h=H):
    """bytes a frame of `fmt` writes"""
    return {"yuv444p8": 3 * w, "yuv444p16": 6 * w, "yuv422p8": 2 * w, "yuv422p16": 4 * w, "uyvy": 2 * w, "yuy2": 2 * w, "y210": 4 * w, "v210": (w + 5) // 6 * 16, "y410": 4 * w,
            "rgb16": 6 * w, "p010": 3 * w}[fmt] * h


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
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    rows = []
    for k, v in kernels.items():
        m = re.match(r"_Z12k_output_yuvILi(\d)ELi(\d+)ELb([01])EEv", k)
        if m:
            rows.append(dict(col=int(m.group(1)), fmt=CODES[int(m.group(2))], whole=bool(int(m.group(3))), **v))
    ref = {k: v for k, v in kernels.items() if k.startswith("_Z12k_output_rgbILi0ELi33ELb1ELi0E") or k.startswith("_Z14k_output_frame")}
    with open(a.table, "w") as f:
        json.dump({"k_output_yuv": rows, "for_comparison": ref}, f, indent=1)
    print("%d instantiations of k_output_yuv, scratch in %d" % (len(rows), sum(1 for r in rows if r["scratch"])))


def workload(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    from vvdec_amd import abi
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (H, W))).clip(0, 1023).astype(np.uint16)
    planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16),
              (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16)]
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    rec.set_output_colour(9, False)
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    into = {}
    for fmt, _, _ in TRACED:
        shapes, dt = abi.output_plane_shapes((0, 0, W, H), fmt, None, 3)
        t = [torch.empty(s, dtype=tdt[np.dtype(dt).itemsize], device="cuda") for s in shapes]
        into[fmt] = torch.stack(t) if fmt in ("yuv444p16", "rgb16") else t[0] if len(t) == 1 else t
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for fmt, _, _ in TRACED:
            for _ in range(a.repeats):
                rec.output_wait(rec.output_submit(0, fmt=fmt, into=into[fmt]))
    rec.close()
    print("workload done: %d rounds x %d requests of %s" % (a.rounds, a.repeats, ", ".join(f for f, _, _ in TRACED)))


def parse(a):
    files = glob.glob(os.path.join(a.parse, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {fmt: [] for fmt, _, _ in TRACED}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            row = {k.lower(): v for k, v in row.items()}
            name = row["kernel_name"]
            for fmt, kernel, code in TRACED:
                if kernel in name and (code is None or re.search(r"%s(<\d, %d, |ILi\dELi%dE)" % (kernel, code, code), name)):      # (demangled or not)
                    spans[fmt].append((int(row["start_timestamp"]), int(row["end_timestamp"])))
    res = {"rounds": a.rounds, "repeats": a.repeats, "kernel_us": {}}
    for fmt, kernel, _ in TRACED:
        d = np.array([e - s for s, e in sorted(spans[fmt])], np.float64) / 1000.
        assert len(d) == a.rounds * a.repeats, (fmt, len(d))
        med = np.median(d.reshape(a.rounds, a.repeats)[1:], axis=1)      # (the first round is warm-up)
        res["kernel_us"][fmt] = {"kernel": kernel, "round_medians": [round(float(v), 2) for v in med], "median": round(float(np.median(med)), 2), "spread": round(float(med.max() - med.min()), 2)}
    with open(a.times, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def compose(a):
    tab = json.load(open(a.table))
    rows = tab["k_output_yuv"]
    span = lambda rs, key: "%d" % rs[0][key] if len(set(r[key] for r in rs)) == 1 else "%d - %d" % (min(r[key] for r in rs), max(r[key] for r in rs))
    out = ["output queue, Y'CbCr at 4:4:4 / 4:2:2: VVR_OUT_YUV444P8 ... VVR_OUT_Y410 (k_output_yuv), 3840x2160, 10-bit 4:2:0", "",
           "compiler's resource table (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; k_output_yuv<COL, FMT, WHOLE>, %d instantiations:" % len(rows),
           "COL the chroma position bits (4:2:2: bit 1 alone), FMT 64 .. 72, WHOLE rows of a multiple of 8 samples; v210 has one kind of store):"]
    for fmt in CODES.values():
        for whole in (True, False):
            rs = [r for r in rows if r["fmt"] == fmt and r["whole"] == whole]
            if rs:
                out.append("  %-10s %-13s %d positions   %8s VGPRs   %8s SGPRs   %6s bytes of LDS   scratch %s   occupancy %s waves/SIMD" % (
                    fmt, "whole" if whole else "pair by pair", len(rs), span(rs, "vgpr"), span(rs, "sgpr"), span(rs, "lds"), span(rs, "scratch"), span(rs, "occ")))
    out += ["  every instantiation: no scratch, no spills.  LDS: 13 760 bytes at 4:4:4 (k_output_rgb's tile: 2 x 20 x 36 staged chroma samples, 2 x 20 x 68",
            "  int32 sums), 2560 bytes at 4:2:2 (2 x 20 x 32 staged samples, no sums), 5120 bytes for v210 (2 x 20 x 16 cells of 8 bytes, three samples each).",
            "  A 4K frame is 60 x 68 = 4080 workgroups of 64 x 32 samples, for v210 40 x 68 = 2720 of 96 x 32.", "  for comparison:"]
    for k, v in tab["for_comparison"].items():
        out.append("    %-60s %d VGPRs, %d SGPRs, %d bytes of LDS, scratch %d, occupancy %d" % (k[:60], v["vgpr"], v["sgpr"], v["lds"], v["scratch"], v["occ"]))
    out += ["", "bytes per 4K frame: %.1f MB read by every format (12.4 M samples of 2 bytes; k_output_rgb and k_output_frame storing P010 alike); written:" % (W * H * 3 / 1e6)]
    for fmt in list(CODES.values()) + ["rgb16", "p010"]:
        out.append("  %-10s %5.1f MB%s" % (fmt, written(fmt) / 1e6, "   (k_output_rgb)" if fmt == "rgb16" else "   (k_output_frame)" if fmt == "p010" else ""))
    out += ["", "kernel time (rocprofv3 --kernel-trace --stats, a run of its own: tools/output_yuv_cost.py --workload; k_output_yuv storing yuv444p16, v210 and y210",
            "beside the unchanged k_output_rgb storing rgb16 and k_output_frame storing p010, on the same frame in the same trace, into device tensors):"]
    if not a.times:
        out.append("  not measured")
    else:
        t = json.load(open(a.times))
        out.append("  one MI355X, one process; %d rounds in which the formats take turns, %d launches of each in a round, the first round warm-up.  Per format: the" % (t["rounds"], t["repeats"]))
        out.append("  median of the rounds' medians, their spread (largest - smallest) and the round medians, in microseconds; GB/s: read + written bytes over the median.")
        for fmt, s in t["kernel_us"].items():
            out.append("  %-10s %-15s median %7.2f   spread %5.2f   %5.0f GB/s   %r" % (fmt, s["kernel"], s["median"], s["spread"], (W * H * 3 + written(fmt)) / s["median"] / 1e3, s["round_medians"]))
        k = t["kernel_us"]
        y, r = k["yuv444p16"], k["rgb16"]
        slack = max(y["spread"], r["spread"])
        out += ["", "  the yardstick: k_output_rgb storing rgb16 in this trace, %.2f us.  yuv444p16 reads and writes the same bytes and does less arithmetic: %.2f us, %s" % (
                r["median"], y["median"], "not slower beyond the spread of the repeats (%.2f us)." % slack if y["median"] <= r["median"] + slack else
                "SLOWER by %.2f us, more than the spread of the repeats (%.2f us): the expectation fails." % (y["median"] - r["median"], slack))]
        for fmt in ("y210", "v210"):
            out.append("  %s writes %.0f %% of those bytes: %.2f us, %.0f %% of yuv444p16's time." % (fmt, 100. * written(fmt) / written("yuv444p16"), k[fmt]["median"], 100. * k[fmt]["median"] / y["median"]))
    out += ["", "pictures per second delivered through the queue, and one frame alone against the parent commit:", "  not measured"]
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
