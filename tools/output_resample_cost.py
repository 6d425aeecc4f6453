"""What antialiased resampling at the output costs (vvr_set_output_resampling: k_output_resample), on the model of profiles/output_narrow_4k.txt:
the compiler's resource table of the new kernel beside k_rescale's, and the kernels' times from one rocprofv3 kernel trace in which a
3840x2160 10-bit frame leaves as 1920x1080 P010 under each filter beside the same request at filter 0 - k_rescale, unchanged - and as a
224x224 normalised RGBF32 frame under the triangle and the cubic filter, which no request without a filter can ask for.

  python tools/output_resample_cost.py --table FILE        the resource table (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) as JSON
  rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/output_resample_cost.py --workload [--rounds 6] [--repeats 10]
                                                           the requests: a run of its own, into device tensors, the kinds taking turns inside a
                                                           round; the first round is warm-up
  python tools/output_resample_cost.py --parse DIR --times FILE [--rounds 6] [--repeats 10]
                                                           per request kind the median of every round's median and the spread of those medians, as JSON
  python tools/output_resample_cost.py --compose profiles/output_resample_4k.txt --table FILE [--times FILE]
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
# the order of a round: (what, kernel, filter, size, format); a request is a launch of its kernel per plane (Y, Cb, Cr) - two where the plane shrinks by more than 4 vertically - summed
TRACED = [("1080p p010 reference", "k_rescale", None, (1920, 1080), "p010"), ("1080p p010 area", "k_output_resample", "area", (1920, 1080), "p010"),
          ("1080p p010 triangle", "k_output_resample", "triangle", (1920, 1080), "p010"), ("1080p p010 cubic", "k_output_resample", "cubic", (1920, 1080), "p010"),
          ("224 rgbf32 triangle", "k_output_resample", "triangle", (224, 224), "rgbf32"), ("224 rgbf32 cubic", "k_output_resample", "cubic", (224, 224), "rgbf32")]
READ = W * H * 3                                   # 12.4 M samples of 2 bytes


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
    one = {k: v for k, v in kernels.items() if "k_output_resample" in k or re.match(r"_Z9k_rescaleILi\d", k)}
    assert len(one) == 10, list(one)      # (k_output_resample<false>, k_output_resample_h, k_output_resample<true>; k_rescale<8>, <4> - each for the single request and with the regions of a batch)
    with open(a.table, "w") as f:
        json.dump({"kernels": one}, f, indent=1)
    print(json.dumps(one, indent=1))


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
    rec.set_output_colour(1, False)
    rec.set_output_normalisation((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    into = {"p010": [torch.empty((1080, 1920), dtype=torch.int16, device="cuda"), torch.empty((540, 1920), dtype=torch.int16, device="cuda")],
            "rgbf32": torch.empty((3, 224, 224), dtype=torch.float32, device="cuda")}
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for _, _, filt, size, fmt in TRACED:
            rec.set_output_resampling(filt)
            for _ in range(a.repeats):
                rec.output_wait(rec.output_submit(0, fmt=fmt, size=size, into=into[fmt]))
    rec.close()
    print("workload done: %d rounds x %d requests of %s" % (a.rounds, a.repeats, ", ".join(t[0] for t in TRACED)))


def parse(a):
    files = glob.glob(os.path.join(a.parse, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {"k_output_resample": [], "k_rescale": []}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            row = {k.lower(): v for k, v in row.items()}
            for kernel in spans:
                if kernel in row["kernel_name"]:
                    spans[kernel].append((int(row["start_timestamp"]), int(row["end_timestamp"])))
    us = {k: np.array([e - s for s, e in sorted(v)], np.float64) / 1000. for k, v in spans.items()}
    # in start order: round, kind, repeat, component; a plane that shrinks by more than 4 vertically is two launches (k_output_resample_h, then the vertical pass)
    parts = [2 if filt and H > 4 * size[1] else 1 for _, _, filt, size, _ in TRACED]
    per_round = sum(3 * n * a.repeats for n, t in zip(parts, TRACED) if t[2])
    assert len(us["k_output_resample"]) == a.rounds * per_round and len(us["k_rescale"]) == a.rounds * a.repeats * 3, {k: len(v) for k, v in us.items()}
    new = us["k_output_resample"].reshape(a.rounds, per_round)
    old = us["k_rescale"].reshape(a.rounds, a.repeats, 3)
    res = {"rounds": a.rounds, "repeats": a.repeats, "kernel_us": {}}
    at = 0
    for n, (what, kernel, filt, size, fmt) in enumerate(TRACED):
        if filt:
            d = new[:, at:at + 3 * parts[n] * a.repeats].reshape(a.rounds, a.repeats, 3, parts[n]).sum(axis=-1)
            at += 3 * parts[n] * a.repeats
        else:
            d = old
        med = np.median(d[1:].sum(axis=-1), axis=1)      # (the first round is warm-up; a request: the sum of its launches)
        comp = np.median(d[1:].reshape(-1, 3), axis=0)
        res["kernel_us"][what] = {"kernel": kernel, "launches": 3 * parts[n], "round_medians": [round(float(v), 2) for v in med], "median": round(float(np.median(med)), 2), "spread": round(float(med.max() - med.min()), 2),
                                  "components": [round(float(v), 2) for v in comp]}
    with open(a.times, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def compose(a):
    tab = json.load(open(a.table))
    out = ["output queue, antialiased resampling for out_w / out_h (vvr_set_output_resampling): area, triangle, Keys cubic (k_output_resample), 3840x2160, 10-bit 4:2:0", "",
           "compiler's resource table (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage):"]
    for k, v in sorted(tab["kernels"].items()):
        out.append("  %-52s %d VGPRs, %d SGPRs, %d bytes of LDS, scratch %d, spills %d + %d, occupancy %d waves/SIMD%s" % (
            k[:52], v["vgpr"], v["sgpr"], v["lds"], v["scratch"], v["vspill"], v["sspill"], v["occ"], "" if "resample" in k else "   (unchanged, for comparison; its LDS is sized at launch, up to 32 KiB more)"))
    new = [v for k, v in tab["kernels"].items() if "resample" in k]
    out += ["  the new kernel: %s; its LDS does not depend on the ratio (48 rows of horizontal results, four row pieces of 1024 samples)." % ("no scratch, no spills" if not any(r["scratch"] or r["vspill"] or r["sspill"] for r in new) else "SCRATCH OR SPILLS - see above"), "",
            "kernel time (rocprofv3 --kernel-trace --stats, a run of its own: tools/output_resample_cost.py --workload; a request is a launch of its kernel per",
            "plane - Y, Cb, Cr; to 224x224 two, k_output_resample_h and the vertical pass - whose times are added; into device tensors; the tap tables are",
            "cached, nothing is uploaded per request):"]
    if not a.times:
        out.append("  not measured")
    else:
        t = json.load(open(a.times))
        out.append("  one MI355X, one process; %d rounds in which the kinds take turns, %d requests of each in a round, the first round warm-up.  Per kind: the" % (t["rounds"], t["repeats"]))
        out.append("  median of the rounds' medians, their spread (largest - smallest), the round medians and the median per component, in microseconds.")
        for what, s in t["kernel_us"].items():
            out.append("  %-22s %-18s median %8.2f   spread %6.2f   %r   Y, Cb, Cr %r" % (what, s["kernel"], s["median"], s["spread"], s["round_medians"], s["components"]))
        k = t["kernel_us"]
        p = k["1080p p010 reference"]
        out += ["", "  3840x2160 -> 1920x1080 P010.  The yardstick: the same request at filter 0 in this trace, k_rescale, %.2f us (the parent commit's kernel, unchanged);" % p["median"],
                "  margin: the spread of its round medians, %.2f us." % p["spread"]]
        for what in ("1080p p010 area", "1080p p010 triangle", "1080p p010 cubic"):
            s = k[what]
            out.append("  %-22s %8.2f us, %.2f times the yardstick: %s" % (what, s["median"], s["median"] / p["median"], "not slower beyond that margin." if s["median"] <= p["median"] + p["spread"] else "slower beyond that margin."))
        out += ["", "  3840x2160 -> 224x224 RGBF32, normalised (refused without a filter: no yardstick).  Read rate: the frame's %.1f MB (12.4 M samples of 2 bytes) over the request's six launches." % (READ / 1e6)]
        for what in ("224 rgbf32 triangle", "224 rgbf32 cubic"):
            s = k[what]
            out.append("  %-22s %8.2f us, %5.0f GB/s" % (what, s["median"], READ / s["median"] / 1e3))
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
    ap.add_argument("--repeats", type=int, default=10)
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
