"""What the 3-D LUT stage of the RGB formats costs (vvr_set_output_lut3d): k_output_rgb over the 3840x2160 window of one 10-bit picture as rgb8 and
as rgbf16 into a contiguous (3, h, w) device tensor - without a LUT and under the 17-, 33- and 65-point PQ preset, each without a transform and
behind the PQ / BT.2020 -> sRGB transform preset.  The configurations take turns inside a round (--repeats launches of each behind three rounds of
warm-up); a process runs --rounds rounds and reports, per configuration, the median of every round and the spread of those medians, which is the
run-to-run spread a difference has to exceed.  The kernel time is the library's (HIP events around the launch, vvr_enable_stats / vvr_get_stats).
--yuv FILE: the picture, one 4:2:0 frame of 16-bit samples at --size (a picture some decoder wrote: the vertex loads' cache behaviour depends on
real content); without it a structured synthetic picture (tools/output_transform_cost.py's).
--root DIR: import vvdec_amd from another checkout - the parent commit's, which gives the yardstick of the requests without a LUT (a library
without vvr_set_output_lut3d reports those only).
Usage: python tools/output_lut3d_cost.py [--yuv FILE --size 3840x2176] [--repeats 30] [--rounds 5] [--root DIR] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yuv", default="")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import vvdec_amd
    PW, PH = [int(v) for v in a.size.split("x")]
    W, H = 3840, 2160
    assert PW >= W and PH >= H
    if a.yuv:
        raw = np.fromfile(a.yuv, np.uint16, PW * PH * 3 // 2)
        planes = [raw[:PW * PH].reshape(PH, PW), raw[PW * PH:PW * PH * 5 // 4].reshape(PH // 2, PW // 2), raw[PW * PH * 5 // 4:].reshape(PH // 2, PW // 2)]
        assert int(raw.max()) < 1024
    else:
        rng = np.random.default_rng(7)
        yy, xx = np.mgrid[0:PH, 0:PW]
        luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (PH, PW))).clip(0, 1023).astype(np.uint16)
        planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (PH // 2, PW // 2))).clip(0, 1023).astype(np.uint16),
                  (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (PH // 2, PW // 2))).clip(0, 1023).astype(np.uint16)]
    rec = vvdec_amd.Reconstructor(PW, PH, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    rec.set_output_colour(9, False)
    rec.enable_stats()
    has = hasattr(rec, "set_output_lut3d")
    transform = vvdec_amd.output_transform(16, 9, "srgb", 1000., 100., 10)
    luts = {0: None}
    if has:
        luts.update({n: vvdec_amd.output_lut3d(n, 16, 9, "srgb", 1000., 100.) for n in (17, 33, 65)})
    into = {"rgb8": torch.empty((3, H, W), dtype=torch.uint8, device="cuda"), "rgbf16": torch.empty((3, H, W), dtype=torch.float16, device="cuda")}
    torch.cuda.synchronize()
    configs = [(fmt, n, xf) for fmt in ("rgb8", "rgbf16") for n in luts for xf in (False, True)]

    def kernel_ms():
        return {s["name"]: s["total_ms"] for s in rec.stats()}.get("k_output_rgb", 0.)

    medians = {c: [] for c in configs}
    for _ in range(a.rounds):
        times = {c: [] for c in configs}
        for k in range(3 + a.repeats):
            for c in configs:
                fmt, n, xf = c
                rec.set_output_transform(transform if xf else None)
                if has:
                    rec.set_output_lut3d(luts[n])
                k0 = kernel_ms()
                rec.output_wait(rec.output_submit(0, window=(0, 0, W, H), fmt=fmt, into=into[fmt]))
                if k >= 3:
                    times[c].append(kernel_ms() - k0)
        for c in configs:
            medians[c].append(float(np.median(times[c])))
    rec.close()
    res = {"size": [W, H], "bit_depth": 10, "picture": os.path.basename(a.yuv) if a.yuv else "structured synthetic", "repeats": a.repeats, "rounds": a.rounds,
           "library": vvdec_amd.lib().vvr_version().decode(), "root": a.root, "k_output_rgb_us": {}}
    for (fmt, n, xf), m in medians.items():
        name = "%s %s %s" % (fmt, "lut%d" % n if n else "no-lut", "pq-transform" if xf else "no-transform")
        res["k_output_rgb_us"][name] = {"round_medians": [round(1000 * v, 2) for v in m], "median": round(1000 * float(np.median(m)), 2), "spread": round(1000 * (max(m) - min(m)), 2)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
