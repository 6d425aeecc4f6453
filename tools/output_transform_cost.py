"""What the colour transform of the RGB formats costs (vvr_set_output_transform): k_output_rgb over one 3840x2160 10-bit picture as rgbf16 into a
contiguous (3, h, w) device tensor, plain and under the PQ / BT.2020 -> sRGB preset in turn in one process, --repeats launches of each behind
three rounds of warm-up; the kernel time is the library's (HIP events around the launch, vvr_enable_stats / vvr_get_stats).  Median, minimum and
maximum of both, and of the three torch passes over a 4:4:4 frame the stage replaces (table gather, 3x3 matmul, table gather; float32, no
interpolation in the last one: the cheapest form of them), timed with torch's events in the same process.
--root DIR: import vvdec_amd from another checkout - the parent commit's, which gives the yardstick of the plain request (a library without
vvr_set_output_transform reports the plain request only).
Usage: python tools/output_transform_cost.py [--repeats 30] [--root DIR] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v, digits=4):
    return {"median": round(float(np.median(v)), digits), "min": round(float(min(v)), digits), "max": round(float(max(v)), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import vvdec_amd
    W, H = 3840, 2160
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=1, num_streams=1)
    rng = np.random.default_rng(7)
    # (a picture with structure, not noise: neighbouring samples of video are close, which is what the table gathers in LDS meet)
    yy, xx = np.mgrid[0:H, 0:W]
    luma = (512 + 380 * np.sin(xx / 97.) * np.cos(yy / 61.) + rng.integers(-12, 13, (H, W))).clip(0, 1023).astype(np.uint16)
    planes = [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16),
              (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (H // 2, W // 2))).clip(0, 1023).astype(np.uint16)]
    noise = [rng.integers(0, 1024, (H >> s, W >> s), dtype=np.uint16) for s in (0, 1, 1)]
    rec.set_output_colour(9, False)
    rec.enable_stats()
    has = hasattr(rec, "set_output_transform")
    preset = vvdec_amd.output_transform(16, 9, "srgb", 1000., 100., 10) if has else None
    into = torch.empty((3, H, W), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def kernel_ms():
        return {s["name"]: s["total_ms"] for s in rec.stats()}.get("k_output_rgb", 0.)

    res = {"size": [W, H], "bit_depth": 10, "format": "rgbf16", "repeats": a.repeats, "library": vvdec_amd.lib().vvr_version().decode(), "root": a.root}
    for content, pic in (("structured", planes), ("noise", noise)):
        rec.write_picture(0, pic)
        times = {"plain": [], "pq_preset": []}
        for n in range(3 + a.repeats):
            for way in ("plain", "pq_preset") if has else ("plain",):
                if has:
                    rec.set_output_transform(preset if way == "pq_preset" else None)
                k0 = kernel_ms()
                rec.output_wait(rec.output_submit(0, fmt="rgbf16", into=into))
                if n >= 3:
                    times[way].append(kernel_ms() - k0)
        res[content] = {"k_output_rgb_%s_ms" % way: spread(v) for way, v in times.items() if v}
    if has:
        # the three passes a consumer runs without the stage, over the rgb16 frame the plain request would have written
        rec.set_output_transform(None)
        frame = torch.empty((3, H, W), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        rec.output_wait(rec.output_submit(0, fmt="rgb16", into=frame))
        lin, m, enc = [torch.from_numpy(t.astype(np.float32)).cuda() for t in vvdec_amd.abi.output_transform_arrays(preset)]
        m = m / 16384
        idx = frame.long()
        torch.cuda.synchronize()
        passes = []
        for n in range(3 + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L = lin[idx]
            T = torch.matmul(m, L.view(3, -1)).clamp_(0, 65535)
            E = (enc[(T.long() >> 6)] * (1 / 65535)).half()
            e1.record()
            e1.synchronize()
            if n >= 3:
                passes.append(e0.elapsed_time(e1))
        res["torch_gather_matmul_gather_ms"] = spread(passes)
    rec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
