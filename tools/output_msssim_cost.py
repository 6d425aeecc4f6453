"""What an MS-SSIM request of the output queue costs (vvr_msssim_submit): on the 3840x2160 window of one 10-bit picture, at 5 scales, the device
time of the block launches (k_output_msssim, one per scale, timed together) and of the fold (k_output_msssim_sum) with the reference in device
memory (torch tensors, read in place; 16-bit planes) and in another slot - next to the SSIM request of the same frame in the same process
(k_output_ssim: the yardstick).  Per level: requests of 1 .. 5 scales of the same frame take turns with the others, and what is reported for
level k is the request of k + 1 scales less the request of k scales - the launch of level k and, with it, the next level's stores that level
k - 1 now makes.  The levels so attributed sum to the 5-scale request's time.
The configurations take turns inside a round (--repeats requests of each behind three of warm-up); the process runs --rounds rounds and reports,
per configuration, the median of every round, the median of those medians and their spread.  The kernel time is the library's (HIP events around
the launches, vvr_enable_stats / vvr_get_stats); the wall time is vvr_msssim_submit .. vvr_output_wait on the host.
--table FILE: the compiler's resource table (tools/kernel_resources.sh); the lines of the kernels measured here are quoted in the note.
--table-only: no GPU: the note holds the compiler's table and says that the times are NOT YET measured.
Usage: python tools/output_msssim_cost.py [--repeats 30] [--rounds 5] [--table FILE] [--table-only] [--out profiles/output_msssim_4k.txt] [--json FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from output_cost_common import W, H, picture, noisy, summary, timed, take_turns, main      # noqa: E402

KERNELS = ("k_output_msssim", "k_output_msssim_sum", "k_output_ssim", "k_output_ssim_sum")
YARDSTICK = "SSIM request of the same frame (k_output_ssim), reference in device memory, 16-bit"
SCALES = 5


def measure(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    rng = np.random.default_rng(7)
    planes = picture(rng)
    # the reference: the picture with coding-noise-like differences in a quarter of the samples
    other = [noisy(rng, p) for p in planes]
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=2, num_streams=1)
    rec.write_picture(0, planes)
    rec.write_picture(1, other)
    ceiling = rec.copy_bandwidth(20)
    rec.enable_stats()
    dev16 = [torch.from_numpy(p.view(np.int16)).cuda() for p in other]
    torch.cuda.synchronize()
    # (name, reference, scales; 0: the SSIM request)
    configs = [("reference in device memory, 16-bit", dev16, SCALES), ("reference in another slot", 1, SCALES), (YARDSTICK, dev16, 0)]
    configs += [("%d scale%s, reference in device memory, 16-bit" % (n, "s" if n > 1 else ""), dev16, n) for n in range(1, SCALES)]

    def request(config):
        name, ref, scales = config
        if scales:
            return timed(rec, KERNELS, lambda: rec.msssim(0, ref, window=(0, 0, W, H), scales=scales))
        return timed(rec, KERNELS, lambda: rec.ssim(0, ref, window=(0, 0, W, H)))

    medians = take_turns(configs, a.rounds, a.repeats, request)
    first = rec.msssim(0, dev16, window=(0, 0, W, H), scales=SCALES)
    rec.close()
    res = {"size": [W, H], "bit_depth": 10, "scales": SCALES, "repeats": a.repeats, "rounds": a.rounds, "library": vvdec_amd.lib().vvr_version().decode(),
           "copy_bandwidth_GBps": round(ceiling / 1e9, 1), "msssim": [round(v, 6) for v in first["msssim"]], "windows": first["windows"], "configs": {}}
    for name, ref, scales in configs:
        m = np.array(medians[name]) * 1000      # microseconds
        main, fold = (m[:, 0], m[:, 1]) if scales else (m[:, 2], m[:, 3])
        res["configs"][name] = {"scales": scales, "kernel_us": summary(main), "fold_us": summary(fold), "request_wall_us": summary(m[:, 4])}
    return res


def compose(res, table):
    out = ["MS-SSIM of a picture against a reference frame through the output queue (vvr_msssim_submit): the compiler's resource lines of the two kernels",
           "and their time at 5 scales on the 3840x2160 window of one 10-bit 4:2:0 picture (a structured synthetic picture; the reference differs from",
           "it in a quarter of the samples)." + (" Windows per level and component %r, MS-SSIM %r (Y, Cb, Cr, all)." % (res["windows"], res["msssim"]) if res else ""), ""]
    if table:
        out += ["== Compiler table (tools/kernel_resources.sh: hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) =="]
        out += [l.rstrip() for l in open(table) if "k_output_msssim" in l or "k_output_ssim" in l] + [""]
    if not res:
        return "\n".join(out + ["== Kernel time at 4K ==", "NOT YET measured: no run on the device has been made with this library (tools/output_msssim_cost.py writes this section).", ""])
    out += ["== Kernel time at 4K ==",
            "One MI355X, one process (%s).  %d rounds; in a round the configurations take turns, %d timed requests of each behind three of" % (res["library"], res["rounds"], res["repeats"]),
            "warm-up.  Kernel time: HIP events around the launches (vvr_enable_stats) - the k_output_msssim launches of a request together, from before",
            "the first to behind the last, its fold k_output_msssim_sum apart.  Wall time: vvr_msssim_submit .. vvr_output_wait on the host,",
            "registration of the tensors included.  Per configuration the median of the round medians, their spread (largest - smallest) and the",
            "round medians, in microseconds.  vvr_measure_copy_bandwidth of this run: %.1f GB/s (read + written by the library's copy kernel)." % res["copy_bandwidth_GBps"], ""]
    for name, c in res["configs"].items():
        k, f, w_ = c["kernel_us"], c["fold_us"], c["request_wall_us"]
        out += ["-- %s" % name,
                "   kernel%s median %8.2f  spread %6.2f  %r" % ("s" if c["scales"] > 1 else " ", k["median"], k["spread"], k["round_medians"]),
                "   fold    median %8.2f  spread %6.2f  %r" % (f["median"], f["spread"], f["round_medians"]),
                "   request median %8.2f  spread %6.2f  (host wall time)" % (w_["median"], w_["spread"]), ""]
    yard = res["configs"][YARDSTICK]["kernel_us"]["median"]
    by_scales = {c["scales"]: c["kernel_us"]["median"] for name, c in res["configs"].items() if "device memory" in name and c["scales"]}
    out += ["== Per level (reference in device memory, 16-bit): the request of k + 1 scales less the request of k scales =="]
    for k in range(SCALES):
        out += ["level %d: %7.2f us" % (k, by_scales[k + 1] - by_scales.get(k, 0.))]
    out += ["sum:     %7.2f us (the request of %d scales)" % (by_scales[SCALES], SCALES), "", "== Against k_output_ssim =="]
    for name, c in res["configs"].items():
        if c["scales"] == SCALES:
            out += ["k_output_msssim x %d, %s: %.2f us = %.2f x k_output_ssim (%.2f us in this process); folds %.2f us against %.2f us" %
                    (SCALES, name, c["kernel_us"]["median"], c["kernel_us"]["median"] / yard, yard, c["fold_us"]["median"], res["configs"][YARDSTICK]["fold_us"]["median"])]
    out += ["k_output_msssim, 1 scale (no next level is written): %.2f us = %.2f x k_output_ssim" % (by_scales[1], by_scales[1] / yard)]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main(measure, compose)
