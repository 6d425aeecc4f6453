"""What the measures of the output queue cost against a reference of another size (vvr_set_compare_scaling): a 1920x1080 10-bit 4:2:0 picture
rescaled to 3840x2160 and measured against a 16-bit reference of that size in device memory (torch tensors, read in place), in one process:
  1. the scaled comparison - k_output_compare_scaled, which rescales and compares in one pass;
  2. the unfused sequence it replaces - the three k_rescale launches as they are timed inside a scaled SSIM request, plus k_output_compare of an
     unscaled comparison of a 3840x2160 picture in the same context;
  3. scaled SSIM, MS-SSIM (5 scales) and XPSNR requests beside their unscaled 4K times.
The requests take turns inside a round (--repeats of each behind three of warm-up); the process runs --rounds rounds and reports the median of
every round, the median of those medians and their spread.  Kernel time is the library's (HIP events around the launches, vvr_enable_stats /
vvr_get_stats).  The condition the fused kernel has to meet: the median of (1) is not above the median of (2) by more than the spread of (2)'s
round medians.  vvr_measure_copy_bandwidth of the same run is the ceiling the bytes stand against.
--table FILE: the compiler's resource table (tools/kernel_resources.sh); the lines of the kernels measured here are quoted in the note.
Usage: python tools/output_scaled_cost.py [--repeats 30] [--rounds 5] [--table FILE] [--out profiles/output_scaled_4k.txt] [--json FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from output_cost_common import W, H, picture, noisy, summary, timed, take_turns, main      # noqa: E402

PW, PH = 1920, 1080
KERNELS = ("k_output_compare_scaled", "k_rescale", "k_output_compare", "k_output_ssim", "k_output_msssim", "k_output_xpsnr")
FUSED, RESCALE, COMPARE = 0, 1, 2


def measure(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    rng = np.random.default_rng(11)
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=2, num_streams=1)
    rec.write_picture(0, picture(rng))
    rec._check(rec.L.vvr_slot_picture_size(rec.ctx, 1, PW, PH))
    for c, p in enumerate(picture(rng, PW, PH)):
        rec._check(rec.L.vvr_write_plane(rec.ctx, 1, c, p.ctypes.data, p.shape[1]))
    ceiling = rec.copy_bandwidth(20)
    small, full = (0, 0, PW, PH), (0, 0, W, H)
    # the reference: the rescaled picture with coding-noise-like differences in a quarter of the samples
    up = rec.read_output(1, small, 2, size=(W, H))
    other = [noisy(rng, p) for p in up]
    ref = [torch.from_numpy(p.view(np.int16)).cuda() for p in other]
    prev = [torch.from_numpy(np.roll(other[0], 3, 1).view(np.int16)).cuda()]
    torch.cuda.synchronize()
    rec.enable_stats()
    requests = [("comparison", lambda slot, win: rec.compare(slot, ref, window=win, with_map=True)),
                ("SSIM", lambda slot, win: rec.ssim(slot, ref, window=win, with_map=True)),
                ("MS-SSIM, 5 scales", lambda slot, win: rec.msssim(slot, ref, window=win, scales=5)),
                ("XPSNR, temporal 1", lambda slot, win: rec.xpsnr(slot, ref, prev, window=win))]
    configs = [("%s, %s" % (name, how), call, scaled) for name, call in requests for how, scaled in (("1080p rescaled to 4K", True), ("4K picture", False))]

    def request(config):
        name, call, scaled = config
        rec.set_compare_scaling((W, H) if scaled else None)
        return timed(rec, KERNELS, lambda: call(1 if scaled else 0, small if scaled else full))[:-1]

    unfused = []

    def unfused_pairs(times):
        """the unfused sequence, request by request: k_rescale of this turn's scaled SSIM request + k_output_compare of this turn's 4K comparison"""
        pairs = np.array(times["SSIM, 1080p rescaled to 4K"])[:, RESCALE] + np.array(times["comparison, 4K picture"])[:, COMPARE]
        unfused.append(float(np.median(pairs)))

    medians = take_turns(configs, a.rounds, a.repeats, request, unfused_pairs)
    rec.set_compare_scaling((W, H))
    first = rec.compare(1, ref, window=small)
    rec.close()
    res = {"picture": [PW, PH], "size": [W, H], "bit_depth": 10, "repeats": a.repeats, "rounds": a.rounds, "library": vvdec_amd.lib().vvr_version().decode(),
           "copy_bandwidth_GBps": round(ceiling / 1e9, 1), "differing": first["differing"], "configs": {}}
    for name, _c, _s in configs:
        m = np.array(medians[name]) * 1000      # microseconds
        res["configs"][name] = {k: summary(m[:, i]) for i, k in enumerate(KERNELS) if m[:, i].any()}
    fused = res["configs"]["comparison, 1080p rescaled to 4K"]["k_output_compare_scaled"]
    res["fused_us"] = fused
    res["unfused_us"] = summary(np.array(unfused) * 1000)
    res["condition_met"] = bool(fused["median"] <= res["unfused_us"]["median"] + res["unfused_us"]["spread"])
    return res


def compose(res, table):
    out = ["The measures of the output queue against a reference of another size (vvr_set_compare_scaling): a %dx%d 10-bit 4:2:0 picture rescaled to" % tuple(res["picture"]),
           "%dx%d and measured against a 16-bit reference of that size in device memory (a structured synthetic picture; the reference is the" % tuple(res["size"]),
           "rescaled picture with differences in a quarter of the samples: %r differing samples per component)." % (res["differing"],), ""]
    if table:
        out += ["== Compiler table (tools/kernel_resources.sh: hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) =="]
        out += [l.rstrip() for l in open(table) if "k_output_compare_scaled" in l or "k_output_compare_clear" in l or "k_rescale<" in l or "k_output_compare<" in l] + [""]
    f, u = res["fused_us"], res["unfused_us"]
    bytes_fused = (res["picture"][0] * res["picture"][1] + res["size"][0] * res["size"][1]) * 3
    floor = bytes_fused / (res["copy_bandwidth_GBps"] * 1e9) * 1e6
    out += ["== The fused comparison against the sequence it replaces ==",
            "One MI355X, one process (%s).  %d rounds; in a round the eight requests take turns, %d timed requests of each behind three of warm-up." % (res["library"], res["rounds"], res["repeats"]),
            "Kernel time: HIP events around the launches (vvr_enable_stats).  Microseconds: the median of the round medians, their spread (largest -",
            "smallest), the round medians.  vvr_measure_copy_bandwidth of this run: %.1f GB/s (read + written by the library's copy kernel)." % res["copy_bandwidth_GBps"], "",
            "(1) k_output_compare_scaled, the launch that clears its records included",
            "      median %8.2f  spread %6.2f  %r" % (f["median"], f["spread"], f["round_medians"]),
            "      %.1f MB read (the picture and the reference); the copy ceiling implies %.2f us for these bytes: the kernel takes %.2f times that" % (bytes_fused / 1e6, floor, f["median"] / floor),
            "(2) the three k_rescale launches of a scaled SSIM request + k_output_compare of a 4K comparison, summed turn by turn",
            "      median %8.2f  spread %6.2f  %r" % (u["median"], u["spread"], u["round_medians"]),
            "Condition - (1) not above (2) by more than the spread of (2): %s (%.2f against %.2f + %.2f)." % ("met" if res["condition_met"] else "NOT met", f["median"], u["median"], u["spread"]), "",
            "== Every request, scaled beside unscaled =="]
    for name, c in res["configs"].items():
        out += ["-- %s" % name]
        out += ["   %-24s median %8.2f  spread %6.2f  %r" % (k, v["median"], v["spread"], v["round_medians"]) for k, v in c.items()]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main(measure, compose, table_only=False)
