"""What an XPSNR request of the output queue costs (vvr_xpsnr_submit): on the 3840x2160 window of one 10-bit picture, filter 2 and B = 128 (what
the request resolves to at that size), the device time of k_output_xpsnr for temporal 0 and 2 with the planes in device memory (torch tensors,
read in place; 16-bit and 8-bit) - next to the comparison request of the same frame in the same process (k_output_compare, which reads the
slot and the reference without the halo, the stencil and the prev planes: the yardstick, scaled by the bytes read).
The configurations take turns inside a round (--repeats requests of each behind three of warm-up); the process runs --rounds rounds and reports,
per configuration, the median of every round, the median of those medians and their spread.  The kernel time is the library's (HIP events around
the launch, vvr_enable_stats / vvr_get_stats; the clearing of the records and their copy back are outside them); the wall time is
vvr_xpsnr_submit .. vvr_output_wait on the host.
--table FILE: the compiler's resource table (tools/kernel_resources.sh); the lines of the kernels measured here are quoted in the note.
--table-only: no GPU: the note holds the compiler's table and says that the times are unmeasured.
Usage: python tools/output_xpsnr_cost.py [--repeats 30] [--rounds 5] [--table FILE] [--table-only] [--out profiles/output_xpsnr_4k.txt] [--json FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from output_cost_common import W, H, picture, noisy, summary, timed, take_turns, main      # noqa: E402

KERNELS = ("k_output_xpsnr", "k_output_compare")
YARDSTICK = "comparison request of the same frame (k_output_compare), reference in device memory, 16-bit"


def measure(a):
    import torch                      # first: its HIP runtime is the one the process initialises
    sys.path.insert(0, ROOT)
    import vvdec_amd
    rng = np.random.default_rng(7)
    planes = picture(rng)
    # the reference ("source"): the picture with coding-noise-like differences in a quarter of the samples; its two predecessors: the same again
    other = [noisy(rng, p) for p in planes]
    before = [noisy(rng, other[0]), noisy(rng, other[0])]
    rec = vvdec_amd.Reconstructor(W, H, bit_depth=10, num_slots=2, num_streams=1)
    rec.write_picture(0, planes)
    ceiling = rec.copy_bandwidth(20)
    rec.enable_stats()
    dev16, prev16 = [torch.from_numpy(p.view(np.int16)).cuda() for p in other], [torch.from_numpy(p.view(np.int16)).cuda() for p in before]
    dev8, prev8 = [torch.from_numpy((p >> 2).astype(np.uint8)).cuda() for p in other], [torch.from_numpy((p >> 2).astype(np.uint8)).cuda() for p in before]
    torch.cuda.synchronize()
    luma, samples = W * H, W * H * 3 // 2
    configs = [("temporal 0, planes in device memory, 16-bit", dev16, [], samples * 4),
               ("temporal 2, planes in device memory, 16-bit", dev16, prev16, samples * 4 + 2 * luma * 2),
               ("temporal 0, planes in device memory, 8-bit", dev8, [], samples * 3),
               ("temporal 2, planes in device memory, 8-bit", dev8, prev8, samples * 3 + 2 * luma),
               (YARDSTICK, dev16, None, samples * 4)]

    def request(config):
        name, ref, prev, _b = config
        if prev is None:
            return timed(rec, KERNELS, lambda: rec.compare(0, ref, window=(0, 0, W, H), with_map=True))
        return timed(rec, KERNELS, lambda: rec.xpsnr(0, ref, prev, window=(0, 0, W, H)))

    medians = take_turns(configs, a.rounds, a.repeats, request)
    first = rec.xpsnr(0, dev16, prev16, window=(0, 0, W, H))
    rec.close()
    res = {"size": [W, H], "bit_depth": 10, "repeats": a.repeats, "rounds": a.rounds, "library": vvdec_amd.lib().vvr_version().decode(),
           "copy_bandwidth_GBps": round(ceiling / 1e9, 1), "xpsnr": [round(v, 4) for v in first["xpsnr"]], "block": first["block"], "filter": first["filter"],
           "blocks": [first["blocks_x"], first["blocks_y"]], "configs": {}}
    for name, ref, prev, nbytes in configs:
        m = np.array(medians[name]) * 1000      # microseconds
        main = m[:, 1] if prev is None else m[:, 0]
        res["configs"][name] = {"kernel_us": summary(main), "request_wall_us": summary(m[:, 2]), "bytes_read": nbytes,
                                "read_GBps": round(nbytes / (float(np.median(main)) * 1e-6) / 1e9, 1)}
    return res


def compose(res, table):
    out = ["XPSNR of a picture against a reference frame through the output queue (vvr_xpsnr_submit): the compiler's resource lines of the kernel and its",
           "time on the 3840x2160 window of one 10-bit 4:2:0 picture (a structured synthetic picture; the reference differs from it in a quarter of the",
           "samples, each prev plane from the reference likewise)." +
           (" Filter %d, B = %d, %d x %d blocks; XPSNR %r dB (Y, Cb, Cr, all) at temporal 2." % (res["filter"], res["block"], res["blocks"][0], res["blocks"][1], res["xpsnr"]) if res else ""), ""]
    if table:
        out += ["== Compiler table (tools/kernel_resources.sh: hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) =="]
        out += [l.rstrip() for l in open(table) if "k_output_xpsnr" in l or "k_output_compare<" in l] + [""]
    if not res:
        return "\n".join(out + ["== Kernel time at 4K ==", "unmeasured: no run on the device has been made with this library (tools/output_xpsnr_cost.py writes this section).", ""])
    out += ["== Kernel time at 4K ==",
            "One MI355X, one process (%s).  %d rounds; in a round the configurations take turns, %d timed requests of each behind three of" % (res["library"], res["rounds"], res["repeats"]),
            "warm-up.  Kernel time: HIP events around the launch of k_output_xpsnr (vvr_enable_stats); the clearing of the %d records before it and" % (res["blocks"][0] * res["blocks"][1]),
            "their copy to the host behind it are not in it.  Wall time: vvr_xpsnr_submit .. vvr_output_wait on the host, registration of the tensors",
            "included.  Per configuration the median of the round medians, their spread (largest - smallest) and the round medians, in microseconds;",
            "bytes read: the slot's and the reference's samples and `temporal` luma planes, the halo of 2 samples around every tile (13 % more luma",
            "reference, from the cache for the most part) not counted; GB/s: those bytes over the kernel's median.  vvr_measure_copy_bandwidth of this",
            "run: %.1f GB/s (read + written by the library's copy kernel)." % res["copy_bandwidth_GBps"], ""]
    for name, c in res["configs"].items():
        k, w_ = c["kernel_us"], c["request_wall_us"]
        floor = c["bytes_read"] / (res["copy_bandwidth_GBps"] * 1e9) * 1e6
        out += ["-- %s" % name,
                "   kernel  median %8.2f  spread %6.2f  %r" % (k["median"], k["spread"], k["round_medians"]),
                "   request median %8.2f  spread %6.2f  (host wall time)" % (w_["median"], w_["spread"]),
                "   %.1f MB read, %.1f GB/s; the copy ceiling implies %.2f us for these bytes: the kernel takes %.2f times that" % (c["bytes_read"] / 1e6, c["read_GBps"], floor, k["median"] / floor), ""]
    yard = res["configs"][YARDSTICK]
    out += ["== Against k_output_compare, scaled by the bytes read =="]
    for name, c in res["configs"].items():
        if name != YARDSTICK:
            ratio, by = c["kernel_us"]["median"] / yard["kernel_us"]["median"], c["bytes_read"] / yard["bytes_read"]
            out += ["k_output_xpsnr, %s: %.2f us = %.2f x k_output_compare (%.2f us in this process); it reads %.2f x the bytes: %.2f x per byte" %
                    (name, c["kernel_us"]["median"], ratio, yard["kernel_us"]["median"], by, ratio / by)]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main(measure, compose)
