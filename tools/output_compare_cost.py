"""What a comparison request of the output queue costs (vvr_compare_submit): on the 3840x2160 window of one 10-bit picture, the device time of
k_output_compare and k_output_compare_sum with the reference in device memory (torch tensors, read in place), in memory of vvr_host_alloc (copied
to the device on the output stream ahead of the kernel: the copy is outside the kernel's events and shows in the request's wall time), in another
slot, and as 8-bit planes in device memory - next to the luma-mode statistics request of the same frame (k_output_stats reads half the bytes).
The configurations take turns inside a round (--repeats requests of each behind three of warm-up); the process runs --rounds rounds and reports,
per configuration, the median of every round, the median of those medians and their spread.  The kernel time is the library's (HIP events around
the launch, vvr_enable_stats / vvr_get_stats); the wall time is vvr_compare_submit .. vvr_output_wait on the host.  Bytes read per second - the
slot's and the reference's samples over the kernel's time - stand against vvr_measure_copy_bandwidth of the same run (bytes read + written per
second of the library's copy kernel).
--table FILE: the compiler's resource table (tools/kernel_resources.sh); the lines of the kernels measured here are quoted in the note.
Usage: python tools/output_compare_cost.py [--repeats 30] [--rounds 5] [--table FILE] [--out profiles/output_compare_4k.txt] [--json FILE]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from output_cost_common import W, H, picture, noisy, summary, timed, take_turns, main      # noqa: E402

KERNELS = ("k_output_compare", "k_output_compare_sum", "k_output_stats", "k_output_stats_sum")


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
    dev8 = [torch.from_numpy((p >> 2).astype(np.uint8)).cuda() for p in other]
    pin16 = []
    for p in other:
        buf = rec.host_array(p.size, np.uint16).reshape(p.shape)
        buf[...] = p
        pin16.append(buf)
    torch.cuda.synchronize()
    configs = [("reference in device memory, 16-bit", dev16, 4), ("reference in memory of vvr_host_alloc, 16-bit", pin16, 4), ("reference in another slot", 1, 4),
               ("reference in device memory, 8-bit", dev8, 3), ("luma-mode statistics of the same frame (k_output_stats)", None, 2)]
    samples = W * H * 3 // 2

    def request(config):
        name, ref, _b = config
        if ref is None:
            return timed(rec, KERNELS, lambda: rec.stats_wait(rec.stats_submit(0, window=(0, 0, W, H), mode="luma")))
        return timed(rec, KERNELS, lambda: rec.compare(0, ref, window=(0, 0, W, H), with_map=True))

    medians = take_turns(configs, a.rounds, a.repeats, request)
    first = rec.compare(0, dev16, window=(0, 0, W, H))
    rec.close()
    res = {"size": [W, H], "bit_depth": 10, "repeats": a.repeats, "rounds": a.rounds, "library": vvdec_amd.lib().vvr_version().decode(),
           "copy_bandwidth_GBps": round(ceiling / 1e9, 1), "differing": first["differing"], "configs": {}}
    for name, ref, bps in configs:
        m = np.array(medians[name]) * 1000      # microseconds
        main, fold = (m[:, 2], m[:, 3]) if ref is None else (m[:, 0], m[:, 1])
        nbytes = W * H * 2 if ref is None else samples * bps
        res["configs"][name] = {"kernel_us": summary(main), "fold_us": summary(fold), "request_wall_us": summary(m[:, 4]), "bytes_read": nbytes,
                                "read_GBps": round(nbytes / (float(np.median(main)) * 1e-6) / 1e9, 1)}
    return res


def compose(res, table):
    out = ["A picture compared with a reference frame through the output queue (vvr_compare_submit): the compiler's resource lines of the two kernels and",
           "their time on the 3840x2160 window of one 10-bit 4:2:0 picture (a structured synthetic picture; the reference differs from it in a quarter",
           "of the samples: %r differing samples per component)." % (res["differing"],), ""]
    if table:
        out += ["== Compiler table (tools/kernel_resources.sh: hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no GPU needed) =="]
        out += [l.rstrip() for l in open(table) if "k_output_compare" in l or "k_output_stats(" in l] + [""]
    out += ["== Kernel time at 4K ==",
            "One MI355X, one process (%s).  %d rounds; in a round the configurations take turns, %d timed requests of each behind three of" % (res["library"], res["rounds"], res["repeats"]),
            "warm-up.  Kernel time: HIP events around the launch (vvr_enable_stats) - k_output_compare, its fold k_output_compare_sum apart.  Wall time:",
            "vvr_compare_submit .. vvr_output_wait on the host, with the map (8 KB more over PCIe), registration of the tensors included.  Per",
            "configuration the median of the round medians, their spread (largest - smallest) and the round medians, in microseconds; bytes read: the",
            "slot's and the reference's samples; GB/s: those bytes over the kernel's median.  vvr_measure_copy_bandwidth of this run: %.1f GB/s (read +" % res["copy_bandwidth_GBps"],
            "written by the library's copy kernel), i.e. the ceiling for a kernel that only reads is that many bytes per second.", ""]
    for name, c in res["configs"].items():
        k, f, w_ = c["kernel_us"], c["fold_us"], c["request_wall_us"]
        floor = c["bytes_read"] / (res["copy_bandwidth_GBps"] * 1e9) * 1e6
        out += ["-- %s" % name,
                "   kernel  median %8.2f  spread %6.2f  %r" % (k["median"], k["spread"], k["round_medians"]),
                "   fold    median %8.2f  spread %6.2f  %r" % (f["median"], f["spread"], f["round_medians"]),
                "   request median %8.2f  spread %6.2f  (host wall time)" % (w_["median"], w_["spread"]),
                "   %.1f MB read, %.1f GB/s; the copy ceiling implies %.2f us for these bytes: the kernel takes %.2f times that" % (c["bytes_read"] / 1e6, c["read_GBps"], floor, k["median"] / floor), ""]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main(measure, compose, table_only=False)
