"""What the cost tools of the measures of the output queue share (tools/output_compare_cost.py, output_ssim_cost.py, output_msssim_cost.py,
output_xpsnr_cost.py, output_scaled_cost.py): the synthetic 4K picture and its noisy copy, the rounds in which the configurations take turns,
the reduction of the rounds, and the command line.  Each tool keeps its configurations, its prose and its compose()."""
import argparse
import json
import time

import numpy as np

W, H = 3840, 2160


def picture(rng, w=W, h=H):
    """a structured synthetic 10-bit 4:2:0 picture of w x h: the 4K picture's content at that size"""
    yy, xx = np.mgrid[0:h, 0:w]
    luma = (512 + 380 * np.sin(xx * (W / w) / 97.) * np.cos(yy * (H / h) / 61.) + rng.integers(-12, 13, (h, w))).clip(0, 1023).astype(np.uint16)
    return [luma, (512 + (luma[::2, ::2].astype(np.int64) - 512) // 3 + rng.integers(-6, 7, (h // 2, w // 2))).clip(0, 1023).astype(np.uint16),
            (512 - (luma[::2, ::2].astype(np.int64) - 512) // 4 + rng.integers(-6, 7, (h // 2, w // 2))).clip(0, 1023).astype(np.uint16)]


def noisy(rng, p):
    """the plane with coding-noise-like differences in a quarter of the samples"""
    return np.where(rng.random(p.shape) < 0.25, (p.astype(np.int64) + rng.integers(-3, 4, p.shape)).clip(0, 1023), p).astype(np.uint16)


def summary(v):
    return {"round_medians": [round(float(x), 2) for x in v], "median": round(float(np.median(v)), 2), "spread": round(float(np.max(v) - np.min(v)), 2)}


def timed(rec, kernels, call):
    """one request: the milliseconds the library counted for each of `kernels` (vvr_enable_stats) during call(), then its wall time in ms"""
    def kernel_ms():
        st = {s["name"]: s["total_ms"] for s in rec.stats()}
        return [st.get(k, 0.) for k in kernels]
    k0, t0 = kernel_ms(), time.perf_counter()
    call()
    wall = time.perf_counter() - t0
    return [y - x for x, y in zip(k0, kernel_ms())] + [wall * 1000]


def take_turns(configs, rounds, repeats, run, each_round=None):
    """`rounds` rounds; in a round the configurations (tuples whose first element is the name) take turns, `repeats` timed requests of each behind
    three of warm-up; run( config ) makes one request and returns its numbers -> {name: the median of the numbers, per round};
    each_round( {name: the numbers of every timed request} ) sees a round's requests"""
    medians = {c[0]: [] for c in configs}
    for _ in range(rounds):
        times = {c[0]: [] for c in configs}
        for k in range(3 + repeats):
            for c in configs:
                numbers = run(c)
                if k >= 3:
                    times[c[0]].append(numbers)
        for c in configs:
            medians[c[0]].append([float(v) for v in np.median(np.array(times[c[0]]), axis=0)])
        if each_round:
            each_round(times)
    return medians


def main(measure, compose, table_only=True):
    """the command line: measure( args ) -> the result (a dict, written to --json), compose( result or None, table file ) -> the note, printed and
    written to --out; table_only: the tool has --table-only, which composes the note without a measurement"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--table", default="")
    if table_only:
        ap.add_argument("--table-only", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    res = None if table_only and a.table_only else measure(a)
    if res is not None and a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    text = compose(res, a.table)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
