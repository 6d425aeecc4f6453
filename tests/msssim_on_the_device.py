"""GPU helper of tests/test_gpu_output_msssim.py (run as a script; prints "ok tensors" when the case passes: Reconstructor.msssim with torch
tensors, numpy planes and a slot as the reference).  A process of its own because the reference planes are torch tensors: torch brings its
own HIP runtime, which has to be the first one the process initialises (as tests/compare_on_the_device.py explains)."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import output_support as SUP        # noqa: E402
import compare_ref                # noqa: E402
import msssim_ref                 # noqa: E402
import test_output_msssim_host as X               # noqa: E402


def agrees(got, want, win, what, weights=None):
    X.same(got["raw"], want, win, 10, what)
    n = want["scales"]
    assert got["scales"] == n and got["sum_cs"] == want["sum_cs"][:n] and got["sum_v"] == want["sum_v"][:n] and got["windows"] == want["windows"][:n], what
    assert got["width"] == want["width"][:n] and got["height"] == want["height"][:n] and X.close(got["msssim"], msssim_ref.value(want, weights)), what


def tensors_as_the_reference():
    rec = vvdec_amd.Reconstructor(X.W, X.H_, bit_depth=10, num_slots=2, num_streams=1)
    rng = np.random.default_rng(1580)
    planes = SUP.random_planes(rng, X.W, X.H_, 10, 1)
    rec.write_picture(0, planes)
    rec.enable_stats()
    launches = runs = 0
    for win, scales in X.CASES:
        part = compare_ref.window_planes(planes, win)
        for bps, dt, tdt in ((2, np.int16, torch.int16), (1, np.uint8, torch.uint8)):
            ref = X.reference("noise", rng, part, 10, scales) if bps == 2 else [rng.integers(0, 256, p.shape, dtype=np.int64) for p in part]
            want = msssim_ref.msssim(part, ref, 10, scales)
            for shift in (0, 1):
                tensors = []
                for p in ref:
                    t = torch.zeros((p.shape[0], p.shape[1] + 8 + shift), dtype=tdt, device="cuda")
                    t[:, shift:shift + p.shape[1]] = torch.from_numpy(p.astype(np.uint16 if bps == 2 else np.uint8).view(dt)).cuda()
                    tensors.append(t[:, shift:shift + p.shape[1]])
                torch.cuda.synchronize()
                got = rec.msssim(0, tensors, window=win, scales=scales)
                runs, launches = runs + 1, launches + scales
                agrees(got, want, win, "tensors, window %r, %d bytes per sample, column %d" % (win, bps, shift))
    # the other forms Reconstructor.msssim takes: numpy planes (uint16 and uint8, copied during the call) and a slot; a caller's weights
    win, scales = X.CASES[1]
    part = compare_ref.window_planes(planes, win)
    for bps, dt in ((2, np.uint16), (1, np.uint8)):
        ref = X.reference("noise", rng, part, 10, scales) if bps == 2 else [rng.integers(0, 256, p.shape, dtype=np.int64) for p in part]
        got = rec.msssim(0, [p.astype(dt) for p in ref], window=win, scales=scales)
        runs, launches = runs + 1, launches + scales
        agrees(got, msssim_ref.msssim(part, ref, 10, scales), win, "numpy planes, %d bytes per sample" % bps)
    other = SUP.noisy(planes, 10, 1581)
    rec.write_picture(1, other)
    mine = [0.1, 0.2, 0.3, 0.25, 0.15]
    got = rec.msssim(0, 1, weights=mine)
    runs, launches = runs + 1, launches + 5
    agrees(got, msssim_ref.msssim(planes, other, 10, 5), (0, 0, X.W, X.H_), "slot 1 as the reference", mine)
    assert got["windows"][4] == [3 * 3, 1, 1] and all(0 < v < 1 for v in got["msssim"])
    got = rec.msssim(0, 0 + 1, window=(6, 2, 16, 16), scales=1)
    runs, launches = runs + 1, launches + 1
    assert got["windows"] == [[9, 1, 1]] and got["scales"] == 1
    st = {s["name"]: s["launches"] for s in rec.stats()}
    assert st == {"k_output_msssim": launches, "k_output_msssim_sum": runs}, st
    rec.close()


if __name__ == "__main__":
    try:
        tensors_as_the_reference()
    except BaseException:
        traceback.print_exc()
        print("FAILED tensors", flush=True)
        sys.exit(1)
    print("ok tensors", flush=True)
