"""GPU helper of tests/test_gpu_output_ssim.py (run as a script; prints "ok tensors" when the case passes: Reconstructor.ssim with torch
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
import ssim_ref                   # noqa: E402
import test_output_ssim_host as X                 # noqa: E402


def agrees(got, want, win, what):
    X.same((got["raw"], got["map"]), want, win, 10, what)
    assert got["sum"] == want["sum"] and got["windows"] == want["windows"] and got["min"] == want["min"] and got["ssim"] == ssim_ref.mean(want), what
    assert got["min_at"] == [(x, y) if n else None for x, y, n in zip(want["min_x"], want["min_y"], want["windows"])], what


def tensors_as_the_reference():
    rec = vvdec_amd.Reconstructor(X.W, X.H_, bit_depth=10, num_slots=2, num_streams=1)
    rng = np.random.default_rng(1480)
    planes = SUP.random_planes(rng, X.W, X.H_, 10, 1)
    rec.write_picture(0, planes)
    rec.enable_stats()
    runs = 0
    for win in X.WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps, dt, tdt in ((2, np.int16, torch.int16), (1, np.uint8, torch.uint8)):
            ref = X.reference("noise", rng, part, 10) if bps == 2 else [rng.integers(0, 256, p.shape, dtype=np.int64) for p in part]
            want = ssim_ref.ssim(part, ref, 10)
            for shift in (0, 1):
                tensors = []
                for p in ref:
                    t = torch.zeros((p.shape[0], p.shape[1] + 8 + shift), dtype=tdt, device="cuda")
                    t[:, shift:shift + p.shape[1]] = torch.from_numpy(p.astype(np.uint16 if bps == 2 else np.uint8).view(dt)).cuda()
                    tensors.append(t[:, shift:shift + p.shape[1]])
                torch.cuda.synchronize()
                got = rec.ssim(0, tensors, window=win, with_map=True)
                runs += 1
                agrees(got, want, win, "tensors, window %r, %d bytes per sample, column %d" % (win, bps, shift))
    # the other forms Reconstructor.ssim takes: numpy planes (uint16 and uint8, copied during the call) and a slot
    win = X.WINDOWS[1]
    part = compare_ref.window_planes(planes, win)
    for bps, dt in ((2, np.uint16), (1, np.uint8)):
        ref = X.reference("noise", rng, part, 10) if bps == 2 else [rng.integers(0, 256, p.shape, dtype=np.int64) for p in part]
        got = rec.ssim(0, [p.astype(dt) for p in ref], window=win, with_map=True)
        runs += 1
        agrees(got, ssim_ref.ssim(part, ref, 10), win, "numpy planes, %d bytes per sample" % bps)
    other = SUP.noisy(planes, 10, 1481)
    rec.write_picture(1, other)
    got = rec.ssim(0, 1, with_map=True)
    runs += 1
    agrees(got, ssim_ref.ssim(planes, other, 10), (0, 0, X.W, X.H_), "slot 1 as the reference")
    assert got["windows"] == [51 * 19, 25 * 9, 25 * 9] and all(0 < v < 1 for v in got["ssim"])
    got = rec.ssim(0, 0 + 1, window=(6, 2, 8, 8))
    runs += 1
    assert got["windows"] == [1, 0, 0] and got["min_at"] == [(0, 0), None, None] and "map" not in got and got["ssim"][1] == 0.
    st = {s["name"]: s["launches"] for s in rec.stats()}
    assert st == {"k_output_ssim": runs, "k_output_ssim_sum": runs}, st
    rec.close()


if __name__ == "__main__":
    try:
        tensors_as_the_reference()
    except BaseException:
        traceback.print_exc()
        print("FAILED tensors", flush=True)
        sys.exit(1)
    print("ok tensors", flush=True)
