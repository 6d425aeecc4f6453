"""GPU helper of tests/test_gpu_output_compare.py (run as a script; prints "ok tensors" when the case passes: Reconstructor.compare with
torch tensors, numpy planes and a slot as the reference).  A process of its own because the
reference planes are torch tensors: torch brings its own HIP runtime, which has to be the first one the process initialises (as
tests/semiplanar_on_the_device.py explains)."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import output_support as SUP        # noqa: E402
import compare_ref                # noqa: E402
import test_output_compare_host as X              # noqa: E402


def tensors_as_the_reference():
    rec = vvdec_amd.Reconstructor(X.W, X.H_, bit_depth=10, num_slots=2, num_streams=1)
    rng = np.random.default_rng(1280)
    planes = SUP.random_planes(rng, X.W, X.H_, 10, 1)
    rec.write_picture(0, planes)
    rec.enable_stats()
    runs = 0
    for win in X.WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps, dt, tdt in ((2, np.int16, torch.int16), (1, np.uint8, torch.uint8)):
            ref = X.reference("random", rng, part, 10, bps)
            want = compare_ref.compare(part, ref)
            for shift in (0, 1):
                tensors = []
                for p in ref:
                    t = torch.zeros((p.shape[0], p.shape[1] + 8 + shift), dtype=tdt, device="cuda")
                    t[:, shift:shift + p.shape[1]] = torch.from_numpy(p.astype(np.uint16 if bps == 2 else np.uint8).view(dt)).cuda()
                    tensors.append(t[:, shift:shift + p.shape[1]])
                torch.cuda.synchronize()
                got = rec.compare(0, tensors, window=win, with_map=True)
                runs += 1
                what = "tensors, window %r, %d bytes per sample, column %d" % (win, bps, shift)
                X.same((got["raw"], got["map"]), want, win, 10, what)
                assert got["differing"] == want["differing"] and got["sse"] == want["sse"]
                assert got["first"] == [(x, y) if n else None for x, y, n in zip(want["first_x"], want["first_y"], want["differing"])]
                for g, w_ in zip(rec.psnr(got), compare_ref.psnr(want, 10)):
                    assert g == w_ or abs(g - w_) <= 1e-9
    # the other forms Reconstructor.compare takes: numpy planes (uint16 and uint8, copied during the call) and a slot
    win = X.WINDOWS[1]
    part = compare_ref.window_planes(planes, win)
    for bps, dt in ((2, np.uint16), (1, np.uint8)):
        ref = X.reference("random", rng, part, 10, bps)
        got = rec.compare(0, [p.astype(dt) for p in ref], window=win, with_map=True)
        runs += 1
        X.same((got["raw"], got["map"]), compare_ref.compare(part, ref), win, 10, "numpy planes, %d bytes per sample" % bps)
    other = [p ^ 1 for p in planes]
    rec.write_picture(1, other)
    got = rec.compare(0, 1, with_map=True)
    runs += 1
    X.same((got["raw"], got["map"]), compare_ref.compare(planes, other), (0, 0, X.W, X.H_), 10, "slot 1 as the reference")
    assert got["differing"] == [X.W * X.H_, X.W * X.H_ // 4, X.W * X.H_ // 4] and got["first"] == [(0, 0)] * 3 and rec.psnr(got)[3] < 70
    st = {s["name"]: s["launches"] for s in rec.stats()}
    assert st == {"k_output_compare": runs, "k_output_compare_sum": runs}, st
    rec.close()


if __name__ == "__main__":
    try:
        tensors_as_the_reference()
    except BaseException:
        traceback.print_exc()
        print("FAILED tensors", flush=True)
        sys.exit(1)
    print("ok tensors", flush=True)
