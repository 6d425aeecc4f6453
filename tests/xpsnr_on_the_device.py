"""GPU helper of tests/test_gpu_output_xpsnr.py (run as a script; prints "ok tensors" when the case passes: Reconstructor.xpsnr with torch
tensors, numpy planes and a slot as the reference).  A process of its own because the planes are torch tensors: torch brings its own HIP
runtime, which has to be the first one the process initialises (as tests/compare_on_the_device.py explains)."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import output_support as SUP        # noqa: E402
import compare_ref                # noqa: E402
import xpsnr_ref                  # noqa: E402
import test_output_xpsnr_host as X                # noqa: E402


def agrees(got, want, win, what):
    X.same((got["raw"], got["blocks"].reshape(-1)), want, win, 10, what)
    assert got["sse"] == want["sse"][:3] and (got["act_spatial"], got["act_temporal"], got["count"]) == (want["act_spatial"], want["act_temporal"], want["count"]), what
    assert (got["block"], got["filter"], got["blocks_x"], got["blocks_y"], got["temporal"]) == (want["block"], want["filter"], want["blocks_x"], want["blocks_y"], want["temporal"]), what
    assert got["blocks"].shape == (want["blocks_y"], want["blocks_x"]), what
    X.close_enough(got["xpsnr"], xpsnr_ref.xpsnr(want, 10), what)


def tensors_as_the_planes():
    rec = vvdec_amd.Reconstructor(X.W, X.H_, bit_depth=10, num_slots=2, num_streams=1)
    rng = np.random.default_rng(1580)
    planes = SUP.random_planes(rng, X.W, X.H_, 10, 1)
    rec.write_picture(0, planes)
    rec.enable_stats()
    runs = 0
    for win in X.WINDOWS:
        part = compare_ref.window_planes(planes, win)
        for bps, dt, tdt in ((2, np.int16, torch.int16), (1, np.uint8, torch.uint8)):
            ref, prev = X.reference("noise", rng, part, 10) if bps == 2 else X.reference("random16", rng, part, 10, 8)
            for shift, block, flt, temporal in ((0, 0, 1, 2), (1, 44, 2, 1), (0, 64, 2, 2), (1, 128, 1, 0)):
                want = xpsnr_ref.xpsnr_integers(part, ref, prev[:temporal], block, flt)
                tensors = []
                for p in ref + prev[:temporal]:
                    t = torch.zeros((p.shape[0], p.shape[1] + 8 + shift), dtype=tdt, device="cuda")
                    t[:, shift:shift + p.shape[1]] = torch.from_numpy(p.astype(np.uint16 if bps == 2 else np.uint8).view(dt)).cuda()
                    tensors.append(t[:, shift:shift + p.shape[1]])
                torch.cuda.synchronize()
                got = rec.xpsnr(0, tensors[:3], tensors[3:], window=win, block=block, filter=flt, with_blocks=True)
                runs += 1
                agrees(got, want, win, "tensors, window %r, %d bytes per sample, column %d, block %d, filter %d, temporal %d" % (win, bps, shift, block, flt, temporal))
    # the other forms Reconstructor.xpsnr takes: numpy planes (uint16 and uint8, copied during the call) and a slot with prev planes on the host
    win = X.WINDOWS[1]
    part = compare_ref.window_planes(planes, win)
    for bps, dt in ((2, np.uint16), (1, np.uint8)):
        ref, prev = X.reference("noise", rng, part, 10) if bps == 2 else X.reference("random16", rng, part, 10, 8)
        got = rec.xpsnr(0, [p.astype(dt) for p in ref], [p.astype(dt) for p in prev], window=win, with_blocks=True)
        runs += 1
        agrees(got, xpsnr_ref.xpsnr_integers(part, ref, prev), win, "numpy planes, %d bytes per sample" % bps)
    other = SUP.noisy(planes, 10, 1581)
    rec.write_picture(1, other)
    prev = [SUP.noisy(planes, 10, 1582)[0]]
    got = rec.xpsnr(0, 1, prev, with_blocks=True, a_pic=1000., peak=1020.)
    runs += 1
    want = xpsnr_ref.xpsnr_integers(planes, other, prev)
    X.same((got["raw"], got["blocks"].reshape(-1)), want, (0, 0, X.W, X.H_), 10, "slot 1 as the reference")
    X.close_enough(got["xpsnr"], xpsnr_ref.xpsnr(want, 10, 1000., 1020.), "a_pic and peak given")
    assert (got["block"], got["blocks_x"], got["blocks_y"], got["temporal"]) == (4, 52, 20, 1) and all(20 < v < 80 for v in got["xpsnr"])
    got = rec.xpsnr(0, 0 + 1, window=(6, 2, 8, 8), filter=2)
    runs += 1
    assert got["count"] == 4 and "blocks" not in got
    st = {s["name"]: s["launches"] for s in rec.stats()}
    assert st == {"k_output_xpsnr": runs}, st
    rec.close()


if __name__ == "__main__":
    try:
        tensors_as_the_planes()
    except BaseException:
        traceback.print_exc()
        print("FAILED tensors", flush=True)
        sys.exit(1)
    print("ok tensors", flush=True)
