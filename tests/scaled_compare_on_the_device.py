"""GPU helper of tests/test_gpu_output_scaled_compare.py (run as a script; prints "ok tensors" when the case passes:
Reconstructor.set_compare_scaling, then compare / ssim / msssim / xpsnr with torch tensors of the scaled size as the reference, and with
numpy planes).  A process of its own because the reference planes are torch tensors: torch brings its own HIP runtime, which has to be the
first one the process initialises (as tests/semiplanar_on_the_device.py explains)."""
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
import ssim_ref                   # noqa: E402
import xpsnr_ref                  # noqa: E402
import test_output_compare_host as XC             # noqa: E402
import test_output_msssim_host as XM              # noqa: E402
import test_output_scaled_compare_host as S       # noqa: E402
import test_output_ssim_host as XS                # noqa: E402
import test_output_xpsnr_host as XX               # noqa: E402


def on_device(planes, shift):
    out = []
    for p in planes:
        t = torch.zeros((p.shape[0], p.shape[1] + 8 + shift), dtype=torch.int16, device="cuda")
        t[:, shift:shift + p.shape[1]] = torch.from_numpy(p.astype(np.uint16).view(np.int16)).cuda()
        out.append(t[:, shift:shift + p.shape[1]])
    torch.cuda.synchronize()
    return out


def tensors_as_the_reference():
    bd = 10
    rec = vvdec_amd.Reconstructor(S.W, S.H_, bit_depth=bd, num_slots=2, num_streams=1)
    rng = np.random.default_rng(2200)
    planes = SUP.random_planes(rng, S.W, S.H_, bd, 1)
    rec.write_picture(0, planes)
    for name, win, size in (S.LADDER, S.UNEVEN):
        rec.set_compare_scaling(size)
        part = rec.read_output(0, win, 2, size=size, collocated=(True, False))
        swin = S.as_window(size)
        ref = [rng.integers(0, 1 << bd, p.shape, dtype=np.int64) for p in part]
        prev = [rng.integers(0, 1 << bd, part[0].shape, dtype=np.int64)]
        for shift in (0, 1):          # planes that start at an even and at an odd column: the wide and the sample-by-sample class
            tensors, tprev = on_device(ref, shift), on_device(prev, shift)
            what = "%s, tensors from column %d" % (name, shift)
            got = rec.compare(0, tensors, window=win, with_map=True)
            XC.same((got["raw"], got["map"]), compare_ref.compare(part, ref), swin, bd, "compare, " + what)
            got = rec.ssim(0, tensors, window=win, with_map=True)
            XS.same((got["raw"], got["map"]), ssim_ref.ssim(part, ref, bd), swin, bd, "ssim, " + what)
            got = rec.msssim(0, tensors, window=win, scales=2)
            XM.same(got["raw"], msssim_ref.msssim(part, ref, bd, 2), swin, bd, "msssim, " + what)
            got = rec.xpsnr(0, tensors, tprev, window=win, block=8, with_blocks=True)
            XX.same((got["raw"], got["blocks"].reshape(-1)), xpsnr_ref.xpsnr_integers(part, ref, prev, 8, 0), swin, bd, "xpsnr, " + what)
        # numpy planes of the scaled size; planes of the window's size are refused by the wrapper, and so is a slot by the library
        got = rec.compare(0, [p.astype(np.uint16) for p in ref], window=win, with_map=True)
        XC.same((got["raw"], got["map"]), compare_ref.compare(part, ref), swin, bd, name + ", numpy planes")
        try:
            rec.compare(0, [np.zeros((win[3] >> s, win[2] >> s), np.uint16) for s in (0, 1, 1)], window=win)
            raise AssertionError("planes of the window's size were accepted")
        except ValueError:
            pass
        try:
            rec.compare(0, 1, window=win)
            raise AssertionError("a slot as the reference was accepted under scaling")
        except vvdec_amd.VvrError as e:
            assert "ref_slot" in str(e), e
    # off again: the window's size
    rec.set_compare_scaling(None)
    win = (0, 0, S.W, S.H_)
    got = rec.compare(0, [p ^ 1 for p in planes], window=win, with_map=True)
    XC.same((got["raw"], got["map"]), compare_ref.compare(planes, [p ^ 1 for p in planes]), win, bd, "scaling off again")
    rec.close()


if __name__ == "__main__":
    try:
        tensors_as_the_reference()
    except BaseException:
        traceback.print_exc()
        print("FAILED tensors", flush=True)
        sys.exit(1)
    print("ok tensors", flush=True)
