"""GPU helper of tests/test_gpu_output_resample.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and
stops at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which
has to be the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: a window of a frame resampled into a (3, 20, 48) float32 tensor on the device, normalised, under every filter ("tensor"); the
formats behind the resampler of tests/test_output_resample_host.py with torch tensors inside a guard region as the device destinations
("formats-<bit depth>"); the statistics entries ("stats").  Everything is compared with tests/resample_ref.py, exactly."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import interleaved_ref                            # noqa: E402
import resample_ref as R                          # noqa: E402
import test_film_grain_host as H                  # noqa: E402
import test_output_resample_host as N             # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
import yuv_on_the_device as YD                    # noqa: E402
from vvdec_amd import abi                         # noqa: E402

YD.TORCH_DT.setdefault(np.float32, torch.float32)


def _rec(bd):
    rec = vvdec_amd.Reconstructor(N.W, N.H_, bit_depth=bd, chroma_format=1, num_slots=2, num_streams=1)
    return rec


def a_window_into_a_float32_tensor():
    """a model's input: (2, 2, 204, 76) of a 10-bit frame -> (3, 20, 48) float32 on the device, BT.709, normalised, under every filter and
    through Reconstructor.set_output_resampling's names; exact against the restatement fed to interleaved_ref"""
    bd, win, size, col = 10, (2, 2, 204, 76), (48, 20), (True, False)
    rec = _rec(bd)
    picture = N.content("noise", N.W, N.H_, bd, 3, 90)
    rec.write_picture(0, picture)
    rec.set_output_colour(1, False)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    rec.set_output_normalisation(*norm)
    for name in ("area", "triangle", "cubic"):
        rec.set_output_resampling(name)
        into = torch.full((3, 20, 48), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()       # (idle before the request: the fill runs on torch's stream)
        got = rec.output_wait(rec.output_submit(0, window=win, fmt="rgbf32", size=size, collocated=col, into=into))
        assert got is into
        want = interleaved_ref.frame(R.resample(S.crop(picture, win), R.FILTERS[name], size, bd, col), bd, "rgbf32", 1, False, col, None, norm)
        N.same(list(into.cpu().numpy()), want, "rgbf32 tensor under %s" % name)
    for bad in ("lanczos", 4, -1):
        try:
            rec.set_output_resampling(bad)
        except (vvdec_amd.VvrError, ValueError):
            pass
        else:
            assert False, bad
    rec.set_output_resampling(None)
    try:
        rec.output_submit(0, window=(0, 0, 208, 80), fmt="planar16", size=(4, 2))
    except vvdec_amd.VvrError as e:
        assert "within 1/8 .. 8 times" in str(e)
    else:
        assert False, "accepted below 1/8 with no filter set"
    assert vvdec_amd.resample_taps("cubic", 208, 56, 2, 3) == (R.taps(R.CUBIC, 208, 56, 2, 3)[0], list(R.taps(R.CUBIC, 208, 56, 2, 3)[1]))
    rec.close()


def formats_on_the_device(bd):
    rec = _rec(bd)
    bank = abi.film_grain_bank(**H._bank(np.random.default_rng(520 + bd)))
    N.check_formats(rec.L, rec.ctx, lambda ctx, slot, p: rec.write_picture(slot, p), bd, bank, device=YD._into_tensors(rec, []))
    rec.close()


def statistics_name_the_kernel():
    """a request under a filter: k_output_resample with one launch per component, its algorithmic bytes, and no k_rescale; the format kernel
    behind it as ever"""
    rec = _rec(10)
    rec.write_picture(0, N.content("noise", N.W, N.H_, 10, 3, 91))
    rec.enable_stats()
    rec.set_output_resampling("cubic")
    win, size = N.GEOMETRIES[0]
    rec.output_wait(rec.output_submit(0, window=win, fmt="p010", size=size))
    rec.output_wait(rec.output_submit(0, window=win, fmt="planar16", size=size))
    stats = {s["name"]: s for s in rec.stats()}
    assert stats["k_output_resample"]["launches"] == 6 and "k_rescale" not in stats and stats["k_output_frame"]["launches"] == 1, stats
    assert stats["k_output_resample"]["algo_bytes"] == 2 * (208 * 80 + 56 * 24) * 2 * 3 // 2, stats
    rec.set_output_resampling(None)
    rec.output_wait(rec.output_submit(0, window=win, fmt="planar16", size=size))
    assert {s["name"]: s for s in rec.stats()}["k_output_resample"]["launches"] == 6
    rec.close()


def main(names):
    for name in names:
        try:
            if name.startswith("formats-"):
                formats_on_the_device(int(name.split("-")[1]))
            else:
                {"tensor": a_window_into_a_float32_tensor, "stats": statistics_name_the_kernel}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
