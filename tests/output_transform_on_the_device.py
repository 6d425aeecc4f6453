"""GPU helper of tests/test_gpu_output_transform.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and
stops at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has
to be the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases are those of tests/test_output_transform_host.py on the device, each request into host memory and into a (3, h, w) torch tensor inside a
guard region: the identity ("identity-<bit depth>"), random tables at every format and chroma position on windows stored whole and pair by pair,
behind a rescale and behind grain and a rescale ("random-<bit depth>"), the extremes of the 64-bit sum ("extremes-<bit depth>"), two transforms
in flight and the formats that ignore them ("snapshot-<bit depth>"); three pictures of a GOP as rgbf16 under the PQ preset, consumed on the GPU
behind vvr_output_stream_wait without the host waiting for any of them ("gop"); the statistics entry ("stats").  Everything is compared with
tests/colour_transform_ref.py as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import colour_transform_ref as X                  # noqa: E402
import rgb_on_the_device as D                     # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
import test_output_transform_host as TH           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402


def _on(bd, seed, check, **kw):
    rec, picture = D._setup(bd, seed)
    aligned = []
    check(rec.L, rec.ctx, picture, bd, device=D._into_a_tensor(rec, aligned), **kw)
    assert aligned
    rec.close()


def snapshot_and_scope(bd):
    rec, picture = D._setup(bd, 170 + bd)
    TH.check_snapshot_and_scope(rec.L, rec.ctx, picture, bd)
    rec.close()


def a_gop_under_the_pq_preset_consumed_on_the_gpu():
    """three pictures, every picture's rgbf16 output under the PQ / BT.2020 -> sRGB preset requested into its own (3, h, w) tensor the moment the
    picture is submitted; a side stream waits for each request on the device and clones the tensor; the host waits for nothing until the end"""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    plans = plans[:3]
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [995])[0]
    preset = vvdec_amd.output_transform(16, 9, "srgb", 1000., 100., 10)
    tables = abi.output_transform_arrays(preset)
    ref = X.preset(16, 9, X.TO_SRGB, 1000., 100., 10)
    assert all(np.abs(a.astype(np.int64) - b).max() <= 1 for a, b in zip(tables, ref))
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    rec.set_output_colour(9, False)
    rec.set_output_transform(preset)
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for pl in plans:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(pl, Wd, Hd, seed=995, tool_flags=G.TOOLS, **G.GEO)))
        into = torch.empty((3, Hd, Wd), dtype=torch.float16, device="cuda")
        tickets.append(rec.output_submit(pl.slot, job=jobs[-1], fmt="rgbf16", into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append(into.clone())
    side.synchronize()
    for n, c in enumerate(clones):
        w_ = X.rgb(want[n], 10, "rgbf16", 9, False, (True, False), tables)
        got = c.cpu().numpy()
        for k in range(3):
            assert got[k].tobytes() == w_[k].tobytes(), "picture %d plane %d: %d samples differ" % (n, k, int((got[k].view(np.uint16) != w_[k].view(np.uint16)).sum()))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_count_one_launch_per_request():
    """k_output_rgb: one launch per RGB request with a transform or without, also behind k_rescale; nothing else is launched for the transform"""
    import film_grain_ref
    rec = D._rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(180), S.W, S.H_, 10, 1))
    rec.set_output_colour(9, False)
    rec.enable_stats()
    rng = np.random.default_rng(181)
    for fmt, size, transform in [("rgb8", None, True), ("rgb16", None, True), ("rgbf16", None, False), ("planar16", None, True), ("rgb16", (300, 96), True), ("rgb8", None, True)]:
        rec.set_output_transform(X.random_transform(rng) if transform else None)
        rec.output_wait(rec.output_submit(0, window=(8, 4, 200, 64), fmt=fmt, size=size))
    stats = {s["name"]: s["launches"] for s in rec.stats()}
    assert stats.get("k_output_rgb") == 5 and stats.get("k_output_frame") == 1, stats
    rec.close()


def main(names):
    for name in names:
        try:
            kind, _, bd = name.partition("-")
            if kind == "identity":
                _on(int(bd), 160 + int(bd), TH.check_identity)
            elif kind == "random":
                _on(int(bd), 162 + int(bd), TH.check_random_tables)
            elif kind == "extremes":
                _on(int(bd), 164 + int(bd), TH.check_extremes)
            elif kind == "snapshot":
                snapshot_and_scope(int(bd))
            else:
                {"gop": a_gop_under_the_pq_preset_consumed_on_the_gpu, "stats": statistics_count_one_launch_per_request}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
