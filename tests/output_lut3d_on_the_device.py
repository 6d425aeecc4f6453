"""GPU helper of tests/test_gpu_output_lut3d.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and stops
at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to be
the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases are those of tests/test_output_lut3d_host.py on the device, each request into host memory and into a (3, h, w) / (h, w, c) / (h, w)
torch tensor inside a guard region: random LUTs of the three sizes under every RGB format and chroma position, with and without a transform ahead,
on windows stored whole and pair by pair, behind a rescale and behind grain and a rescale ("random-<bit depth>"); all nodes 65535, all 0 and
0 / 65535 by parity ("extremes-<bit depth>"); a grey picture, whose fractions tie everywhere ("grey-<bit depth>"); two LUTs of different sizes in
flight, the formats and the synchronous calls that ignore them, NULL ("snapshot-<bit depth>"); three pictures of a GOP as rgba8 under the PQ LUT
preset, consumed on the GPU behind vvr_output_stream_wait without the host waiting for any of them ("gop"); the statistics entry ("stats").
Everything is compared with tests/lut3d_ref.py as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import interleaved_on_the_device as ID            # noqa: E402
import lut3d_ref as U                             # noqa: E402
import rgb_on_the_device as D                     # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_lut3d_host as LH               # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402


def _setup(bd, seed):
    rec, picture = ID._setup(bd, seed)
    return rec, picture


def _into_a_tensor(rec, aligned):
    """the `device` of the host cases: one request into a tensor inside a guard region, compared - (3, h, w) for the planar formats, (h, w, c) or
    (h, w) for the interleaved ones; aligned collects whether the base is a multiple of 32 bytes (then the kernel stores plane 0 itself)"""
    mem = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def device(L, ctx, slot, win, fmt, ncomp, want, what, seed, size, grain, stride_kind, mis, col):
        d = (D if fmt in U.PLANAR else ID).GuardedTensor(mem, win, fmt, size, stride_kind != "row", mis)
        aligned.append((fmt, d.into.data_ptr() % 32 == 0))
        if seed is not None:
            rec.set_film_grain_seed(seed)
        t = rec.output_submit(slot, window=win, fmt=fmt, size=size, collocated=col, grain=grain, into=d.into)
        assert rec.output_wait(t) is d.into
        d.check(want, what)
    return device


def _on(bd, seed, check, **kw):
    rec, picture = _setup(bd, seed)
    aligned = []
    check(rec.L, rec.ctx, picture, bd, device=_into_a_tensor(rec, aligned), **kw)
    assert any(a for _, a in aligned)
    rec.close()


def grey(bd):
    rec, picture = _setup(bd, 784 + bd)
    LH.check_grey(rec.L, rec.ctx, picture, bd, lambda ctx, slot, p: rec.write_picture(slot, p), device=_into_a_tensor(rec, []))
    rec.close()


def snapshot_and_scope(bd):
    rec, picture = _setup(bd, 786 + bd)
    LH.check_snapshot_and_scope(rec.L, rec.ctx, picture, bd)
    rec.close()


def a_gop_under_the_pq_lut_preset_consumed_on_the_gpu():
    """three pictures, every picture's rgba8 output under the 33-point PQ / BT.2020 -> sRGB LUT preset requested into its own (h, w, 4) tensor the
    moment the picture is submitted; a side stream waits for each request on the device and clones the tensor; the host waits for nothing until
    the end"""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    plans = plans[:3]
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [997])[0]
    n, nodes = vvdec_amd.output_lut3d(33, 16, 9, "srgb", 1000., 100.)
    ref = U.preset(33, 16, 9, 0, 1000., 100.)
    assert np.abs(nodes.astype(np.int64) - ref).max() <= 1
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    rec.set_output_colour(9, False)
    rec.set_output_lut3d((n, nodes))
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for pl in plans:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(pl, Wd, Hd, seed=997, tool_flags=G.TOOLS, **G.GEO)))
        into = torch.empty((Hd, Wd, 4), dtype=torch.uint8, device="cuda")
        tickets.append(rec.output_submit(pl.slot, job=jobs[-1], fmt="rgba8", into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append(into.clone())
    side.synchronize()
    for k, c in enumerate(clones):
        w_ = U.frame(want[k], 10, "rgba8", 9, False, (True, False), n, nodes)
        LH.same([c.cpu().numpy().reshape(Hd, Wd * 4)], w_, "picture %d" % k)
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_count_one_launch_per_request():
    """k_output_rgb: one launch per RGB request with a LUT or without, with a transform ahead of it or not, also behind k_rescale; nothing else
    is launched for the LUT"""
    import colour_transform_ref as X
    import film_grain_ref
    rec = D._rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(790), S.W, S.H_, 10, 1))
    rec.set_output_colour(9, False)
    rec.enable_stats()
    rng = np.random.default_rng(791)
    for fmt, size, n, transform in [("rgb8", None, 17, False), ("rgb16", None, 65, True), ("rgbf16", None, 0, False), ("planar16", None, 33, True), ("rgba8", (300, 96), 33, False), ("rgb8", None, 17, False)]:
        rec.set_output_transform(X.random_transform(rng) if transform else None)
        rec.set_output_lut3d((n, U.random_lut(rng, n)) if n else None)
        rec.output_wait(rec.output_submit(0, window=(8, 4, 200, 64), fmt=fmt, size=size))
    stats = {s["name"]: s["launches"] for s in rec.stats()}
    assert stats.get("k_output_rgb") == 5 and stats.get("k_output_frame") == 1, stats
    rec.close()


def main(names):
    for name in names:
        try:
            kind, _, bd = name.partition("-")
            if kind == "random":
                _on(int(bd), 780 + int(bd), LH.check_random)
            elif kind == "extremes":
                _on(int(bd), 782 + int(bd), LH.check_extremes)
            elif kind == "grey":
                grey(int(bd))
            elif kind == "snapshot":
                snapshot_and_scope(int(bd))
            else:
                {"gop": a_gop_under_the_pq_lut_preset_consumed_on_the_gpu, "stats": statistics_count_one_launch_per_request}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
