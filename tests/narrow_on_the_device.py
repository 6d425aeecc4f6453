"""GPU helper of tests/test_gpu_output_narrow.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and stops
at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to
be the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: the case matrix of tests/test_output_narrow_host.py with host destinations and with torch destinations - 2-D tensors or a (3, h, w)
tensor, contiguous or views with padded rows, inside a guard region ("matrix-<bit depth>"); k_output_narrow and every new instantiation of
k_output_yuv straight from the slot, with the checks that do not go through tests/narrow_ref.py and the state of the context
("straight-<bit depth>"); a 3840x2160 frame and a window of it as nv12 under DITHER ("4k"); a GOP whose frames are consumed on the GPU as nv12
behind vvr_output_stream_wait without the host waiting for any of them ("gop"); the statistics entries ("stats").  Everything is compared
with tests/narrow_ref.py as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import narrow_ref                                 # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_narrow_host as N               # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
import yuv_on_the_device as YD                    # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402


def _rec(bd, cf=1, **kw):
    rec = vvdec_amd.Reconstructor(S.W, S.H_, bit_depth=bd, chroma_format=cf, num_slots=2, num_streams=1, **kw)
    return rec


def _setup(bd, seed):
    import film_grain_ref
    import test_film_grain_host as H
    rec = _rec(bd)
    rng = np.random.default_rng(seed)
    picture = N.plant(film_grain_ref.grain_picture(rng, S.W, S.H_, bd, 1), bd)
    N.assert_planted(picture, bd)
    rec.write_picture(0, picture)
    if bd != 9:
        rec.set_film_grain(H._bank(rng))
    return rec, picture


def matrix_on_the_device(bd):
    rec, picture = _setup(bd, 200 + bd)
    aligned = []
    N.check_matrix(rec.L, rec.ctx, picture, bd, device=YD._into_tensors(rec, aligned), strides=(("row", 0), ("row+6", 0), ("row", 4)))
    assert any(all(a[3]) for a in aligned) and any(not any(a[3]) for a in aligned), aligned
    rec.close()


def straight_from_the_slot(bd):
    """k_output_narrow and the 20 new instantiations of k_output_yuv on 448x160, 200x64 (whole stores), 202x38 and 18x6 (pair by pair; partial
    last pieces in the caller's memory), into pageable memory and into contiguous tensors at a base of 256 bytes.  Then the checks that do not
    go through the restatement, the out-of-range words, and the state of the context - through Reconstructor.set_output_narrowing too"""
    rec, picture = _setup(bd, 205 + bd)
    aligned = []
    N.check_instantiations(rec.L, rec.ctx, picture, bd, device=YD._into_tensors(rec, aligned))
    assert (N.TINY, "nv12", None, (True, True)) in aligned and (N.TINY, "planar8", None, (True, True, True)) in aligned, aligned
    N.check_truncate_and_luma(rec.L, rec.ctx, bd, bd == 10)
    N.check_state(rec.L, rec.ctx, picture, bd)
    # the binding: names and numbers, and what it refuses
    win = (2, 6, 202, 38)
    p16 = rec.output_wait(rec.output_submit(0, window=win, fmt="planar16"))
    for name, mode in abi.NARROW_MODES.items():
        if not mode:
            continue
        rec.set_output_narrowing(name, 3)
        N.same_bytes(rec.output_wait(rec.output_submit(0, window=win, fmt="nv12")), narrow_ref.narrow(p16, bd, "nv12", mode, 3), name)
        rec.set_output_narrowing(mode)
        N.same_bytes(rec.output_wait(rec.output_submit(0, window=win, fmt="planar8", pinned=True)), narrow_ref.narrow(p16, bd, "planar8", mode, 0), name)
    for bad in (("dither", 4), (4, 0), ("floyd", 0)):
        try:
            rec.set_output_narrowing(*bad)
        except (vvdec_amd.VvrError, ValueError, TypeError):
            pass
        else:
            assert False, bad
    rec.set_output_narrowing("refuse")
    try:
        rec.output_submit(0, window=win, fmt="nv12")
    except vvdec_amd.VvrError as e:
        assert "8-bit output of a stream with more than 8 bits per sample" in str(e)
    else:
        assert False, "accepted with no mode set"
    write = lambda ctx, slot, p: rec.write_picture(slot, p)
    if bd == 10:
        N.check_cells_add_up(rec.L, rec.ctx, write, values=(3, 517, 1020))
        N.check_multiples_of_4(rec.L, rec.ctx, write, np.random.default_rng(207))
    N.check_out_of_range_words(rec.L, rec.ctx, write, np.random.default_rng(208))
    rec.close()
    # 4:0:0: planar8 alone, luma alone
    rec = _rec(bd, cf=0)
    luma = N.plant([np.random.default_rng(209).integers(0, 1 << bd, (S.H_, S.W)).astype(np.uint16)], bd)
    rec.write_picture(0, luma)
    for mode, phase in N.MODES:
        rec.set_output_narrowing(mode, phase)
        for win in (N.TINY, (2, 6, 202, 38)):
            N.same_bytes(rec.output_wait(rec.output_submit(0, window=win, fmt="planar8")), [narrow_ref.reduce(S.crop(luma, win)[0], bd, mode, phase)], "4:0:0 %r" % (win,))
    rec.close()


def a_4k_frame_and_a_window_of_it():
    """3840x2160, 10 bits, as nv12 under DITHER into contiguous tensors: the frame, and a window at an offset whose chroma rows are of odd length
    (1913 samples), against narrow_ref on the picture that was written"""
    Wk, Hk = 3840, 2160
    rng = np.random.default_rng(201)
    planes = [rng.integers(0, 1 << 10, (Hk >> s, Wk >> s), dtype=np.uint16) for s in (0, 1, 1)]
    rec = vvdec_amd.Reconstructor(Wk, Hk, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    for win, phase in [((0, 0, Wk, Hk), 0), ((2, 4, 3826, 2152), 3)]:
        assert (win[2] >> 1) & 1 == (0 if win[0] == 0 else 1)
        rec.set_output_narrowing("dither", phase)
        want = narrow_ref.narrow(S.crop(planes, win), 10, "nv12", narrow_ref.DITHER, phase)
        shapes, dt = abi.output_plane_shapes(win, "nv12", None, 3)
        into = [torch.zeros(s, dtype=torch.uint8, device="cuda") for s in shapes]
        torch.cuda.synchronize()       # (idle before the request: the zeros are written on torch's stream)
        got = rec.output_wait(rec.output_submit(0, window=win, fmt="nv12", into=into))
        assert all(a is b for a, b in zip(got, into))
        for k, w_ in enumerate(want):
            g = into[k].cpu().numpy()
            assert g.tobytes() == w_.tobytes(), "nv12 %r plane %d: %d bytes differ" % (win, k, int((g != w_).sum()))
    rec.close()


def frames_consumed_on_the_gpu_without_the_host_waiting():
    """a GOP and the first pictures of the next one (which overwrite the first GOP's slots), every picture's nv12 output requested into its own
    tensors the moment the picture is submitted, the phase of the dither moving from frame to frame; a side stream waits for each request on
    the device (output_stream_wait) and clones the tensors; the host waits for nothing until the side stream is synchronised at the end"""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [1993, 1994])
    order = [(0, n) for n in range(len(plans))] + [(1, n) for n in range(3)]       # eight requests: the ring
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for k, (g, n) in enumerate(order):
        jobs.append(rec.decompress_picture(synth.picture_for_plan(plans[n], Wd, Hd, seed=1993 + g, tool_flags=G.TOOLS, **G.GEO)))
        into = [torch.empty((Hd, Wd), dtype=torch.uint8, device="cuda"), torch.empty((Hd // 2, Wd), dtype=torch.uint8, device="cuda")]
        rec.set_output_narrowing("dither", k & 3)      # (a request takes the phase that is set when it is submitted)
        tickets.append(rec.output_submit(plans[n].slot, job=jobs[-1], fmt="nv12", into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append([t.clone() for t in into])
    side.synchronize()
    for k, ((g, n), c) in enumerate(zip(order, clones)):
        w_ = narrow_ref.narrow(want[g][n], 10, "nv12", narrow_ref.DITHER, k & 3)
        for pl in range(2):
            got = c[pl].cpu().numpy()
            assert got.tobytes() == w_[pl].tobytes(), "GOP %d picture %d plane %d: %d bytes differ" % (g, n, pl, int((got != w_[pl]).sum()))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_name_the_kernels():
    """k_output_narrow: one launch per planar8 / nv12 request of a context of 10 bits, also behind k_film_grain / k_rescale, and its algorithmic
    bytes; the narrowed 4:2:2 / 4:4:4 formats count under k_output_yuv; the 16-bit formats stay with k_output_frame"""
    import film_grain_ref
    rec = _rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(202), S.W, S.H_, 10, 1))
    rec.set_output_narrowing("round")
    rec.enable_stats()
    win = (8, 4, 200, 64)
    for fmt, size in [("nv12", None), ("planar8", None), ("planar8", (300, 96)), ("p010", None), ("planar16", None), ("yuv444p8", None), ("uyvy", (300, 96)), ("yuv422p8", None), ("y210", None)]:
        rec.output_wait(rec.output_submit(0, window=win, fmt=fmt, size=size))
    stats = {s["name"]: s for s in rec.stats()}
    assert stats["k_output_narrow"]["launches"] == 3 and stats["k_output_frame"]["launches"] == 2 and stats["k_output_yuv"]["launches"] == 4, stats
    # read: 2 bytes a sample of the three planes (1.5 samples a luma sample); written: a byte each
    assert stats["k_output_narrow"]["algo_bytes"] == (2 * 200 * 64 + 300 * 96) * 3 * 3 // 2, stats
    # read: 3 bytes a luma sample; written: 3, 2 and 2 bytes a luma sample, and y210's 4
    assert stats["k_output_yuv"]["algo_bytes"] == 3 * (3 * 200 * 64 + 300 * 96) + 200 * 64 * (3 + 2 + 4) + 300 * 96 * 2, stats
    arr = (abi.KernelStat * 64)()
    n = rec.L.vvr_get_stats(rec.ctx, arr, 64)
    assert n == len(stats) and arr[n - 1].name == b"k_output_narrow"      # (the last id of the list)
    rec.close()


def main(names):
    for name in names:
        try:
            if name.startswith("matrix-"):
                matrix_on_the_device(int(name.split("-")[1]))
            elif name.startswith("straight-"):
                straight_from_the_slot(int(name.split("-")[1]))
            else:
                {"4k": a_4k_frame_and_a_window_of_it, "gop": frames_consumed_on_the_gpu_without_the_host_waiting, "stats": statistics_name_the_kernels}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
