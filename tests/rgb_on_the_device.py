"""GPU helper of tests/test_gpu_output_rgb.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and stops at
the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to be the
first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: the case matrix of tests/test_output_rgb_host.py with host destinations and with torch destinations - one (3, h, w) tensor per request,
contiguous or a view with padded rows and planes, inside a guard region ("matrix-<bit depth>"); every instantiation of the kernel straight
from the slot - formats x chroma positions x whole and pair-by-pair stores ("straight-<bit depth>"); a 3840x2160 frame and a window of it ("4k");
a GOP whose frames are consumed on the GPU behind vvr_output_stream_wait without the host waiting for any of them ("gop"); the statistics
entry ("stats").  Everything is compared with tests/rgb_ref.py as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import rgb_ref                                    # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_rgb_host as R                  # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402

FILL = S.FILL
TORCH_DT = {np.uint8: torch.uint8, np.uint16: torch.int16, np.float16: torch.float16}      # (2-byte integers: the element size is what counts)


class GuardedTensor:
    """a (3, h, w) destination inside the uint8 tensor `mem` (filled with FILL here), 256 + mis bytes from its start: contiguous, or - padded -
    a view of a (3, h + 1, w + 3) tensor; check(): the planes hold `want` and no other byte of `mem` has changed"""

    def __init__(self, mem, win, fmt, size, padded, mis):
        shapes, dt = abi.output_plane_shapes(win, fmt, size, 3)
        (h, w), item = shapes[0], np.dtype(dt).itemsize
        self.full = (3, h + 1, w + 3) if padded else (3, h, w)
        self.h, self.w, self.item, self.off, self.mem = h, w, item, 256 + mis, mem
        self.nbytes = int(np.prod(self.full)) * item
        assert mem.data_ptr() % 256 == 0 and self.off + self.nbytes + 256 <= mem.numel()
        mem.fill_(FILL)
        torch.cuda.synchronize()       # (the fill runs on torch's stream, the request on the context's: a destination must be idle when it is submitted)
        self.into = mem[self.off:self.off + self.nbytes].view(TORCH_DT[dt]).view(self.full)[:, :h, :w]
        assert self.into.is_contiguous() == (not padded)

    def check(self, want, what):
        host = self.mem[:self.off + self.nbytes + 256].cpu().numpy()
        exp = np.full(host.shape, FILL, np.uint8)
        inner = exp[self.off:self.off + self.nbytes].reshape(self.full[0], self.full[1], self.full[2] * self.item)
        for k in range(3):
            inner[k, :self.h, :self.w * self.item] = np.ascontiguousarray(want[k]).view(np.uint8).reshape(self.h, self.w * self.item)
        bad = host != exp
        if bad.any():
            inside = np.zeros(host.shape, bool)
            inside[self.off:self.off + self.nbytes].reshape(inner.shape)[:, :self.h, :self.w * self.item] = True
            assert False, "%s: %d bytes of the planes differ, %d bytes outside them changed" % (what, int((bad & inside).sum()), int((bad & ~inside).sum()))


def _rec(bd, **kw):
    rec = vvdec_amd.Reconstructor(S.W, S.H_, bit_depth=bd, chroma_format=1, num_slots=2, num_streams=1, **kw)
    return rec


def _setup(bd, seed):
    import film_grain_ref
    import test_film_grain_host as H
    rec = _rec(bd)
    rng = np.random.default_rng(seed)
    picture = film_grain_ref.grain_picture(rng, S.W, S.H_, bd, 1)
    rec.write_picture(0, picture)
    if bd != 9:
        rec.set_film_grain(H._bank(rng))
    return rec, picture


def _into_a_tensor(rec, aligned):
    """the `device` of R.check_matrix / R.check_instantiations: one request into a (3, h, w) tensor inside a guard region, compared; aligned
    collects, for the contiguous tensors, which planes start at a multiple of 32 bytes (those the kernel stores itself)"""
    mem = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def device(L, ctx, slot, win, fmt, ncomp, want, what, seed, size, grain, stride_kind, mis, col):
        d = GuardedTensor(mem, win, fmt, size, stride_kind != "row", mis)
        if stride_kind == "row":
            aligned.append((win, fmt, size, tuple(d.into[k].data_ptr() % 32 == 0 for k in range(3))))
        if seed is not None:
            rec.set_film_grain_seed(seed)
        t = rec.output_submit(slot, window=win, fmt=fmt, size=size, collocated=col, grain=grain, into=d.into)
        assert len(rec._reg[t]) == 1
        assert rec.output_wait(t) is d.into
        d.check(want, what)
        assert L.vvr_device_unregister(ctx, d.into.data_ptr()) == abi.VVR_ERR_PARAMETER      # (unregistered by output_wait)
    return device


def matrix_on_the_device(bd):
    rec, picture = _setup(bd, 90 + bd)
    aligned = []
    R.check_matrix(rec.L, rec.ctx, picture, bd, device=_into_a_tensor(rec, aligned), strides=(("row", 0), ("row+6", 0), ("row", 2)))
    assert any(a[3] == (True, True, True) for a in aligned) and any(a[3] == (False, False, False) for a in aligned)
    rec.close()


def every_instantiation_straight_from_the_slot(bd):
    """formats x chroma positions on 448x160 and 200x64 (whole stores) and 202x38 (pair by pair), into pageable memory and into contiguous
    (3, h, w) tensors: planes 1 and 2 start at h * w * bytes, so both the store by the kernel and the laid-out copy are taken"""
    rec, picture = _setup(bd, 95 + bd)
    aligned = []
    R.check_instantiations(rec.L, rec.ctx, picture, bd, device=_into_a_tensor(rec, aligned))
    assert ((2, 6, 202, 38), "rgb8", None, (True, False, False)) in aligned and ((0, 0, 448, 160), "rgb16", None, (True, True, True)) in aligned, aligned
    rec.close()


def a_4k_frame_and_a_window_of_it():
    """3840x2160, 10 bits, as rgbf16 into contiguous tensors: the frame (rows of a multiple of 8 samples: whole stores) and a window at an offset
    whose width is no multiple of 8 (pair by pair), against rgb_ref on the picture that was written"""
    Wk, Hk = 3840, 2160
    rng = np.random.default_rng(91)
    planes = [rng.integers(0, 1 << 10, (Hk >> s, Wk >> s), dtype=np.uint16) for s in (0, 1, 1)]
    rec = vvdec_amd.Reconstructor(Wk, Hk, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    for win, col, colour in [((0, 0, Wk, Hk), (True, False), (9, 0)), ((2, 4, 3826, 2152), (False, True), (1, 1))]:
        rec.set_output_colour(*colour)
        want = rgb_ref.rgb(S.crop(planes, win), 10, "rgbf16", colour[0], bool(colour[1]), col)
        into = torch.zeros((3, win[3], win[2]), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()       # (idle before the request: the zeros are written on torch's stream)
        got = rec.output_wait(rec.output_submit(0, window=win, fmt="rgbf16", collocated=col, into=into))
        assert got is into
        host = into.cpu().numpy()
        for k in range(3):
            assert host[k].tobytes() == want[k].tobytes(), "%r plane %d: %d samples differ" % (win, k, int((host[k].view(np.uint16) != want[k].view(np.uint16)).sum()))
    rec.close()


def frames_consumed_on_the_gpu_without_the_host_waiting():
    """a GOP and the first pictures of the next one (which overwrite the first GOP's slots), every picture's rgbf16 output requested into its own
    (3, h, w) tensor the moment the picture is submitted; a side stream waits for each request on the device (output_stream_wait) and clones the
    tensor; the host waits for nothing until the side stream is synchronised at the end"""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [993, 994])
    order = [(0, n) for n in range(len(plans))] + [(1, n) for n in range(3)]       # eight requests: the ring
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    rec.set_output_colour(1, False)
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for g, n in order:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(plans[n], Wd, Hd, seed=993 + g, tool_flags=G.TOOLS, **G.GEO)))
        into = torch.empty((3, Hd, Wd), dtype=torch.float16, device="cuda")
        tickets.append(rec.output_submit(plans[n].slot, job=jobs[-1], fmt="rgbf16", into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append(into.clone())
    side.synchronize()
    for (g, n), c in zip(order, clones):
        w_ = rgb_ref.rgb(want[g][n], 10, "rgbf16", 1, False, (True, False))
        got = c.cpu().numpy()
        for k in range(3):
            assert got[k].tobytes() == w_[k].tobytes(), "GOP %d picture %d plane %d: %d samples differ" % (g, n, k, int((got[k].view(np.uint16) != w_[k].view(np.uint16)).sum()))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_name_the_kernel():
    """k_output_rgb: one launch per RGB request, also behind k_film_grain / k_rescale; the other formats do not count there"""
    import film_grain_ref
    rec = _rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(92), S.W, S.H_, 10, 1))
    rec.set_output_colour(5, True)
    rec.enable_stats()
    for fmt, size in [("rgb8", None), ("rgb16", None), ("rgbf16", None), ("planar16", None), ("rgb16", (300, 96)), ("p010", None), ("rgb8", None)]:
        rec.output_wait(rec.output_submit(0, window=(8, 4, 200, 64), fmt=fmt, size=size))
    stats = {s["name"]: s["launches"] for s in rec.stats()}
    assert stats.get("k_output_rgb") == 5 and stats.get("k_output_frame") == 2, stats
    rec.close()


def main(names):
    for name in names:
        try:
            if name.startswith("matrix-"):
                matrix_on_the_device(int(name.split("-")[1]))
            elif name.startswith("straight-"):
                every_instantiation_straight_from_the_slot(int(name.split("-")[1]))
            else:
                {"4k": a_4k_frame_and_a_window_of_it, "gop": frames_consumed_on_the_gpu_without_the_host_waiting, "stats": statistics_name_the_kernel}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
