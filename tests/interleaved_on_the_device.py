"""GPU helper of tests/test_gpu_output_interleaved.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and
stops at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has
to be the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: the case matrix of tests/test_output_interleaved_host.py with host destinations and with torch destinations - (h, w, C) tensors for the
interleaved formats, (h, w) int32 for rgb10a2, (3, h, w) float32 for rgbf32, contiguous at an aligned base (the kernel stores), misaligned by 2
bytes or with padded rows (the laid-out copy), inside a guard region ("matrix-<bit depth>"); every instantiation of the store straight from the
slot - classes x chroma positions x whole and pair-by-pair x with and without a transform on five windows ("straight-<bit depth>"); the new
formats against the planar requests of the same frame and the normalisation's state ("cross-<bit depth>"); a GOP whose frames are consumed on the
GPU as bgra8 and normalised rgbf32 behind vvr_output_stream_wait without the host waiting for any of them ("gop"); the statistics entry
("stats").  Everything is compared as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import interleaved_ref as IR                      # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_interleaved_host as I          # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402

FILL = S.FILL
TORCH_DT = {np.uint8: torch.uint8, np.float16: torch.float16, np.uint32: torch.int32, np.float32: torch.float32}      # (4-byte integers: the element size is what counts)


class GuardedTensor:
    """the destination of one request inside the uint8 tensor `mem` (filled with FILL here), 256 + mis bytes from its start: (h, w, C), (h, w)
    or (3, h, w), contiguous, or - padded - a view of a tensor with one more row and three more pixels per row; check(): the rows hold `want`
    and no other byte of `mem` has changed"""

    def __init__(self, mem, win, fmt, size, padded, mis):
        shapes, dt = abi.output_plane_shapes(win, fmt, size, 3)
        item, c = np.dtype(dt).itemsize, abi.OUT_INTERLEAVED.get(fmt, 1)
        mis = mis if item < 4 else 2 * mis      # (a tensor of 4-byte elements lies at a multiple of 4: off the 32-byte grid by 4 instead of 2)
        (h, n), planes = shapes[0], len(shapes)
        w = n // c
        self.rows, self.row, self.planes = h, n * item, planes                      # rows of a plane, bytes of a row
        self.stride = (w + 3) * c * item if padded else self.row                    # bytes from row to row
        self.plane = (h + 1) * self.stride if padded else h * self.stride          # bytes from plane to plane
        self.off, self.mem, self.nbytes = 256 + mis, mem, planes * self.plane
        assert mem.data_ptr() % 256 == 0 and self.off + self.nbytes + 256 <= mem.numel()
        mem.fill_(FILL)
        torch.cuda.synchronize()       # (the fill runs on torch's stream, the request on the context's: a destination must be idle when it is submitted)
        t = mem[self.off:self.off + self.nbytes].view(TORCH_DT[dt])
        hh, ww = (h + 1, w + 3) if padded else (h, w)
        if planes == 3:
            self.into = t.view(3, hh, ww)[:, :h, :w]
        elif fmt == "rgb10a2":
            self.into = t.view(hh, ww)[:h, :w]
        else:
            self.into = t.view(hh, ww, c)[:h, :w]
        assert self.into.is_contiguous() == (not padded)

    def check(self, want, what):
        host = self.mem[:self.off + self.nbytes + 256].cpu().numpy()
        exp = np.full(host.shape, FILL, np.uint8)
        inside = np.zeros(host.shape, bool)
        for k in range(self.planes):
            w_ = np.ascontiguousarray(want[k]).view(np.uint8).reshape(self.rows, self.row)
            for j in range(self.rows):
                at = self.off + k * self.plane + j * self.stride
                exp[at:at + self.row] = w_[j]
                inside[at:at + self.row] = True
        bad = host != exp
        assert not bad.any(), "%s: %d bytes of the rows differ, %d bytes outside them changed" % (what, int((bad & inside).sum()), int((bad & ~inside).sum()))


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
    """the `device` of I.check_matrix / I.check_straight: one request into a tensor inside a guard region, compared; aligned collects, for the
    contiguous tensors, whether the base is a multiple of 32 bytes (then the kernel stores plane 0 itself)"""
    mem = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def device(L, ctx, slot, win, fmt, ncomp, want, what, seed, size, grain, stride_kind, mis, col):
        d = GuardedTensor(mem, win, fmt, size, stride_kind != "row", mis)
        if stride_kind == "row":
            aligned.append((fmt, d.into.data_ptr() % 32 == 0))
        if seed is not None:
            rec.set_film_grain_seed(seed)
        t = rec.output_submit(slot, window=win, fmt=fmt, size=size, collocated=col, grain=grain, into=d.into)
        assert len(rec._reg[t]) == 1
        assert rec.output_wait(t) is d.into
        d.check(want, what)
        assert L.vvr_device_unregister(ctx, d.into.data_ptr()) == abi.VVR_ERR_PARAMETER      # (unregistered by output_wait)
    return device


def matrix_on_the_device(bd):
    rec, picture = _setup(bd, 490 + bd)
    aligned = []
    I.check_matrix(rec.L, rec.ctx, picture, bd, device=_into_a_tensor(rec, aligned), strides=(("row", 0), ("row+6", 0), ("row", 2)))
    assert set(aligned) == set((fmt, a) for fmt in I.FORMATS for a in (False, True)), aligned
    rec.close()


def every_instantiation_straight_from_the_slot(bd):
    rec, picture = _setup(bd, 495 + bd)
    aligned = []
    I.check_straight(rec.L, rec.ctx, picture, bd, device=_into_a_tensor(rec, aligned))
    assert all(a for _, a in aligned) and set(f for f, _ in aligned) == set(I.FORMATS)      # (every one of them stored by the kernel)
    rec.close()


def cross_checks_and_state(bd):
    rec, picture = _setup(bd, 500 + bd)
    for tf in (None, I.transforms(bd)["pq"]):
        I.check_against_the_planar_formats(rec.L, rec.ctx, bd, tf)
    I.check_normalisation_state(rec.L, rec.ctx, picture, bd)
    rec.close()


def frames_consumed_on_the_gpu_without_the_host_waiting():
    """a GOP (test_gpu_output_queue's small stream), every picture's bgra8 and normalised rgbf32 output requested the moment the picture is
    submitted, each into its own tensor; a side stream waits for each request on the device (output_stream_wait) and clones the tensor; the
    host waits for nothing until the side stream is synchronised.  Two requests per picture: four pictures fill the ring, so the GOP goes in
    two parts, the I picture with the first three B pictures and the last B picture."""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [993])[0]
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    norm = I.NORMS[1]
    rec.set_output_colour(1, False)
    rec.set_output_normalisation(*norm)
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for part in (range(4), range(4, len(plans))):
        for t in tickets:              # (the ring has eight entries: the tickets of the part before are retired - its stream has been synchronised)
            rec.output_wait(t)
        tickets = []
        for n in part:
            jobs.append(rec.decompress_picture(synth.picture_for_plan(plans[n], Wd, Hd, seed=993, tool_flags=G.TOOLS, **G.GEO)))
            for fmt, into in (("bgra8", torch.empty((Hd, Wd, 4), dtype=torch.uint8, device="cuda")), ("rgbf32", torch.empty((3, Hd, Wd), dtype=torch.float32, device="cuda"))):
                tickets.append(rec.output_submit(plans[n].slot, job=jobs[-1], fmt=fmt, into=into))
                rec.output_stream_wait(tickets[-1], side)
                with torch.cuda.stream(side):
                    clones.append((n, fmt, into.clone()))
        side.synchronize()
    for n, fmt, c in clones:
        w_ = IR.frame(want[n], 10, fmt, 1, False, (True, False), None, norm)
        got = c.cpu().numpy()
        got = [got.reshape(Hd, Wd * 4)] if fmt == "bgra8" else list(got)
        I.same_planes(got, w_, "picture %d as %s" % (n, fmt))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_name_the_kernel():
    """k_output_rgb: one launch per request of a new format, also behind k_film_grain / k_rescale; the other formats do not count there"""
    import film_grain_ref
    rec = _rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(492), S.W, S.H_, 10, 1))
    rec.set_output_colour(5, True)
    rec.enable_stats()
    requests = [(fmt, None) for fmt in I.FORMATS] + [("planar16", None), ("rgba8", (300, 96)), ("p010", None), ("rgbf32", (134, 26))]
    for fmt, size in requests:
        rec.output_wait(rec.output_submit(0, window=(8, 4, 200, 64), fmt=fmt, size=size))
    stats = {s["name"]: s["launches"] for s in rec.stats()}
    assert stats.get("k_output_rgb") == 9 and stats.get("k_output_frame") == 2, stats
    rec.close()


def main(names):
    for name in names:
        try:
            if "-" in name:
                kind, bd = name.split("-")
                {"matrix": matrix_on_the_device, "straight": every_instantiation_straight_from_the_slot, "cross": cross_checks_and_state}[kind](int(bd))
            else:
                {"gop": frames_consumed_on_the_gpu_without_the_host_waiting, "stats": statistics_name_the_kernel}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
