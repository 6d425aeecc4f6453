"""GPU helper of tests/test_gpu_output_yuv.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and stops at
the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to be the
first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: the case matrix of tests/test_output_yuv_host.py with host destinations and with torch destinations - a (3, h, w) tensor, three 2-D
tensors or one, contiguous or views with padded rows, inside a guard region ("matrix-<bit depth>"); every instantiation of the kernel straight
from the slot and the two cross-checks that do not go through tests/yuv_ref.py ("straight-<bit depth>"); a 3840x2160 frame and a window of it as
v210 and as yuv444p16 ("4k"); a GOP whose frames are consumed on the GPU as y210 behind vvr_output_stream_wait without the host waiting for any of
them ("gop"); the statistics entry and the checks of `into` ("stats").  Everything is compared with tests/yuv_ref.py as bytes."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import yuv_ref                                    # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_yuv_host as Y                  # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402

FILL = S.FILL
TORCH_DT = {np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32}      # (the element size is what counts)


class Guarded:
    """the destination of one request inside the uint8 tensor `mem` (filled with FILL here), 256 + mis bytes from its start: a (3, h, w) tensor
    for the planar 4:4:4 formats, three 2-D tensors for the planar 4:2:2 ones, one 2-D tensor for the packed ones - contiguous, or - padded -
    views of tensors with three more elements to a row (and one more row to a plane of the 3-D tensor); check(): the planes hold `want` and no
    other byte of `mem` has changed"""

    def __init__(self, mem, win, fmt, size, padded, mis):
        shapes, dt = abi.output_plane_shapes(win, fmt, size, 3)
        item, tdt = np.dtype(dt).itemsize, TORCH_DT[dt]
        assert mem.data_ptr() % 256 == 0 and mis % item == 0
        mem.fill_(FILL)
        torch.cuda.synchronize()       # (the fill runs on torch's stream, the request on the context's: a destination must be idle when it is submitted)
        self.mem, self.spans, off = mem, [], 256 + mis      # spans: (first byte, rows, bytes of a row, bytes from row to row) of every plane
        if fmt in ("yuv444p8", "yuv444p16"):
            h, w = shapes[0]
            full = (3, h + 1, w + 3) if padded else (3, h, w)
            nbytes = int(np.prod(full)) * item
            self.into = mem[off:off + nbytes].view(tdt).view(full)[:, :h, :w]
            self.planes = list(self.into)
            self.spans = [(off + k * full[1] * full[2] * item, h, w * item, full[2] * item) for k in range(3)]
            off += nbytes
        else:
            self.planes = []
            for r, n in shapes:
                fulln = n + 3 if padded else n
                nbytes = r * fulln * item
                self.planes.append(mem[off:off + nbytes].view(tdt).view(r, fulln)[:, :n])
                self.spans.append((off, r, n * item, fulln * item))
                off = (off + nbytes + 255) // 256 * 256 + 256 + mis
            self.into = self.planes if len(self.planes) > 1 else self.planes[0]
        self.end = off + 256
        assert self.end <= mem.numel()

    def check(self, want, what):
        host = self.mem[:self.end].cpu().numpy()
        exp, inside = np.full(host.shape, FILL, np.uint8), np.zeros(host.shape, bool)
        assert len(want) == len(self.spans), what
        for (first, rows, row, pitch), w_ in zip(self.spans, want):
            b = np.ascontiguousarray(w_).view(np.uint8).reshape(rows, row)
            for j in range(rows):
                exp[first + j * pitch:first + j * pitch + row] = b[j]
                inside[first + j * pitch:first + j * pitch + row] = True
        bad = host != exp
        assert not bad.any(), "%s: %d bytes of the planes differ, %d bytes outside them changed" % (what, int((bad & inside).sum()), int((bad & ~inside).sum()))


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


def _into_tensors(rec, aligned):
    """the `device` of Y.check_matrix / Y.check_instantiations: one request into tensors inside a guard region, compared; aligned collects, for
    the contiguous destinations, which planes start at a multiple of 32 bytes (those the kernel stores itself)"""
    mem = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def device(L, ctx, slot, win, fmt, ncomp, want, what, seed, size, grain, stride_kind, mis, col):
        d = Guarded(mem, win, fmt, size, stride_kind != "row", mis)
        if stride_kind == "row":
            aligned.append((win, fmt, size, tuple(t.data_ptr() % 32 == 0 for t in d.planes)))
        if seed is not None:
            rec.set_film_grain_seed(seed)
        t = rec.output_submit(slot, window=win, fmt=fmt, size=size, collocated=col, grain=grain, into=d.into)
        got = rec.output_wait(t)
        assert got is d.into or (isinstance(got, list) and all(a is b for a, b in zip(got, d.planes))), what
        d.check(want, what)
        assert L.vvr_device_unregister(ctx, d.planes[0].data_ptr()) == abi.VVR_ERR_PARAMETER      # (unregistered by output_wait)
    return device


def matrix_on_the_device(bd):
    rec, picture = _setup(bd, 170 + bd)
    aligned = []
    Y.check_matrix(rec.L, rec.ctx, picture, bd, device=_into_tensors(rec, aligned), strides=(("row", 0), ("row+6", 0), ("row", 4)))
    assert any(all(a[3]) for a in aligned) and any(not any(a[3]) for a in aligned), aligned
    rec.close()


def every_instantiation_straight_from_the_slot(bd):
    """formats x chroma positions on 448x160 and 200x64 (whole stores) and 202x38 (pixel pair by pixel pair), into pageable memory and into
    contiguous tensors at a base of 256 bytes: the planes of the 2-D tensors are stored by the kernel itself, planes 1 and 2 of a (3, h, w)
    tensor start at h * w * bytes, so both the store by the kernel and the laid-out copy are taken.  Then the two cross-checks."""
    rec, picture = _setup(bd, 175 + bd)
    aligned = []
    Y.check_instantiations(rec.L, rec.ctx, picture, bd, device=_into_tensors(rec, aligned))
    assert ((2, 6, 202, 38), "v210", None, (True,)) in aligned and ((0, 0, 448, 160), "yuv444p16", None, (True, True, True)) in aligned, aligned
    assert ((2, 6, 202, 38), "yuv422p16", None, (True, True, True)) in aligned and ((2, 6, 202, 38), "yuv444p16", None, (True, False, False)) in aligned, aligned
    Y.check_the_planes_are_the_ones_rgb_converts(rec.L, rec.ctx, bd)
    Y.check_phase_0_is_the_identity(rec.L, rec.ctx, picture)
    rec.close()


def a_4k_frame_and_a_window_of_it():
    """3840x2160, 10 bits, into contiguous tensors as v210 and as yuv444p16: the frame (rows of 640 full groups; of a multiple of 8 samples:
    whole stores) and a window at an offset (rows that end in a group of four pixels; pixel pair by pixel pair), against yuv_ref on the
    picture that was written"""
    Wk, Hk = 3840, 2160
    rng = np.random.default_rng(171)
    planes = [rng.integers(0, 1 << 10, (Hk >> s, Wk >> s), dtype=np.uint16) for s in (0, 1, 1)]
    rec = vvdec_amd.Reconstructor(Wk, Hk, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    for win, col in [((0, 0, Wk, Hk), (True, False)), ((2, 4, 3826, 2152), (False, True))]:
        assert win[2] % 6 == (0 if win[0] == 0 else 4)
        for fmt in ("v210", "yuv444p16"):
            want = yuv_ref.yuv(S.crop(planes, win), 10, fmt, col)
            shapes, dt = abi.output_plane_shapes(win, fmt, None, 3)
            into = torch.zeros((3,) + shapes[0] if fmt == "yuv444p16" else shapes[0], dtype=TORCH_DT[dt], device="cuda")
            torch.cuda.synchronize()       # (idle before the request: the zeros are written on torch's stream)
            got = rec.output_wait(rec.output_submit(0, window=win, fmt=fmt, collocated=col, into=into))
            assert got is into
            host = into.cpu().numpy().view(dt)
            for k, w_ in enumerate(want):
                g = host[k] if fmt == "yuv444p16" else host
                assert g.tobytes() == w_.tobytes(), "%s %r plane %d: %d elements differ" % (fmt, win, k, int((g != w_).sum()))
    rec.close()


def frames_consumed_on_the_gpu_without_the_host_waiting():
    """a GOP and the first pictures of the next one (which overwrite the first GOP's slots), every picture's y210 output requested into its own
    (h, 2 w) tensor the moment the picture is submitted; a side stream waits for each request on the device (output_stream_wait) and clones the
    tensor; the host waits for nothing until the side stream is synchronised at the end"""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [1993, 1994])
    order = [(0, n) for n in range(len(plans))] + [(1, n) for n in range(3)]       # eight requests: the ring
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    side = torch.cuda.Stream()
    jobs, tickets, clones = [], [], []
    for g, n in order:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(plans[n], Wd, Hd, seed=1993 + g, tool_flags=G.TOOLS, **G.GEO)))
        into = torch.empty((Hd, 2 * Wd), dtype=torch.int16, device="cuda")
        tickets.append(rec.output_submit(plans[n].slot, job=jobs[-1], fmt="y210", collocated=(False, False), into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append(into.clone())
    side.synchronize()
    for (g, n), c in zip(order, clones):
        w_, = yuv_ref.yuv(want[g][n], 10, "y210", (False, False))
        got = c.cpu().numpy().view(np.uint16)
        assert got.tobytes() == w_.tobytes(), "GOP %d picture %d: %d words differ" % (g, n, int((got != w_).sum()))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def statistics_name_the_kernel():
    """k_output_yuv: one launch per request of a new format, also behind k_film_grain / k_rescale; the other formats do not count there.  And
    what `into` must look like"""
    import film_grain_ref
    rec = _rec(10)
    rec.write_picture(0, film_grain_ref.grain_picture(np.random.default_rng(172), S.W, S.H_, 10, 1))
    rec.set_output_colour(5, True)
    rec.enable_stats()
    win = (8, 4, 200, 64)
    for fmt, size in [("yuv444p16", None), ("v210", None), ("y210", None), ("planar16", None), ("yuv422p16", (300, 96)), ("rgb16", None), ("y410", None), ("p010", None)]:
        rec.output_wait(rec.output_submit(0, window=win, fmt=fmt, size=size))
    stats = {s["name"]: s for s in rec.stats()}
    assert stats["k_output_yuv"]["launches"] == 5 and stats["k_output_rgb"]["launches"] == 1 and stats["k_output_frame"]["launches"] == 2, stats
    # read: 3 bytes a luma sample; written: 6, 34 groups of 16 bytes a row, 4, 4 and 4 bytes a luma sample
    assert stats["k_output_yuv"]["algo_bytes"] == 3 * (4 * 200 * 64 + 300 * 96) + 200 * 64 * (6 + 4 + 4) + 34 * 16 * 64 + 300 * 96 * 4, stats
    arr = (abi.KernelStat * 64)()
    assert rec.L.vvr_get_stats(rec.ctx, arr, 64) == len(stats) and any(arr[i].name == b"k_output_yuv" for i in range(len(stats)))

    def bad(fmt, into, text):
        try:
            rec.output_submit(0, window=win, fmt=fmt, into=into)
        except ValueError as e:
            assert text in str(e), (fmt, str(e))
        else:
            assert False, "%s: `into` was accepted" % fmt
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    bad("v210", z((64, 34 * 4), torch.int16), "4-byte elements")
    bad("v210", z((64, 200), torch.int32), "of shape (64, 136)")
    bad("y210", z((64, 400), torch.int32), "2-byte elements")
    bad("y410", z((3, 64, 200), torch.int32), "one 2-D tensor")
    bad("uyvy", z((64, 400), torch.uint8).cpu(), "on the context's device")
    bad("yuv422p16", z((3, 64, 200), torch.int16), "4:4:4")
    bad("yuv422p16", [z((64, 200), torch.int16)] * 3, "of shape (64, 100)")
    bad("yuv444p16", [z((64, 200), torch.int16)] * 2, "needs 3 planes")
    bad("yuv444p16", z((3, 64, 200), torch.uint8), "2-byte elements")
    assert not rec._reg      # (nothing stays registered behind a refused argument)
    # ... and what is accepted: a list for a planar 4:4:4 format, as for planar RGB
    into = [z((64, 200), torch.int16) for _ in range(3)]
    torch.cuda.synchronize()
    got = rec.output_wait(rec.output_submit(0, window=win, fmt="yuv444p16", into=into))
    assert all(a is b for a, b in zip(got, into))
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
