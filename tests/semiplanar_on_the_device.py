"""GPU helper of tests/test_gpu_output_semiplanar.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and
stops at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to
be the first one the process initialises (the order bench.py and tests/two_back_ends_on_one_device.py use) - in the pytest process the library's
runtime is up long before, and torch then finds no device.

The cases: the case matrix of tests/test_output_semiplanar_host.py with the device destinations in torch tensors
(Reconstructor.output_submit(into=...)) and in memory of vvr_device_alloc ("matrix-<bit depth>-<format>"), a 3840x2160 frame through the direct and
the laid-out store ("4k"), and a GOP whose frames are consumed on the GPU behind vvr_output_stream_wait without the host waiting for any of them
("gop"; ordered on the device: nothing there depends on timing)."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import test_gpu_output_queue as G                 # noqa: E402
import test_output_semiplanar_host as S           # noqa: E402
from vvdec_amd import abi, stream, synth          # noqa: E402

FILL = S.FILL


class TensorPlanes:
    """destination planes as strided views into one uint8 tensor `mem` (filled with FILL here): every plane at a 256-byte aligned offset moved by
    `mis` bytes, guard bytes around it"""

    def __init__(self, mem, win, fmt, size, stride_kind, mis):
        shapes, dt = abi.output_plane_shapes(win, fmt, size, 3)
        item = np.dtype(dt).itemsize
        tdt = torch.uint8 if item == 1 else torch.int16          # (2-byte elements: the element size is what counts)
        self.geo, self.mem, self.off, self.views = S.layout(shapes, dt, stride_kind), mem, [], []
        assert mem.data_ptr() % 256 == 0
        mem.fill_(FILL)
        at, self.regions = 0, []
        for (r, n), (_, row, stride, extent) in zip(shapes, self.geo):
            off = 256 + mis
            span = (extent + item - 1) // item * item
            length = (off + span + 256 + 255) // 256 * 256
            typed = mem[at + off:at + off + span].view(tdt)
            self.views.append(torch.as_strided(typed, (r, n), (stride // item, 1)))
            self.off.append(off)
            self.regions.append((at, length))
            at += length
        assert at <= mem.numel()

    def check(self, want, what):
        host = self.mem[:sum(l for _, l in self.regions)].cpu().numpy()
        S.check_planes([host[a:a + l] for a, l in self.regions], self.off, self.geo, want, what)


def _rec(bd, **kw):
    rec = vvdec_amd.Reconstructor(S.W, S.H_, bit_depth=bd, chroma_format=1, num_slots=2, num_streams=1, **kw)
    return rec


def matrix_on_the_device(bd, fmt):
    import film_grain_ref
    import test_film_grain_host as H
    rec = _rec(bd)
    L, ctx = rec.L, rec.ctx
    rng = np.random.default_rng(60 + bd)
    picture = film_grain_ref.grain_picture(rng, S.W, S.H_, bd, 1)
    rec.write_picture(0, picture)
    if bd != 9:
        rec.set_film_grain(H._bank(rng))
    rec.enable_stats()
    own = rec.device_array(1 << 20)
    mems = {"tensor": torch.empty(1 << 20, dtype=torch.uint8, device="cuda"), "vvr_device_alloc": own}
    registered = []

    def device(L_, ctx_, slot, win, fmt_, ncomp, want, what, seed, size, grain, stride_kind, mis):
        for name, mem in mems.items():
            d = TensorPlanes(mem, win, fmt_, size, stride_kind, mis)
            rec.set_film_grain_seed(seed)
            t = rec.output_submit(slot, window=win, fmt=fmt_, size=size, grain=grain, into=d.views)
            registered.append(len(rec._reg[t]))
            got = rec.output_wait(t)
            assert got is not None and len(got) == 2 and got[0] is d.views[0]
            d.check(want, "%s (%s)" % (what, name))
            for v in d.views:          # (unregistered by output_wait; memory of the context never was registered by the caller)
                assert L.vvr_device_unregister(ctx, v.data_ptr()) == abi.VVR_ERR_PARAMETER

    S.check_matrix(L, ctx, picture, bd, fmt, device=device)
    assert set(registered) == {0, 2}, "tensors are registered for the life of the request, memory of vvr_device_alloc is known already"
    assert any(s["name"] == "k_output_frame" and s["launches"] > 0 for s in rec.stats()), "vvr_get_stats does not name k_output_frame"
    rec.close()


def a_4k_frame_direct_and_laid_out():
    """3840x2160, 10 bits, the frame and a window at an offset as P010: into contiguous tensors (k_output_frame stores straight into them) and into
    views with padded rows (scratch, then one device-to-device copy per plane), against the picture that was written"""
    Wk, Hk = 3840, 2160
    rng = np.random.default_rng(61)
    planes = [rng.integers(0, 1 << 10, (Hk >> s, Wk >> s), dtype=np.uint16) for s in (0, 1, 1)]
    rec = vvdec_amd.Reconstructor(Wk, Hk, bit_depth=10, num_slots=1, num_streams=1)
    rec.write_picture(0, planes)
    for win in [(0, 0, Wk, Hk), (2, 4, 3824, 2152)]:
        want = S.semi(S.crop(planes, win), "p010", 10)
        shapes, _ = abi.output_plane_shapes(win, "p010", None, 3)
        for pad in (0, 24):
            full = [torch.full((r, n + pad), -1, dtype=torch.int16, device="cuda") for r, n in shapes]
            into = [f[:, :n] for f, (r, n) in zip(full, shapes)]
            assert all(t.is_contiguous() == (pad == 0) for t in into)
            torch.cuda.synchronize()       # (the fill runs on torch's stream, the request on the context's: a destination must be idle when it is submitted)
            got = rec.output_wait(rec.output_submit(0, window=win, fmt="p010", into=into))
            for k in range(2):
                host = full[k].cpu().numpy().view(np.uint16)
                assert np.array_equal(host[:, :shapes[k][1]], want[k]), "%r pad %d plane %d: %d samples differ" % (win, pad, k, int((host[:, :shapes[k][1]] != want[k]).sum()))
                assert (host[:, shapes[k][1]:] == 0xffff).all(), "wrote beyond the row"
    rec.close()


def frames_consumed_on_the_gpu_without_the_host_waiting():
    """a GOP and the first pictures of the next one (which overwrite the first GOP's slots: the slot protection is at work), every picture's P010
    output requested into its own tensors the moment the picture is submitted; a side stream waits for each request on the device
    (output_stream_wait) and clones the tensors; the host waits for nothing until the side stream is synchronised at the end.  The clones are the
    numpy P010 form of the same pictures decoded with plain waits."""
    Wd, Hd = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = G._decoded_with_plain_waits(plans, nslots, Wd, Hd, [991, 992])
    order = [(0, n) for n in range(len(plans))] + [(1, n) for n in range(3)]       # eight requests: the ring
    slots = [plans[n].slot for _, n in order]
    assert len(set(slots)) < len(slots), "no slot is reused"
    rec = vvdec_amd.Reconstructor(Wd, Hd, num_slots=nslots, num_streams=2, host_threads=2, **G.GEO)
    side = torch.cuda.Stream()
    shapes, _ = abi.output_plane_shapes((0, 0, Wd, Hd), "p010", None, 3)
    jobs, tickets, clones = [], [], []
    for g, n in order:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(plans[n], Wd, Hd, seed=991 + g, tool_flags=G.TOOLS, **G.GEO)))
        into = [torch.empty(s, dtype=torch.int16, device="cuda") for s in shapes]
        tickets.append(rec.output_submit(plans[n].slot, job=jobs[-1], fmt="p010", into=into))
        rec.output_stream_wait(tickets[-1], side)
        with torch.cuda.stream(side):
            clones.append([t.clone() for t in into])
    side.synchronize()
    for (g, n), c in zip(order, clones):
        w_ = S.semi(want[g][n], "p010", 10)
        for k in range(2):
            got = c[k].cpu().numpy().view(np.uint16)
            assert np.array_equal(got, w_[k]), "GOP %d picture %d plane %d: %d samples differ" % (g, n, k, int((got != w_[k]).sum()))
    for t in tickets:
        rec.output_wait(t)
    for j in jobs:
        rec.wait(j)
    rec.close()


def main(names):
    for name in names:
        try:
            if name.startswith("matrix-"):
                _, bd, fmt = name.split("-")
                matrix_on_the_device(int(bd), fmt)
            else:
                {"4k": a_4k_frame_direct_and_laid_out, "gop": frames_consumed_on_the_gpu_without_the_host_waiting}[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
