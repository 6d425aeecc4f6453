"""GPU helper of tests/test_gpu_output_batch.py (run as a script: argv[1:] = the cases to run, in order; prints "ok <case>" behind each and stops
at the first one that fails).  A process of its own because the destinations are torch tensors: torch brings its own HIP runtime, which has to
be the first one the process initialises (as tests/semiplanar_on_the_device.py explains).

The cases: a (4, 3, 12, 28) float32 tensor and a (4, 12, 28, 4) uint8 tensor as into= of Reconstructor.output_submit_batch ("tensors"); the
destinations of tests/test_output_batch_host.py with torch tensors as the device ranges, each inside a guard region ("destinations"); a torch
stream ordered behind the ticket by vvr_output_stream_wait before it reads the tensor ("stream-wait"); the launch counts ("stats").  Everything
is compared with the restatements of tests/, exactly."""
import os
import sys
import traceback
import numpy as np
import torch                      # first: its HIP runtime is the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vvdec_amd                  # noqa: E402
import resample_ref as R                          # noqa: E402
import test_output_batch_host as B                # noqa: E402
from vvdec_amd import abi                         # noqa: E402

NAMES = {R.AREA: "area", R.TRIANGLE: "triangle", R.CUBIC: "cubic"}


def _rec(bd=10):
    rec = vvdec_amd.Reconstructor(B.W, B.H_, bit_depth=bd, chroma_format=1, num_slots=2, num_streams=1)
    return rec


class Tensor:
    """a device range of tests/test_output_batch_host.py: a uint8 tensor registered with the context"""
    name = "a torch tensor"

    def __init__(self, L, ctx, nbytes):
        self.L, self.ctx = L, ctx
        self.t = torch.full((nbytes,), B.FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()       # (idle before the request: the fill runs on torch's stream)
        self.ptr = self.t.data_ptr()
        assert L.vvr_device_register(ctx, self.ptr, nbytes) == abi.VVR_OK, L.vvr_last_error(ctx)

    def read(self):
        return self.t.cpu().numpy()

    def close(self):
        assert self.L.vvr_device_unregister(self.ctx, self.ptr) == abi.VVR_OK, self.L.vvr_last_error(self.ctx)


def _setup(rec, seed, filt=R.TRIANGLE, norm=None):
    pic = B.picture(10, seed)
    rec.write_picture(0, pic)
    rec.set_output_colour(1, False)
    rec.set_output_resampling(NAMES[filt])
    if norm:
        rec.set_output_normalisation(*norm)
    return pic


def tensors_as_destinations():
    wsize, size, origins = B.SECOND
    rec = _rec()
    pic = _setup(rec, 100, norm=B.NORM)
    into = torch.full((4, 3, 12, 28), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = rec.output_wait(rec.output_submit_batch(0, origins, wsize, "rgbf32", size=size, into=into))
    assert got is into
    want = B.expected(pic, origins, wsize, "rgbf32", R.TRIANGLE, size, 10, norm=B.NORM)
    B.N.same([into.cpu().numpy()], [np.stack([np.stack(w) for w in want])], "a (4, 3, 12, 28) float32 tensor")
    into = torch.full((4, 12, 28, 4), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = rec.output_wait(rec.output_submit_batch(0, origins, wsize, "rgba8", size=size, into=into))
    assert got is into
    want = B.expected(pic, origins, wsize, "rgba8", R.TRIANGLE, size, 10)
    B.N.same([into.cpu().numpy()], [np.stack([w[0].reshape(12, 28, 4) for w in want])], "a (4, 12, 28, 4) uint8 tensor")
    assert rec.L.vvr_device_unregister(rec.ctx, into.data_ptr()) == abi.VVR_ERR_PARAMETER      # (unregistered by output_wait)
    # numpy results: pageable and pinned, stacked on a leading axis
    want = B.expected(pic, origins, wsize, "rgb10a2", R.TRIANGLE, size, 10)
    for pinned in (False, True):
        got = rec.output_wait(rec.output_submit_batch(0, origins, wsize, "rgb10a2", size=size, pinned=pinned))
        B.N.same([got], [np.stack([w[0] for w in want])], "(4, 12, 28) words, pinned %r" % pinned)
    for bad in (torch.zeros((4, 3, 12, 28), dtype=torch.float32), torch.zeros((3, 3, 12, 28), dtype=torch.float32, device="cuda"), torch.zeros((4, 3, 12, 56), dtype=torch.float32, device="cuda")[..., ::2]):
        try:
            rec.output_submit_batch(0, origins, wsize, "rgbf32", size=size, into=bad)
        except ValueError:
            pass
        else:
            assert False, "accepted a tensor of shape %r on %s" % (tuple(bad.shape), bad.device)
    rec.close()


def destinations_on_the_device():
    rec = _rec()
    B.check_destinations(rec.L, rec.ctx, lambda ctx, slot, p: rec.write_picture(slot, p), homes=(None, None, Tensor))
    rec.close()


def a_stream_ordered_behind_the_ticket():
    """vvr_output_stream_wait: a torch stream copies the tensor behind the ticket, with no host wait in between"""
    wsize, size, origins = B.SECOND
    rec = _rec()
    pic = _setup(rec, 101, R.CUBIC)
    into = torch.zeros((4, 3, 12, 28), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    t = rec.output_submit_batch(0, origins, wsize, "rgb8", size=size, into=into)
    rec.output_stream_wait(t, s)
    with torch.cuda.stream(s):
        copy = into.clone()
    s.synchronize()
    want = np.stack([np.stack(w) for w in B.expected(pic, origins, wsize, "rgb8", R.CUBIC, size, 10)])
    B.N.same([copy.cpu().numpy()], [want], "the copy on the stream that waited for the ticket")
    assert rec.output_wait(t) is into
    rec.close()


def launch_counts():
    """the increments of vvr_get_stats do not depend on the number of regions"""
    rec = _rec()
    _setup(rec, 102, R.TRIANGLE)
    rec.enable_stats()

    def launches():
        st = {s["name"]: s["launches"] for s in rec.stats()}
        return st.get("k_output_resample", 0), st.get("k_output_rgb", 0), st.get("k_rescale", 0)

    def delta(run):
        a = launches()
        run()
        b = launches()
        return tuple(y - x for x, y in zip(a, b))
    wsize, size, origins = B.SECOND
    for n in (4, 1, 3):
        d = delta(lambda: rec.output_wait(rec.output_submit_batch(0, origins[:n], wsize, "rgb8", size=size)))
        assert d == (3, 1, 0), (n, d)
    wsize, size, origins = B.TWO_LAUNCH
    rec.set_output_resampling("area")
    single = delta(lambda: rec.output_wait(rec.output_submit(0, window=origins[1] + wsize, fmt="rgb8", size=size)))
    many = delta(lambda: rec.output_wait(rec.output_submit_batch(0, origins, wsize, "rgb8", size=size)))
    assert single == many and single[0] > 0 and single[1] == 1, (single, many)
    wsize, _, origins = B.STRAIGHT
    d = delta(lambda: rec.output_wait(rec.output_submit_batch(0, origins, wsize, "rgb8")))
    assert d == (0, 1, 0), d
    rec.close()


def main(names):
    cases = {"tensors": tensors_as_destinations, "destinations": destinations_on_the_device, "stream-wait": a_stream_ordered_behind_the_ticket, "stats": launch_counts}
    for name in names:
        try:
            cases[name]()
        except BaseException:
            traceback.print_exc()
            print("FAILED %s" % name, flush=True)
            return 1                   # (whatever it was, nothing more is started on the device)
        print("ok %s" % name, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
