"""What the tests of the output stage share (tests/test_output_*_host.py on the stand-in runtime of tests/hoststub, tests/test_gpu_output*.py on the
device): the two libraries, contexts and pictures, the probe that compares the ctypes mirrors of vvdec_amd/abi.py with include/vvr.h, the
registry of request kinds and the scenarios that are the same for every kind.  Every helper takes a library and a context, so one set of cases
runs on both."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import compare_ref
import test_host_glue as T
from vvdec_amd import abi

FILL = 0xaa


# ---- libraries

@functools.lru_cache(maxsize=None)
def stub_lib():
    """the product's host code on the stand-in runtime (it compiles vvr_api.cpp itself: the same vvr_* names, bound by the same call), with the
    vvt_* entry points of tests/hoststub that take or return more than ints"""
    L = abi.bind(C.CDLL(T.build_stub()))
    L.vvt_take_h2d.argtypes = [C.c_void_p, C.c_void_p]
    L.vvt_compare_scaled_geometry.restype = None
    L.vvt_compare_scaled_geometry.argtypes = [C.c_int] * 5 + [C.c_void_p]
    return L


def product_lib():
    import vvdec_amd
    return vvdec_amd.lib()


# ---- contexts and pictures

def make_ctx(L, W, H, bit_depth, chroma_format, slots=2, lanes=1, threads=0):
    cfg = abi.Config()
    cfg.abi_version = abi.VVR_ABI_VERSION
    cfg.device, cfg.max_width, cfg.max_height = 0, W, H
    cfg.chroma_format, cfg.bit_depth, cfg.log2_ctu = chroma_format, bit_depth, 7
    cfg.num_slots, cfg.num_streams, cfg.host_threads = slots, lanes, threads
    ctx = C.c_void_p()
    assert L.vvr_create(C.byref(cfg), C.byref(ctx)) == abi.VVR_OK
    return ctx


def stream_ctx(L, W, H, nslots, lanes=2, threads=2):
    """a 10-bit 4:2:0 context that decodes a small stream: lanes and worker threads"""
    return make_ctx(L, W, H, 10, 1, nslots, lanes, threads)


def write_picture(L, ctx, slot, planes):
    for c, p in enumerate(planes):
        p = np.ascontiguousarray(p, np.uint16)
        assert L.vvr_write_plane(ctx, slot, c, p.ctypes.data, p.shape[1]) == abi.VVR_OK


def writer(L):
    return lambda ctx, slot, planes: write_picture(L, ctx, slot, planes)


def random_planes(rng, W, H_, bd, cf):
    """random over the full range, with 0 and 2^bd - 1 in every plane"""
    planes = [rng.integers(0, 1 << bd, (H_ >> s, W >> s), dtype=np.uint16) for s in ((0, 1, 1) if cf else (0,))]
    for p in planes:
        p[0, 0], p[-1, -1] = 0, (1 << bd) - 1
    return planes


def ctx_with(L, size, bd, cf, seed):
    """a context of `size` (w, h) with random planes in slot 0 -> ctx, the planes"""
    planes = random_planes(np.random.default_rng(seed), size[0], size[1], bd, cf)
    ctx = make_ctx(L, size[0], size[1], bd, cf)
    write_picture(L, ctx, 0, planes)
    return ctx, planes


def padded(plane, dt, pad):
    """the plane as a view of an array whose rows are `pad` elements longer (filled with a value the plane never compares equal to by accident)"""
    a = np.full((plane.shape[0], plane.shape[1] + pad), 0x5b, dt)
    a[:, :plane.shape[1]] = plane
    return a[:, :plane.shape[1]]


def forms(ref):
    """the forms a reference is given in: 2-byte samples at strides above the row; 1-byte samples, when its values fit, at an odd byte stride"""
    out = [("16-bit", [padded(p, np.uint16, k) for p, k in zip(ref, (3, 5, 7))])]
    if all(int(p.max()) <= 255 for p in ref):
        out.append(("8-bit", [padded(p, np.uint8, 1 if p.shape[1] % 2 == 0 else 2) for p in ref]))
        assert all(p.strides[0] % 2 == 1 for p in out[-1][1])
    return out


# ---- struct mirrors

def assert_mirrors(tmp_path, names, constants=()):
    """sizeof / offsetof of the structs `names` ((C name, ctypes mirror) pairs) as gcc sees include/vvr.h == their mirrors; constants: (C name,
    value) pairs of integer macros"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vvr.h"', 'int main(void){']
    want = []
    for cname, mirror in names:
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, f[0]) for f in mirror._fields_]
        want += [C.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
    lines += ['printf("%%d\\n", %s);' % cname for cname, _ in constants] + ["return 0;}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(os.path.dirname(T.HERE), "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "probe")]).split()] == want + [v for _, v in constants]


def launches(L, ctx):
    """vvr_get_stats -> {kernel name: launches}"""
    arr = (abi.KernelStat * 32)()
    n = L.vvr_get_stats(ctx, arr, 32)
    return {arr[i].name.decode(): arr[i].launches for i in range(n)}


# ---- the kinds of request the output queue takes, and the scenarios that are the same for each of them

KINDS = {}
HOST_MODULES = {"out": "test_output_queue_host", "hash": "test_output_hash_host", "stats": "test_output_stats_host", "compare": "test_output_compare_host",
                "ssim": "test_output_ssim_host", "msssim": "test_output_msssim_host", "xpsnr": "test_output_xpsnr_host"}
RING_WIN = (8, 4, 200, 64)


class Kind:
    """one kind of request as its module (which keeps its submit / collect / same) registers it.  who: the name its refusals carry, which is the
    name of its submit call.
    ring( L, ctx, planes, win, part, ref, bd ) -> ( submit() -> ( ticket or error, keep ), finish( ticket, keep, what ): vvr_output_wait and the
      result against the expected value ) for the window `win` of the picture `planes` in slot 0, whose planes are `part`, against `ref`.
    stats( L, ctx, planes, bd ) -> ( requests: calls that make one request each and check it, verify( launches ), quiet: one more request ).
    ref_slot( L, ctx, slot, ref_slot, case, ps, pr, bd, what ): the request of `case` with a slot as the reference, against the expected value;
      cases( nc ): the cases.
    failing( L, ctx, slot, win, job, ref_slot ) -> ( ticket, keep ) for a picture of a stream (ref_slot None: a reference of zeros);
      untouched( keep ): nothing was written; delivered( keep ): asserts what the request of the good picture brought."""
    def __init__(self, name, who, ring, stats=None, ref_slot=None, cases=None, failing=None, untouched=None, delivered=None):
        self.name, self.who, self.ring, self.stats, self.ref_slot, self.cases = name, who, ring, stats, ref_slot, cases
        self.failing, self.untouched, self.delivered = failing, untouched, delivered


def register(name, who, ring, **kw):
    KINDS[name] = Kind(name, who, ring, **kw)


def kinds():
    """every kind, in the order of HOST_MODULES (a module registers its kind when it is imported)"""
    import importlib
    for m in HOST_MODULES.values():
        importlib.import_module(m)
    return {name: KINDS[name] for name in HOST_MODULES}


def noisy(planes, bd, seed):
    rng = np.random.default_rng(seed)
    return [np.clip(p.astype(np.int64) + rng.integers(-8, 9, p.shape), 0, (1 << bd) - 1).astype(np.uint16) for p in planes]


def tickets_and_the_ring(first, L, ctx, planes, bd, ext, win=RING_WIN):
    """eight requests in flight that cycle through every kind, `first` first (it has two of them); the ninth of each kind is VVR_ERR_BUSY with the
    kind's name in vvr_last_error; vvr_sync retires nothing; vvr_output_test leaves the tickets; every one of the eight delivers.  ext: a stream
    of the caller's for vvr_output_stream_wait on the requests of `first`"""
    part = compare_ref.window_planes(planes, win)
    ref = noisy(part, bd, 6)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    order = [first] + [k for k in kinds() if k != first]
    made = {k: KINDS[k].ring(L, ctx, planes, win, part, ref, bd) for k in order}
    flight = []
    for n in range(8):
        kind = order[n % len(order)]
        flight.append((kind,) + made[kind][0]())
    assert all(t >= 2 for _, t, _ in flight) and len(set(t for _, t, _ in flight)) == 8, [(k, t, L.vvr_last_error(ctx)) for k, t, _ in flight]
    assert [k for k, _, _ in flight].count(first) == 2
    for kind in order[1:] + [first]:
        t9, _ = made[kind][0]()
        assert t9 == abi.VVR_ERR_BUSY and b"in flight" in L.vvr_last_error(ctx) and KINDS[kind].who in L.vvr_last_error(ctx), (kind, t9, L.vvr_last_error(ctx))
    assert L.vvr_sync(ctx) == abi.VVR_OK
    assert all(L.vvr_output_test(ctx, t) == abi.VVR_OK for _, t, _ in flight)
    for n, (kind, t, keep) in enumerate(flight):
        if kind == first:
            assert L.vvr_output_stream_wait(ctx, t, ext) == abi.VVR_OK
        made[kind][1](t, keep, "request %d of eight (%s)" % (n, kind))
    t = flight[0][1]
    assert L.vvr_output_wait(ctx, t) == abi.VVR_ERR_PARAMETER and b"ticket" in L.vvr_last_error(ctx)


def statistics(kind, L, ctx, planes, bd):
    """vvr_get_stats names the kernels of the kind's requests, and nothing with statistics off"""
    requests, verify, quiet = kinds()[kind].stats(L, ctx, planes, bd)
    assert L.vvr_enable_stats(ctx, 1) == abi.VVR_OK
    for request in requests:
        request()
    verify(launches(L, ctx))
    assert L.vvr_enable_stats(ctx, 0) == abi.VVR_OK
    quiet()
    assert not launches(L, ctx)


def check_ref_slot(kind, L, ctx, write, a, b, bd):
    """two pictures in slots 0 and 1, the kind's measure in both directions at every case"""
    K = kinds()[kind]
    write(ctx, 0, a)
    write(ctx, 1, b)
    for case in K.cases(len(a)):
        win = case[0] if isinstance(case[0], tuple) else case
        pa, pb = compare_ref.window_planes(a, win), compare_ref.window_planes(b, win)
        K.ref_slot(L, ctx, 0, 1, case, pa, pb, bd, "slot 0 against slot 1, %r" % (case,))
        K.ref_slot(L, ctx, 1, 0, case, pb, pa, bd, "slot 1 against slot 0, %r" % (case,))


def small_stream(L, seed=611, **kw):
    """a context and the five pictures of a 256 x 128 stream with the smallest DPB -> ctx, plans, descriptions, the whole window"""
    from vvdec_amd import stream, synth
    Wd, Hd = 256, 128
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    ctx = stream_ctx(L, Wd, Hd, nslots)
    descs = [synth.picture_for_plan(pl, Wd, Hd, seed=seed, tool_flags=T.TOOLS, **kw) for pl in plans]
    return ctx, plans, descs, (0, 0, Wd, Hd)


def a_failed_picture_fails_its_request(kind, L):
    """the second picture of a stream fails on the device: its request fails with it and writes nothing, the request of the first picture
    delivers, and the same request made again after the failure is known is accepted and fails the same way"""
    K = kinds()[kind]
    ctx, plans, descs, win = small_stream(L, p_intra=0.3)
    assert L.vvr_set_output_colour(ctx, 1, 0) == abi.VVR_OK
    pics = [d.c() for d in descs]
    j0 = L.vvr_submit(ctx, C.byref(pics[0]))
    t0, k0 = K.failing(L, ctx, plans[0].slot, win, j0, None)
    assert t0 >= 2
    L.vvt_fail_leaf_waits(1)
    j1 = L.vvr_submit(ctx, C.byref(pics[1]))                         # its intra stage gives up a wait: the job fails when it completes
    t1, k1 = K.failing(L, ctx, plans[1].slot, win, j1, None)
    assert t1 >= 2
    assert L.vvr_output_test(ctx, t1) == abi.VVR_ERR_DEVICE and L.vvr_output_test(ctx, t0) == abi.VVR_OK
    assert L.vvr_output_wait(ctx, t1) == abi.VVR_ERR_DEVICE and b"waited for its neighbours" in L.vvr_last_error(ctx)
    assert K.untouched(k1), "a request that failed writes nothing"
    assert L.vvr_output_wait(ctx, t0) == abi.VVR_OK, L.vvr_last_error(ctx)
    K.delivered(k0)
    t2, k2 = K.failing(L, ctx, plans[1].slot, win, j1, plans[0].slot)      # asked again after the failure is known: accepted, fails the same way
    assert t2 >= 2 and L.vvr_output_wait(ctx, t2) == abi.VVR_ERR_DEVICE and K.untouched(k2)
    L.vvt_fail_leaf_waits(0)
    assert L.vvr_wait(ctx, j1) == abi.VVR_ERR_DEVICE and L.vvr_wait(ctx, j0) == abi.VVR_OK
    L.vvr_destroy(ctx)


def refuser(L, ctx, kind, build):
    """-> refused( text, c = ctx, ** kw ): the request build( ... ) makes - it takes the keywords it names - with the other keywords set as fields
    (strideN, planeN: the reference's; pstrideN, pplaneN: the prev planes'), is refused with VVR_ERR_PARAMETER, `text` and the kind's name"""
    import inspect
    own = set(inspect.signature(build).parameters)
    who = KINDS[kind].who
    call = getattr(L, who.decode())

    def refused(text, c=ctx, **kw):
        req = build(**{k: v for k, v in kw.items() if k in own})
        for k, v in kw.items():
            if k in own:
                continue
            if k.startswith("stride"):
                req.ref_stride_bytes[int(k[6:])] = v
            elif k.startswith("plane"):
                req.ref[int(k[5:])] = v
            elif k.startswith("pstride"):
                req.prev_stride_bytes[int(k[7:])] = v
            elif k.startswith("pplane"):
                req.prev[int(k[6:])] = v
            else:
                setattr(req, k, v)
        rc = call(c, C.byref(req))
        assert rc == abi.VVR_ERR_PARAMETER and text in L.vvr_last_error(c) and who in L.vvr_last_error(c), (kw, rc, L.vvr_last_error(c))
    return refused


def eight_still_fit(L, ctx, submit, finish):
    """the ring is untouched by what went before: eight requests submit( n ) fit, with eight tickets, and finish( ticket, keep ) each"""
    flight = [submit(n) for n in range(8)]
    assert all(t >= 2 for t, _ in flight) and len(set(t for t, _ in flight)) == 8, [t for t, _ in flight]
    for t, keep in flight:
        finish(t, keep)
