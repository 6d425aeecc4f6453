"""GPU: the output queue on the device (k_output_frame, and k_film_grain / k_rescale through it).  The case matrices of tests/test_output_queue_host.py
against the synchronous calls and the application's packing, 3840x2160 and 7680x4320 frames, destinations in memory of vvr_host_alloc, requests
submitted behind pictures that are still being reconstructed, slots that are overwritten while their outputs are on the way (ordered on the
device: nothing here depends on timing), whole streams against the bytes vvdecapp writes with -o x.pyuv, and the kernel's statistics."""
import os
import subprocess

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import test_output_queue_host as Q
from vvdec_amd import abi, stream, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
APP_REF = os.path.join(HERE, "..", "oracle", "_ref", "vvdecapp_ref")


def _ran(L, ctx, name="k_output_frame"):
    arr = (abi.KernelStat * 24)()
    n = L.vvr_get_stats(ctx, arr, 24)
    return sum(arr[i].launches for i in range(n) if arr[i].name.decode() == name)


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_matrix_on_the_device(built, bd, cf):
    L = SUP.product_lib()
    mk = lambda W, H_: SUP.make_ctx(L, W, H_, bd, cf)
    ctx, bank = Q.setup(L, mk, lambda ctx, slot, p: SUP.write_picture(L, ctx, slot, p), np.random.default_rng(bd + cf), bd, cf)
    assert L.vvr_enable_stats(ctx, 1) == abi.VVR_OK
    Q.check_planar(L, ctx, bd, cf)
    Q.check_packed(L, mk, ctx, bd, cf)
    assert _ran(L, ctx) > 0, "vvr_get_stats does not name k_output_frame"
    L.vvr_destroy(ctx)


@pytest.mark.parametrize("size,bd", [((3840, 2160), 10), ((7680, 4320), 10), ((3840, 2160), 8)])
def test_headline_sizes(built, size, bd):
    """whole frames and a window at an offset in every format the bit depth has (8-bit output exists for 8-bit content only), against the
    picture that was written; one request into memory of vvr_host_alloc at a padded stride"""
    L = SUP.product_lib()
    W, H_ = size
    rng = np.random.default_rng(W + bd)
    planes = [rng.integers(0, 1 << bd, (H_ >> s, W >> s), dtype=np.uint16) for s in (0, 1, 1)]
    ctx = SUP.make_ctx(L, W, H_, bd, 1, slots=1)
    SUP.write_picture(L, ctx, 0, planes)
    for n, win in enumerate([(0, 0, W, H_), (2, 4, W - 16, H_ - 8)]):
        if n == 0 and W > 4000:         # (7680x4320: the window at an offset only - the checker's packing of a frame takes a second)
            continue
        x, y, w, h = win
        crop = [p[y >> s:(y + h) >> s, x >> s:(x + w) >> s] for p, s in zip(planes, (0, 1, 1))]
        for fmt in ["planar16", "packed10"] + (["planar8"] if bd == 8 else []):
            want = [Q.pack10(p, bd) for p in crop] if fmt == "packed10" else [p.astype(np.uint8) if fmt == "planar8" else p for p in crop]
            alloc = (lambda nb: L.vvr_host_alloc(ctx, nb)) if n == 1 and fmt != "planar8" else None
            t, outs = Q.submit(L, ctx, 0, win, fmt, 3, alloc=alloc)
            assert t >= 0, L.vvr_last_error(ctx)
            got = Q.collect(L, ctx, t, outs)           # (checks that the padding of every row is untouched)
            for c in range(3):
                assert np.array_equal(got[c], want[c]), "%r %s component %d: %d differ" % (win, fmt, c, int((got[c] != want[c]).sum()))
    L.vvr_destroy(ctx)


GEO = dict(bit_depth=10, chroma_format=1, log2_ctu=6)
TOOLS = abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST


def _decoded_with_plain_waits(plans, nslots, W, H_, seeds):
    """the GOPs of `seeds` one after the other in a context of their own, every picture waited for and read back -> per GOP the list of pictures"""
    import vvdec_amd
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=nslots, num_streams=2, host_threads=2, **GEO)
    out = []
    for seed in seeds:
        pics = []
        for pl in plans:
            rec.wait(rec.decompress_picture(synth.picture_for_plan(pl, W, H_, seed=seed, tool_flags=TOOLS, **GEO)))
            pics.append(rec.read_picture(pl.slot))
        out.append(pics)
    rec.close()
    return out


def test_requests_in_flight_behind_their_pictures(built):
    """every picture's output requested the moment the picture is submitted, before any wait; packed and planar in turn"""
    import vvdec_amd
    W, H_ = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = _decoded_with_plain_waits(plans, nslots, W, H_, [991])[0]
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=nslots, num_streams=2, host_threads=2, **GEO)
    rec.enable_stats()
    flight = []
    for n, pl in enumerate(plans):
        job = rec.decompress_picture(synth.picture_for_plan(pl, W, H_, seed=991, tool_flags=TOOLS, **GEO))
        flight.append((job, rec.output_submit(pl.slot, job=job, fmt="packed10" if n % 2 else "planar16", pinned=n >= 3)))
    for n, (job, t) in enumerate(flight):
        got = rec.output_wait(t)
        for c in range(3):
            w_ = Q.pack10(want[n][c], 10) if n % 2 else want[n][c]
            assert np.array_equal(got[c], w_), "picture %d component %d" % (n, c)
    for job, _ in flight:
        rec.wait(job)
    assert any(s["name"] == "k_output_frame" and s["launches"] == len(plans) for s in rec.stats())
    rec.close()


def test_a_slot_is_not_overwritten_under_a_request(built):
    """two GOPs back to back into the same slots, no host wait in between: the outputs of the first GOP, requested before the second is submitted,
    are the first GOP's pictures (the second GOP's pictures wait for the requests' kernels on the device), the second GOP's are the second's"""
    import vvdec_amd
    W, H_ = 264, 136
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    want = _decoded_with_plain_waits(plans, nslots, W, H_, [991, 992])
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(*want))
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=nslots, num_streams=2, host_threads=2, **GEO)
    jobs, first = [], []
    for pl in plans:
        jobs.append(rec.decompress_picture(synth.picture_for_plan(pl, W, H_, seed=991, tool_flags=TOOLS, **GEO)))
        first.append(rec.output_submit(pl.slot, job=jobs[-1]))
    # (the plan reuses the first picture's slot for the last one inside the GOP as well: every request is submitted before the next picture into
    # its slot is; 8 requests may be in flight, so the last two of the second GOP - nothing overwrites their slots - are asked for after the first GOP's are home)
    second = []
    for n, pl in enumerate(plans):
        job = rec.decompress_picture(synth.picture_for_plan(pl, W, H_, seed=992, tool_flags=TOOLS, **GEO))
        second.append(rec.output_submit(pl.slot, job=job) if n < 3 else job)
    got1 = [rec.output_wait(t) for t in first]
    second[3:] = [rec.output_submit(pl.slot, job=j) for pl, j in zip(plans[3:], second[3:])]
    got2 = [rec.output_wait(t) for t in second]
    for n in range(len(plans)):
        for c in range(3):
            assert np.array_equal(got1[n][c], want[0][n][c]), "first GOP, picture %d component %d" % (n, c)
            assert np.array_equal(got2[n][c], want[1][n][c]), "second GOP, picture %d component %d" % (n, c)
    rec.sync()
    rec.close()


@pytest.mark.parametrize("name,W,H_,bd", [("mini_all_tools_ctu128_384x256", 384, 256, 10), ("mini_inter_tools_ctu128_384x256", 384, 256, 10),
                                          ("mini_all_tools_ctu64_8bit_320x192", 320, 192, 8)])
def test_streams_against_the_applications_packed_output(built, tmp_path, name, W, H_, bd):
    """the frames vvdecapp writes with -o x.yuv, written into slots and sent through the queue as VVR_OUT_PACKED10, concatenated in plane order ==
    the bytes the application writes with -o x.pyuv for the same stream"""
    if not os.path.exists(APP_REF):
        pytest.skip("oracle/_ref/vvdecapp_ref not built (needs /root/reference at build time)")
    import vvdec_amd
    bit = os.path.join(HERE, "bitstreams", name, name + ".bit")
    yuv, pyuv = str(tmp_path / "x.yuv"), str(tmp_path / "x.pyuv")
    for out in (yuv, pyuv):
        subprocess.check_call([APP_REF, "-b", bit, "-t", "1", "-v", "0", "-o", out], stdout=subprocess.DEVNULL, timeout=600)
    raw = np.fromfile(yuv, np.uint16 if bd > 8 else np.uint8)
    want = np.fromfile(pyuv, np.uint8)
    per = W * H_ * 3 // 2
    assert raw.size % per == 0 and raw.size // per > 0 and want.size == raw.size // 4 * 5
    rec = vvdec_amd.Reconstructor(W, H_, bit_depth=bd, num_slots=4, num_streams=1)
    got, flight = [], []
    for n in range(raw.size // per):
        f = raw[n * per:(n + 1) * per].astype(np.uint16)
        planes = [f[:W * H_].reshape(H_, W), f[W * H_:W * H_ * 5 // 4].reshape(H_ // 2, W // 2), f[W * H_ * 5 // 4:].reshape(H_ // 2, W // 2)]
        if len(flight) == 4:                       # (the slot is written by the host: its request has to be home)
            got += [p.tobytes() for p in rec.output_wait(flight.pop(0))]
        rec.write_picture(n % 4, planes)
        flight.append(rec.output_submit(n % 4, fmt="packed10"))
    for t in flight:
        got += [p.tobytes() for p in rec.output_wait(t)]
    rec.close()
    assert b"".join(got) == want.tobytes()
